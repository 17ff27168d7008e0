// clip_tiles.h -- the CLIP network's input from packed SAM masks and the uint8 image, and the per-pixel mask index map
// (include/mi_clip_tiles.h; reference: clip_utils/__init__.py:91-191,
// clip_utils/sam_utils.py:99-114, :212-225).
//
//   tiles     : one workgroup per (mask, band of CT_BAND output rows), one thread per output column (column sets of CT_THREADS).
//               The resize is separable.  Each source row of the band's window is staged once -- image bytes as one contiguous
//               segment, a lane per byte, the mask word of each pixel, the byte -> f32(b) / 255.0f through a 256-entry table -- as
//               f32 RGB in LDS, in chunks of CT_CHUNK pixels, so a row of any length goes through the same code.  A thread resamples
//               it along the width for its column (3 f32 in registers, its taps in ascending source column, the accumulators live
//               across the chunks) and adds the result into the band's CT_BAND x 3 output accumulators with the rows' height
//               weights.  The source rows come in ASCENDING order, so every output element is the width-pass values times their
//               height weights summed in ascending source row: the order the tests' bound assumes.  Both tap loops run over the taps
//               the crop gives; nothing bounds them but the crop.  Stores are coalesced along Sw.
//               antialias off: pm_source_taps per axis, a l0 + b l1 along the width and fmaf(t0, wy0, t1 wy1) along the height, the order of
//               PyTorch's CPU upsample_bilinear2d that ms_resize_kernel (mask_scales.h) has too.
//   index map : one wave per word of the image, one lane per pixel.  The lanes fetch the word of 64 masks at once; the masks that
//               have a bit in the word are walked in ascending order and the last that covers a pixel stays.
#pragma once

#include "../../include/mi_clip_tiles.h"
#include "packed_masks.h"

#include <hip/hip_fp16.h>

namespace mirast {

constexpr int CT_THREADS = 256;
constexpr int CT_BAND = 8;        // output rows per workgroup
constexpr int CT_CHUNK = 1024;    // source pixels staged at a time (12 KB of f32 RGB)
static_assert(CT_THREADS == 256, "the byte table is filled by one thread per entry");

struct CtNorm {
    float mean[3], std[3];
};

// one axis of the resize: in -> out samples
struct CtAxis {
    float scale, support, inv;
    int in;
};

__device__ inline CtAxis ct_axis(int in, int out)
{
    CtAxis a;
    a.scale = (float)in / (float)out;   // area_pixel_compute_scale, align_corners=False
    a.support = a.scale >= 1.f ? a.scale : 1.f;
    a.inv = a.scale >= 1.f ? 1.f / a.scale : 1.f;
    a.in = in;
    return a;
}

// _upsample_bilinear2d_aa's span and triangle weight of output index i, in f32 (include/mi_clip_tiles.h states the formulas)
__device__ inline void ct_aa_span(const CtAxis& a, int i, float& center, int& lo, int& hi)
{
    center = a.scale * ((float)i + 0.5f);
    lo = max(0, (int)((center - a.support) + 0.5f));
    hi = min((int)((center + a.support) + 0.5f), a.in);
}

__device__ inline float ct_aa_raw(const CtAxis& a, float center, int j)
{
    return fmaxf(0.f, 1.f - fabsf((((float)j - center) + 0.5f) * a.inv));
}

__device__ inline float ct_aa_total(const CtAxis& a, float center, int lo, int hi)
{
    float total = 0.f;
    for (int j = lo; j < hi; j++) total += ct_aa_raw(a, center, j);
    return total;
}

__device__ inline void ct_store(float* p, float v) { *p = v; }
__device__ inline void ct_store(__half* p, float v) { *p = __float2half_rn(v); }

template <bool AA, typename OutT>
__global__ void __launch_bounds__(CT_THREADS) ct_tiles_kernel(int H, int W, int Wq, const uint64_t* __restrict__ packed,
                                                              const uint8_t* __restrict__ image, const int* __restrict__ rects, int layout,
                                                              float bg, CtNorm nrm, int Sh, int Sw, OutT* __restrict__ tiles)
{
    __shared__ float s_lut[256];            // f32(b) / 255.0f, correctly rounded
    __shared__ float s_row[3 * CT_CHUNK];   // a chunk of the current source row, RGB interleaved as in the image
    __shared__ float s_yw[2][CT_BAND];      // per output row of the band: AA center, total / else wy0, wy1
    __shared__ int s_yi[2][CT_BAND];        //                             AA first tap, end of taps / else the two taps
    const int m = blockIdx.y, r0 = blockIdx.x * CT_BAND, tid = threadIdx.x;
    const int rows = min(CT_BAND, Sh - r0);
    const int X0 = rects[4 * m], Y0 = rects[4 * m + 1], X1 = rects[4 * m + 2], Y1 = rects[4 * m + 3];
    const long long cwl = (long long)X1 - X0, chl = (long long)Y1 - Y0;
    OutT* tile = tiles + (size_t)m * 3 * Sh * Sw;
    if (cwl < 1 || chl < 1 || cwl > MI_CLIP_TILES_MAX_SIDE || chl > MI_CLIP_TILES_MAX_SIDE) {   // uniform over the workgroup
        for (int c = 0; c < 3; c++) {
            const float v = (bg - nrm.mean[c]) / nrm.std[c];
            for (int r = 0; r < rows; r++)
                for (int j = tid; j < Sw; j += CT_THREADS) ct_store(tile + ((size_t)c * Sh + r0 + r) * Sw + j, v);
        }
        return;
    }
    const int cw = (int)cwl, ch = (int)chl;
    int PW = cw, PH = ch, ox = 0, oy = 0;   // the source plane and where the crop sits in it
    if (layout == MI_CLIP_TILES_PAD_SQUARE) {
        PW = PH = max(cw, ch);
        if (ch > cw)
            ox = (PW - cw) / 2;
        else
            oy = (PH - ch) / 2;
    }
    const CtAxis ax = ct_axis(PW, Sw), ay = ct_axis(PH, Sh);
    s_lut[tid] = (float)tid / 255.0f;
    if (tid < CT_BAND) {
        const int r = min(r0 + tid, Sh - 1);
        if (AA) {
            float center;
            int lo, hi;
            ct_aa_span(ay, r, center, lo, hi);
            s_yw[0][tid] = center;
            s_yw[1][tid] = ct_aa_total(ay, center, lo, hi);
            s_yi[0][tid] = lo;
            s_yi[1][tid] = hi;
        } else {
            pm_source_taps(ay.scale, r, PH, s_yi[0][tid], s_yi[1][tid], s_yw[0][tid], s_yw[1][tid]);
        }
    }
    __syncthreads();
    const int ybeg = s_yi[0][0], yend = AA ? s_yi[1][rows - 1] : s_yi[1][rows - 1] + 1;   // the band's window of source rows

    for (int j0 = 0; j0 < Sw; j0 += CT_THREADS) {   // uniform: the staging below is the whole workgroup's
        const int j = j0 + tid;
        const bool live = j < Sw;
        // this column's taps: AA [xa, xb) around xc with the weight sum xt; else xa, xb with the weights xc, xt
        float xc = 0.f, xt = 1.f;
        int xa = 0, xb = 0;
        if (live) {
            if (AA) {
                ct_aa_span(ax, j, xc, xa, xb);
                xt = ct_aa_total(ax, xc, xa, xb);
            } else {
                pm_source_taps(ax.scale, j, PW, xa, xb, xc, xt);
            }
        }
        float acc[CT_BAND][3];
#pragma unroll
        for (int r = 0; r < CT_BAND; r++) acc[r][0] = acc[r][1] = acc[r][2] = 0.f;

        for (int py = ybeg; py < yend; py++) {   // ascending source row
            const int cy = py - oy;
            const bool row_in = cy >= 0 && cy < ch && (long long)Y0 + cy >= 0 && (long long)Y0 + cy < H;
            const size_t Y = row_in ? (size_t)((long long)Y0 + cy) : 0;
            const uint64_t* mrow = packed + ((size_t)m * H + Y) * Wq;
            const uint8_t* irow = image + Y * (size_t)W * 3;
            float t[3] = {0.f, 0.f, 0.f}, u[3] = {0.f, 0.f, 0.f};   // the width pass: AA the sum in t; else tap xa in t, tap xb in u
            for (int c_lo = 0; c_lo < PW; c_lo += CT_CHUNK) {
                const int n = min(CT_CHUNK, PW - c_lo);
                __syncthreads();   // the previous chunk has been read
                for (int e = tid; e < 3 * n; e += CT_THREADS) {
                    const int cx = c_lo + e / 3 - ox;
                    const long long X = (long long)X0 + cx;
                    float v = bg;
                    if (row_in && cx >= 0 && cx < cw && X >= 0 && X < W && pm_bit(mrow, X))
                        v = s_lut[irow[3 * X + e % 3]];
                    s_row[e] = v;
                }
                __syncthreads();
                if (live) {
                    if (AA) {
                        const int a = max(xa, c_lo), b = min(xb, c_lo + n);
                        for (int x = a; x < b; x++) {   // ascending source column
                            const float wgt = ct_aa_raw(ax, xc, x) / xt;
                            const float* v = s_row + 3 * (x - c_lo);
                            t[0] += wgt * v[0];
                            t[1] += wgt * v[1];
                            t[2] += wgt * v[2];
                        }
                    } else {
                        if (xa >= c_lo && xa < c_lo + n) {
                            const float* v = s_row + 3 * (xa - c_lo);
                            t[0] = v[0], t[1] = v[1], t[2] = v[2];
                        }
                        if (xb >= c_lo && xb < c_lo + n) {
                            const float* v = s_row + 3 * (xb - c_lo);
                            u[0] = v[0], u[1] = v[1], u[2] = v[2];
                        }
                    }
                }
            }
            if (!AA) {
#pragma unroll
                for (int c = 0; c < 3; c++) t[c] = t[c] * xc + u[c] * xt;
            }
            // the height pass of this source row into the band's output rows
#pragma unroll
            for (int r = 0; r < CT_BAND; r++) {
                if (r >= rows) continue;
                if (AA) {
                    if (py >= s_yi[0][r] && py < s_yi[1][r]) {
                        const float wgt = ct_aa_raw(ay, s_yw[0][r], py) / s_yw[1][r];
#pragma unroll
                        for (int c = 0; c < 3; c++) acc[r][c] += wgt * t[c];
                    }
                } else {
                    // tap 0 holds t0 until tap 1 arrives (the same row when the taps coincide): fmaf(t0, wy0, t1 wy1)
                    if (py == s_yi[0][r]) {
#pragma unroll
                        for (int c = 0; c < 3; c++) acc[r][c] = t[c];
                    }
                    if (py == s_yi[1][r]) {
#pragma unroll
                        for (int c = 0; c < 3; c++) acc[r][c] = fmaf(acc[r][c], s_yw[0][r], t[c] * s_yw[1][r]);
                    }
                }
            }
        }
        if (live) {
#pragma unroll
            for (int r = 0; r < CT_BAND; r++) {
                if (r >= rows) continue;
#pragma unroll
                for (int c = 0; c < 3; c++)
                    ct_store(tile + ((size_t)c * Sh + r0 + r) * Sw + j, (acc[r][c] - nrm.mean[c]) / nrm.std[c]);
            }
        }
    }
}

// ---- index map: offset + the highest mask index that covers the pixel, -1 where none does ----------------------------------------
__global__ void __launch_bounds__(CT_THREADS) ct_index_map_kernel(int M, int H, int W, int Wq, const uint64_t* __restrict__ packed,
                                                                  int offset, int* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * (CT_THREADS / 64) + (threadIdx.x >> 6);   // one wave per word of the image
    if (i >= (size_t)H * Wq) return;                                                 // wave-uniform
    const int lane = threadIdx.x & 63;
    const int q = (int)(i % Wq);
    const size_t y = i / Wq;
    int idx = -1;
    for (int base = 0; base < M; base += 64) {
        const int mm = base + lane;   // lane k: the word of mask base + k
        const uint64_t wd = mm < M ? packed[((size_t)mm * H + y) * Wq + q] : 0ull;
        uint64_t any = __ballot(wd != 0ull);
        while (any) {                 // ascending mask index: the last one that covers the pixel stays
            const int k = __ffsll((long long)any) - 1;
            any &= any - 1ull;
            if ((__shfl(wd, k) >> lane) & 1ull) idx = base + k;
        }
    }
    const int x = 64 * q + lane;
    if (x < W) out[y * (size_t)W + x] = idx < 0 ? -1 : idx + offset;
}

}  // namespace mirast
