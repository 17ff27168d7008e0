// mask_scales.h -- SAM-mask 3-D scales: mask erosion and the per-mask point spread (include/mi_mask_scales.h; DESIGN.md section 15;
// reference: get_scale.py:128-159).
//
//   erode (same size) : one lane per output word.  The bilinear resampling is the identity, so "3x3 box sum >= k" is a count of
//                       9 bits: the three rows' west / centre / east bits (neighbour bits across word seams from the adjacent words)
//                       go through a carry-save adder tree, 64 pixels per lane, and the 4-bit count is compared with k bit-sliced
//                       (k = 5, the majority, for mi_mask_erode).
//   erode (resampled) : one wave per output word, one lane per pixel.  Each of the 9 window values is PyTorch's CPU bilinear
//                       interpolation of 4 source bits (upsample_bilinear2d, align_corners=False), summed in f32 in row-major order;
//                       __ballot packs the 64 results.
//   resize            : one wave per output word: the resampled value of the pixel itself > threshold (mi_mask_resize).
//   moments           : one wave per tile of MS_TILE_ROWS rows x 64 pixels.  Each lane holds its pixels' points (f64), the wave
//                       loops over the masks and writes, per mask, the tile's count and sums of x, y, z and |p|^2 (f64).  Tiles a
//                       mask misses cost one ballot; tiles it covers use the tile totals.
//   finalize          : one workgroup per mask adds the tile partials in a fixed order and forms 2 sqrt(var_x + var_y + var_z).
#pragma once

#include "../../include/mi_mask_scales.h"
#include "packed_masks.h"
#include "wave.h"

namespace mirast {

constexpr int MS_THREADS = 256;
constexpr int MS_TILE_ROWS = 16;
constexpr int MS_STATS = 5;   // per (mask, tile): count, sum x, sum y, sum z, sum |p|^2

// ---- erode, same size: bit-sliced "count of the 3x3 window >= k", 0 <= k <= 15 -------------------------------------------------
__global__ void __launch_bounds__(MS_THREADS) ms_erode_same_kernel(int M, int H, int W, int Wq, const uint64_t* __restrict__ in, int k,
                                                                   uint64_t* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= (size_t)M * H * Wq) return;
    const int q = (int)(i % Wq);
    const size_t mrow = i / Wq;   // m H + y
    const int y = (int)(mrow % H);
    uint64_t s[3], c[3];          // per row: the sum bit (weight 1) and the carry bit (weight 2) of west + centre + east
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const int yy = y + r - 1;
        uint64_t ctr = 0, lft = 0, rgt = 0;
        if (yy >= 0 && yy < H) {
            const uint64_t* row = in + (mrow - y + yy) * Wq;
            ctr = row[q];
            if (q > 0) lft = row[q - 1];
            if (q + 1 < Wq) rgt = row[q + 1];
        }
        const uint64_t wst = (ctr << 1) | (lft >> 63);   // bit x = pixel x - 1
        const uint64_t est = (ctr >> 1) | (rgt << 63);   // bit x = pixel x + 1 (padding bits are 0, so the last pixel sees 0)
        s[r] = wst ^ ctr ^ est;
        c[r] = (wst & ctr) | (est & (wst ^ ctr));
    }
    const uint64_t t1 = s[0] ^ s[1] ^ s[2];                                  // weight 1
    const uint64_t u2 = (s[0] & s[1]) | (s[2] & (s[0] ^ s[1]));              // weight 2
    const uint64_t t2 = c[0] ^ c[1] ^ c[2];                                  // weight 2
    const uint64_t u4 = (c[0] & c[1]) | (c[2] & (c[0] ^ c[1]));              // weight 4
    const uint64_t v2 = u2 ^ t2, v4 = u2 & t2;                               // weight 2, 4
    const uint64_t w4 = u4 ^ v4, w8 = u4 & v4;                               // weight 4, 8
    // sum = t1 + 2 v2 + 4 w4 + 8 w8 >= k, from the top bit down: greater where the sum has a bit k lacks and all above agree
    const uint64_t bit[4] = {t1, v2, w4, w8};
    uint64_t gt = 0ull, eq = ~0ull;
#pragma unroll
    for (int b = 3; b >= 0; b--) {
        const uint64_t kb = ((k >> b) & 1) ? ~0ull : 0ull;
        gt |= eq & bit[b] & ~kb;
        eq &= ~(bit[b] ^ kb);
    }
    out[i] = (gt | eq) & pm_valid_bits(W, q);
}

// ---- erode, resampled: PyTorch's CPU bilinear weights (UpSampleKernel.cpp, align_corners=False) --------------------------------
// pm_source_taps (packed_masks.h) states the rounding that makes the resampled values PyTorch's bit for bit.
__global__ void __launch_bounds__(MS_THREADS) ms_erode_resample_kernel(int M, int h, int w, int Wqi, const uint64_t* __restrict__ in,
                                                                       int H, int W, int Wq, float scale_h, float scale_w,
                                                                       float min_sum, uint64_t* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * (MS_THREADS / 64) + (threadIdx.x >> 6);   // one wave per output word
    if (i >= (size_t)M * H * Wq) return;                                             // wave-uniform
    const int lane = threadIdx.x & 63;
    const int q = (int)(i % Wq);
    const size_t mrow = i / Wq;
    const int y = (int)(mrow % H), m = (int)(mrow / H);
    const int x = 64 * q + lane;
    const uint64_t* plane = in + (size_t)m * h * Wqi;
    float box = 0.f;
    if (x < W) {
        for (int dy = -1; dy <= 1; dy++) {
            const int Y = y + dy;
            if (Y < 0 || Y >= H) continue;
            int sy0, sy1;
            float wy0, wy1;
            pm_source_taps(scale_h, Y, h, sy0, sy1, wy0, wy1);
            const uint64_t* r0 = plane + (size_t)sy0 * Wqi;
            const uint64_t* r1 = plane + (size_t)sy1 * Wqi;
            for (int dx = -1; dx <= 1; dx++) {
                const int X = x + dx;
                if (X < 0 || X >= W) continue;
                int sx0, sx1;
                float wx0, wx1;
                pm_source_taps(scale_w, X, w, sx0, sx1, wx0, wx1);
                // the reference's order: the width pass inside, the height pass outside
                const float t0 = (float)pm_bit(r0, sx0) * wx0 + (float)pm_bit(r0, sx1) * wx1;
                const float t1 = (float)pm_bit(r1, sx0) * wx0 + (float)pm_bit(r1, sx1) * wx1;
                box += fmaf(t0, wy0, t1 * wy1);
            }
        }
    }
    const uint64_t word = __ballot(x < W && box >= min_sum);
    if (lane == 0) out[i] = word;
}

// ---- resize: the resampled value alone, against a threshold (clip_utils/__init__.py:99-102) -----------------------------------
// One wave per output word, one lane per pixel, the same taps and the same rounding order as the window values above.
__global__ void __launch_bounds__(MS_THREADS) ms_resize_kernel(int M, int h, int w, int Wqi, const uint64_t* __restrict__ in, int H,
                                                               int W, int Wq, float scale_h, float scale_w, float threshold,
                                                               uint64_t* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * (MS_THREADS / 64) + (threadIdx.x >> 6);   // one wave per output word
    if (i >= (size_t)M * H * Wq) return;                                             // wave-uniform
    const int lane = threadIdx.x & 63;
    const int q = (int)(i % Wq);
    const size_t mrow = i / Wq;
    const int y = (int)(mrow % H), m = (int)(mrow / H);
    const int x = 64 * q + lane;
    bool bit = false;
    if (x < W) {
        int sy0, sy1, sx0, sx1;
        float wy0, wy1, wx0, wx1;
        pm_source_taps(scale_h, y, h, sy0, sy1, wy0, wy1);
        pm_source_taps(scale_w, x, w, sx0, sx1, wx0, wx1);
        const uint64_t* r0 = in + ((size_t)m * h + sy0) * Wqi;
        const uint64_t* r1 = in + ((size_t)m * h + sy1) * Wqi;
        const float t0 = (float)pm_bit(r0, sx0) * wx0 + (float)pm_bit(r0, sx1) * wx1;
        const float t1 = (float)pm_bit(r1, sx0) * wx0 + (float)pm_bit(r1, sx1) * wx1;
        bit = fmaf(t0, wy0, t1 * wy1) > threshold;
    }
    const uint64_t word = __ballot(bit);
    if (lane == 0) out[i] = word;
}

// ---- moments: per (mask, tile) count and f64 sums ----------------------------------------------------------------------------
// partials [M][T][MS_STATS], T = ceil(H / MS_TILE_ROWS) * Wq tiles; one 64-thread workgroup per tile
__global__ void __launch_bounds__(64) ms_moments_kernel(int M, int H, int W, int Wq, const uint64_t* __restrict__ eroded,
                                                        const float* __restrict__ depth, double fx, double fy, int T,
                                                        double* __restrict__ partials)
{
    const int t = blockIdx.x;
    const int q = t % Wq, y0 = (t / Wq) * MS_TILE_ROWS;
    const int rows = min(MS_TILE_ROWS, H - y0);
    const int lane = threadIdx.x;
    const int x = 64 * q + lane;
    const double cx = 0.5 * W, cy = 0.5 * H;
    // get_scale.py:136-143: X pairs the ROW index with cx = W / 2 and fx, Y the column index with cy = H / 2 and fy
    double px[MS_TILE_ROWS], py[MS_TILE_ROWS], pz[MS_TILE_ROWS], pr[MS_TILE_ROWS];
    double tot[MS_STATS] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < MS_TILE_ROWS; r++) {
        double d = 0.0;
        const bool live = r < rows && x < W;
        if (live) d = (double)depth[(size_t)(y0 + r) * W + x];
        px[r] = ((double)(y0 + r) - cx) * d / fx;
        py[r] = ((double)x - cy) * d / fy;
        pz[r] = d;
        pr[r] = px[r] * px[r] + py[r] * py[r] + pz[r] * pz[r];
        if (live) {
            tot[0] += 1.0;
            tot[1] += px[r];
            tot[2] += py[r];
            tot[3] += pz[r];
            tot[4] += pr[r];
        }
    }
#pragma unroll
    for (int k = 0; k < MS_STATS; k++) tot[k] = wave_sum(tot[k]);
    const uint64_t valid = pm_valid_bits(W, q);
    const uint64_t all_rows = (1ull << rows) - 1ull;   // rows <= MS_TILE_ROWS < 64
    for (int m = 0; m < M; m++) {
        const uint64_t wd = lane < rows ? eroded[((size_t)m * H + y0 + lane) * Wq + q] : 0ull;   // lane r: the word of row y0 + r
        const uint64_t any = __ballot(wd != 0ull);
        const uint64_t full = __ballot(lane < rows && wd == valid);
        double st[MS_STATS] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (full == all_rows) {
#pragma unroll
            for (int k = 0; k < MS_STATS; k++) st[k] = tot[k];
        } else if (any) {
#pragma unroll
            for (int r = 0; r < MS_TILE_ROWS; r++) {
                const uint64_t wr = __shfl(wd, r);
                if ((wr >> lane) & 1ull) {
                    st[0] += 1.0;
                    st[1] += px[r];
                    st[2] += py[r];
                    st[3] += pz[r];
                    st[4] += pr[r];
                }
            }
#pragma unroll
            for (int k = 0; k < MS_STATS; k++) st[k] = wave_sum(st[k]);
        }
        double v = st[0];
#pragma unroll
        for (int k = 1; k < MS_STATS; k++) v = lane == k ? st[k] : v;
        if (lane < MS_STATS) partials[((size_t)m * T + t) * MS_STATS + lane] = v;
    }
}

// ---- finalize: one workgroup per mask, fixed-order reduction over the tiles --------------------------------------------------
__global__ void __launch_bounds__(MS_THREADS) ms_finalize_kernel(int T, const double* __restrict__ partials, float* __restrict__ scales,
                                                                 long long* __restrict__ counts)
{
    __shared__ double red[MS_STATS][MS_THREADS];
    const int m = blockIdx.x, tid = threadIdx.x;
    const double* p = partials + (size_t)m * T * MS_STATS;
    double s[MS_STATS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t = tid; t < T; t += MS_THREADS) {
#pragma unroll
        for (int k = 0; k < MS_STATS; k++) s[k] += p[(size_t)t * MS_STATS + k];
    }
#pragma unroll
    for (int k = 0; k < MS_STATS; k++) red[k][tid] = s[k];
    __syncthreads();
    for (int half = MS_THREADS / 2; half > 0; half >>= 1) {
        if (tid < half) {
#pragma unroll
            for (int k = 0; k < MS_STATS; k++) red[k][tid] += red[k][tid + half];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double n = red[0][0];
        float scale = __builtin_nanf("");
        if (n >= 2.0) {
            // sum over the axes of the unbiased variance: (sum |p|^2 - |sum p|^2 / n) / (n - 1)
            const double sx = red[1][0], sy = red[2][0], sz = red[3][0];
            const double var = fmax((red[4][0] - (sx * sx + sy * sy + sz * sz) / n) / (n - 1.0), 0.0);
            scale = (float)(2.0 * sqrt(var));
        }
        scales[m] = scale;
        counts[m] = (long long)n;
    }
}

}  // namespace mirast
