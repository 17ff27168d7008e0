// photometric.h -- the 3DGS photometric loss, fused L1 + D-SSIM forward and backward (include/mi_photometric.h; DESIGN.md
// section 17; reference: train_scene.py:101-104 with utils/loss_utils.py:17-63).
//
//   forward  : one workgroup per tile of PH_TH x PH_TW pixels of one plane.  The tile of x and of g with its 5-pixel halo goes to LDS
//              (zeros outside the image: the window is not renormalised at the border).  Horizontal pass: the 11-tap sums of
//              x, g, x x, g g, x g for every halo row, to LDS.  Vertical pass: each thread owns one column and PH_ROWS consecutive
//              rows, reads PH_ROWS + 10 values per quantity once and forms its window sums in registers.  Then the SSIM value,
//              |x - g| and -- when a gradient will be asked for -- the three derivative maps; the tile's two sums (f64) go to the
//              workspace.
//   finalize : one workgroup adds the tile partials image by image in a fixed order (f64) and writes the means and the loss.
//   backward : the same tiling.  Each derivative map goes through the same two passes (one map at a time through the same LDS),
//              then grad = go (w_l1 sign(x - g) + w_ssim (conv(Dm) + 2 x conv(D11) + g conv(D12))).  A gather: no atomics.
//
// LDS rows are read with consecutive lanes on consecutive dwords in both passes (the lanes of a wave run along a row), so no
// access has a bank conflict and no row needs padding.
//
// The derivative maps, for the window sums m1 = conv(x), m2 = conv(g), e11 = conv(x x), e12 = conv(x g) at a window centre, with
// A1 = 2 m1 m2 + C1, A2 = 2 s12 + C2, B1 = m1^2 + m2^2 + C1, B2 = s1 + s2 + C2 and ssim = A1 A2 / (B1 B2):
//     Dm  = d ssim / d m1  (all paths) = 2 (m2 (A2 - A1) + m1 ssim (B1 - B2)) / (B1 B2)
//     D11 = d ssim / d e11             = -ssim B1 / (B1 B2)
//     D12 = d ssim / d e12             = 2 A1 / (B1 B2)
// written so that x == g gives Dm = 0 and D12 = -2 D11 bit for bit, hence a gradient of exactly 0 at the maximum of the SSIM.
#pragma once

#include "../../include/mi_photometric.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mirast {

constexpr int PH_THREADS = 256;
constexpr int PH_TW = 64;                      // tile width: one wave per row
constexpr int PH_TH = 32;                      // tile height
constexpr int PH_ROWS = PH_TH / (PH_THREADS / PH_TW);   // 8 rows per thread in the vertical pass
constexpr int PH_R = 5;                        // window radius
constexpr int PH_TAPS = 2 * PH_R + 1;
constexpr int PH_IW = PH_TW + 2 * PH_R;        // 74
constexpr int PH_IH = PH_TH + 2 * PH_R;        // 42
constexpr float PH_C1 = (float)(0.01 * 0.01);     // the reference's Python scalars 0.01 ** 2 and 0.03 ** 2, rounded to binary32 where they meet a
constexpr float PH_C2 = (float)(0.03 * 0.03);     // float tensor

// gaussian(11, 1.5) of the reference: the taps rounded to binary32 and normalised in binary32 (tests/test_photometric_host.py pins
// these to the formula through mi_photo_loss_window)
struct PhWindow {
    float w[PH_TAPS];
};
constexpr PhWindow PH_WINDOW = {{0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.106560p-2f,
                                 0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f}};

// The reference's 2-D window is the outer product of the taps ROUNDED to binary32, so its entries sum to (1 + PH_EXCESS) times those of
// the separable window (PH_EXCESS = -7.0e-9).  On the window sums themselves that is far below an ulp, but the variances cancel:
// s = e - m^2 of the reference's window is s + PH_EXCESS (e - 2 m^2) of the separable one to first order, of the size of an ulp of
// s.  The forward adds that term; without it the SSIM mean of a smooth image is off by more than the reference's own rounding.
constexpr double ph_window_excess()
{
    double rounded = 0.0, exact = 0.0;
    for (int i = 0; i < PH_TAPS; i++)
        for (int j = 0; j < PH_TAPS; j++) {
            rounded += (double)(PH_WINDOW.w[i] * PH_WINDOW.w[j]);
            exact += (double)PH_WINDOW.w[i] * (double)PH_WINDOW.w[j];
        }
    return rounded / exact - 1.0;
}
constexpr float PH_EXCESS = (float)ph_window_excess();

struct PhTile {
    int x0, y0;      // first pixel of the tile
    size_t plane;    // offset of the plane
};

__device__ inline PhTile ph_tile(int H, int W, int tiles_x, int tiles_y)
{
    const int b = (int)blockIdx.x;
    const int per_plane = tiles_x * tiles_y;
    const int p = b / per_plane, t = b - p * per_plane;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    return PhTile{tx * PH_TW, ty * PH_TH, (size_t)p * H * W};
}

// the tile of `src` with its halo, zeros outside the image
__device__ inline void ph_load_halo(const float* __restrict__ src, const PhTile& t, int H, int W, float (*dst)[PH_IW])
{
    for (int i = threadIdx.x; i < PH_IH * PH_IW; i += PH_THREADS) {
        const int r = i / PH_IW, c = i - r * PH_IW;
        const int y = t.y0 - PH_R + r, x = t.x0 - PH_R + c;
        dst[r][c] = (y >= 0 && y < H && x >= 0 && x < W) ? src[t.plane + (size_t)y * W + x] : 0.f;
    }
}

// out[j] = sum_k w[k] col[j + k] for the thread's PH_ROWS rows of column c
__device__ inline void ph_vertical(const float (*h)[PH_TW], int r0, int c, float* out)
{
    float v[PH_ROWS + 2 * PH_R];
#pragma unroll
    for (int i = 0; i < PH_ROWS + 2 * PH_R; i++) v[i] = h[r0 + i][c];
#pragma unroll
    for (int j = 0; j < PH_ROWS; j++) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < PH_TAPS; k++) s = fmaf(PH_WINDOW.w[k], v[j + k], s);
        out[j] = s;
    }
}

// sum of `v` over the workgroup in a fixed order; the result is valid in thread 0
__device__ inline double ph_block_sum(double v, double* scratch /* [PH_THREADS / 64] */)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);   // (__shfl_down, lane 0 only: not wave.h's wave_sum, whose order differs)
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < PH_THREADS / 64; w++) s += scratch[w];
    }
    __syncthreads();
    return s;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------
// SSIM = false: the L1 sum alone (l1_loss on its own), no LDS passes.
template <bool SSIM>
__global__ void __launch_bounds__(PH_THREADS) ph_fwd_kernel(int H, int W, int tiles_x, int tiles_y, const float* __restrict__ img,
                                                            const float* __restrict__ gt, float* __restrict__ maps /* [3][P H W] or NULL */,
                                                            size_t map_stride, double* __restrict__ partials /* [blocks][2] */)
{
    __shared__ float s_x[SSIM ? PH_IH : 1][PH_IW];
    __shared__ float s_g[SSIM ? PH_IH : 1][PH_IW];
    __shared__ float s_h[SSIM ? 5 : 1][SSIM ? PH_IH : 1][PH_TW];
    __shared__ double s_red[PH_THREADS / 64];
    const PhTile t = ph_tile(H, W, tiles_x, tiles_y);
    const int c = threadIdx.x & (PH_TW - 1), r0 = (threadIdx.x / PH_TW) * PH_ROWS;
    const int x = t.x0 + c;
    double sum_l1 = 0.0, sum_ssim = 0.0;

    if (SSIM) {
        ph_load_halo(img, t, H, W, s_x);
        ph_load_halo(gt, t, H, W, s_g);
        __syncthreads();
        for (int i = threadIdx.x; i < PH_IH * PH_TW; i += PH_THREADS) {
            const int r = i / PH_TW, cc = i - r * PH_TW;
            float sx = 0.f, sg = 0.f, sxx = 0.f, sgg = 0.f, sxg = 0.f;
#pragma unroll
            for (int k = 0; k < PH_TAPS; k++) {
                const float a = s_x[r][cc + k], b = s_g[r][cc + k];
                const float wa = PH_WINDOW.w[k] * a, wb = PH_WINDOW.w[k] * b;
                sx = fmaf(PH_WINDOW.w[k], a, sx);
                sg = fmaf(PH_WINDOW.w[k], b, sg);
                sxx = fmaf(wa, a, sxx);
                sgg = fmaf(wb, b, sgg);
                sxg = fmaf(wa, b, sxg);
            }
            s_h[0][r][cc] = sx;
            s_h[1][r][cc] = sg;
            s_h[2][r][cc] = sxx;
            s_h[3][r][cc] = sgg;
            s_h[4][r][cc] = sxg;
        }
        __syncthreads();
        float m1[PH_ROWS], m2[PH_ROWS], e11[PH_ROWS], e22[PH_ROWS], e12[PH_ROWS];
        ph_vertical(s_h[0], r0, c, m1);
        ph_vertical(s_h[1], r0, c, m2);
        ph_vertical(s_h[2], r0, c, e11);
        ph_vertical(s_h[3], r0, c, e22);
        ph_vertical(s_h[4], r0, c, e12);
#pragma unroll
        for (int j = 0; j < PH_ROWS; j++) {
            const int y = t.y0 + r0 + j;
            if (y >= H || x >= W) continue;
            const float m11 = m1[j] * m1[j], m22 = m2[j] * m2[j], m12 = m1[j] * m2[j];
            float s1 = fmaf(-m1[j], m1[j], e11[j]), s2 = fmaf(-m2[j], m2[j], e22[j]), s12 = fmaf(-m1[j], m2[j], e12[j]);
            s1 = fmaf(PH_EXCESS, e11[j] - 2.f * m11, s1);
            s2 = fmaf(PH_EXCESS, e22[j] - 2.f * m22, s2);
            s12 = fmaf(PH_EXCESS, e12[j] - 2.f * m12, s12);
            const float A1 = 2.f * m12 + PH_C1, A2 = 2.f * s12 + PH_C2;
            const float B1 = m11 + m22 + PH_C1, B2 = s1 + s2 + PH_C2;
            const float den = B1 * B2;
            const float ssim = (A1 * A2) / den;
            sum_ssim += (double)ssim;
            sum_l1 += (double)fabsf(s_x[r0 + j + PH_R][c + PH_R] - s_g[r0 + j + PH_R][c + PH_R]);
            if (maps) {
                const float inv = 1.f / den;
                const size_t o = t.plane + (size_t)y * W + x;
                maps[o] = 2.f * ((m2[j] * (A2 - A1) + (m1[j] * ssim) * (B1 - B2)) * inv);
                maps[map_stride + o] = -((ssim * B1) * inv);
                maps[2 * map_stride + o] = 2.f * (A1 * inv);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < PH_ROWS; j++) {
            const int y = t.y0 + r0 + j;
            if (y >= H || x >= W) continue;
            const size_t o = t.plane + (size_t)y * W + x;
            sum_l1 += (double)fabsf(img[o] - gt[o]);
        }
    }
    const double tl = ph_block_sum(sum_l1, s_red);
    const double ts = ph_block_sum(sum_ssim, s_red);
    if (threadIdx.x == 0) {
        partials[2 * (size_t)blockIdx.x] = tl;
        partials[2 * (size_t)blockIdx.x + 1] = ts;
    }
}

// one workgroup: the images one after the other, each thread a strided share of the image's tile partials, then the fixed-order
// workgroup sum.  out = { loss, l1, ssim, l1[0], ssim[0], l1[1], ssim[1], ... }
__global__ void __launch_bounds__(PH_THREADS) ph_finalize_kernel(int images, int blocks_per_image, double per_image_count, double lambda,
                                                                 const double* __restrict__ partials, float* __restrict__ out)
{
    __shared__ double s_red[PH_THREADS / 64];
    double tot_l1 = 0.0, tot_ssim = 0.0;
    for (int b = 0; b < images; b++) {
        const double* p = partials + 2 * (size_t)b * blocks_per_image;
        double l = 0.0, s = 0.0;
        for (int i = threadIdx.x; i < blocks_per_image; i += PH_THREADS) {
            l += p[2 * (size_t)i];
            s += p[2 * (size_t)i + 1];
        }
        const double bl = ph_block_sum(l, s_red);
        const double bs = ph_block_sum(s, s_red);
        if (threadIdx.x == 0) {
            out[3 + 2 * b] = (float)(bl / per_image_count);
            out[4 + 2 * b] = (float)(bs / per_image_count);
            tot_l1 += bl;
            tot_ssim += bs;
        }
    }
    if (threadIdx.x == 0) {
        const double n = per_image_count * (double)images;
        const double l1 = tot_l1 / n, ssim = tot_ssim / n;
        out[0] = (float)((1.0 - lambda) * l1 + lambda * (1.0 - ssim));
        out[1] = (float)l1;
        out[2] = (float)ssim;
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
// grad = go (w_l1 sign(x - g) + w_ssim (conv(Dm) + 2 x conv(D11) + g conv(D12))); go = grad_out[image] or grad_out[0].
// SSIM = false: the L1 term alone (maps unused).
template <bool SSIM>
__global__ void __launch_bounds__(PH_THREADS) ph_bwd_kernel(int H, int W, int tiles_x, int tiles_y, int planes_per_image,
                                                            const float* __restrict__ img, const float* __restrict__ gt,
                                                            const float* __restrict__ maps, size_t map_stride,
                                                            const float* __restrict__ grad_out, int grad_per_image, float w_l1,
                                                            float w_ssim, float* __restrict__ grad)
{
    __shared__ float s_in[SSIM ? PH_IH : 1][PH_IW];
    __shared__ float s_h[SSIM ? PH_IH : 1][PH_TW];
    const PhTile t = ph_tile(H, W, tiles_x, tiles_y);
    const int c = threadIdx.x & (PH_TW - 1), r0 = (threadIdx.x / PH_TW) * PH_ROWS;
    const int x = t.x0 + c;
    float conv[3][PH_ROWS];
    if (SSIM) {
#pragma unroll
        for (int q = 0; q < 3; q++) {
            ph_load_halo(maps + q * map_stride, t, H, W, s_in);
            __syncthreads();
            for (int i = threadIdx.x; i < PH_IH * PH_TW; i += PH_THREADS) {
                const int r = i / PH_TW, cc = i - r * PH_TW;
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < PH_TAPS; k++) s = fmaf(PH_WINDOW.w[k], s_in[r][cc + k], s);
                s_h[r][cc] = s;
            }
            __syncthreads();
            ph_vertical(s_h, r0, c, conv[q]);
        }
    }
    const int image = (int)(blockIdx.x / (unsigned)(tiles_x * tiles_y)) / planes_per_image;
    const float go = grad_out[grad_per_image ? image : 0];
#pragma unroll
    for (int j = 0; j < PH_ROWS; j++) {
        const int y = t.y0 + r0 + j;
        if (y >= H || x >= W) continue;
        const size_t o = t.plane + (size_t)y * W + x;
        const float a = img[o], b = gt[o];
        const float d = a - b;
        float v = w_l1 * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
        if (SSIM) {
            // two separately rounded products: with x == g and conv(D12) = -2 conv(D11) they cancel exactly
            const float s = ((2.f * a) * conv[1][j] + b * conv[2][j]) + conv[0][j];
            v = fmaf(w_ssim, s, v);
        }
        grad[o] = go * v;
    }
}

}  // namespace mirast
