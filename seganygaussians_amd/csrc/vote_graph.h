// vote_graph.h -- the language-segmentation vote graph: mask features, anchor bits, CLIP relevancy (include/mi_vote_graph.h;
// DESIGN.md section 21; reference: prompt_segmenting.ipynb, "Language-driven Segmentation").
//
//   resample     : one lane per (channel, working pixel): the bilinear sample of the render in f64, rounded once to f32, into
//                  Fs [C][h w] (the only O(C h w) buffer).
//   mask sums    : one wave per tile of VG_TILE_ROWS rows x 64 pixels, one lane per pixel column.  Per mask the wave reads the
//                  tile's words (a tile the mask misses costs one ballot), forms per pixel w = 1 / max(|g * f|, 1e-12) over all
//                  channels, then in chunks of VG_CHUNK channels the sums of w f over the tile; both in f64.  It writes, per
//                  (mask, tile), the exact pixel count and C f64 sums.  The gate multiplies the sum once, in finalize.
//   finalize     : one workgroup per mask, one thread per channel: adds the tile partials in tile order, applies the gate,
//                  divides by (n + 1e-9) and normalises.  No atomics anywhere: the same inputs give the same bits.
//   anchor bits  : one wave per 32 masks x 32 anchors.  num = sum_c (g phi)_mc a_ac and den = sum_c g_mc^2 a_ac^2 on the exact
//                  f32 matrix instruction (v_mfma_f32_32x32x2_f32), operands straight from global memory into registers; a
//                  __ballot over an accumulator register is two finished words of the pack_bits layout.  (M, A) values never
//                  reach memory.
//   popcount     : one wave per row of words, integer sums.
//   relevancy    : one wave per VG_CR_ROWS rows held in registers; norm and the P + Q dot products accumulate in f64 (a product
//                  of two f32 is exact there), butterfly reductions in a fixed lane order, then the logistic.
#pragma once

#include "wave.h"

namespace mirast {

constexpr int VG_THREADS = 256;
constexpr int VG_TILE_ROWS = 16;
constexpr int VG_CHUNK = 16;       // channels per accumulation pass of the mask sums
constexpr int VG_MASK_GROUP = 4;   // masks per workgroup of the mask sums
constexpr int VG_CR_ROWS = 4;      // rows per wave of the relevancy kernel
constexpr int VG_CR_SLOTS = 16;    // 64 lanes x 16 = 1024 = MI_VOTE_MAX_EMBED_DIM

// ---- resample: Fs[c][y w + x] = bilinear sample of rendered (C, H, W), align_corners=False ---------------------------------------
__device__ inline void vg_taps(double scale, int dst, int in_size, int& i0, int& i1, double& lam)
{
    double src = ((double)dst + 0.5) * scale - 0.5;
    src = src < 0.0 ? 0.0 : src;
    i0 = min((int)floor(src), in_size - 1);
    i1 = min(i0 + 1, in_size - 1);
    lam = src - (double)i0;
}

__global__ void __launch_bounds__(VG_THREADS) vg_resample_kernel(int C, int H, int W, const float* __restrict__ rendered, int h, int w,
                                                                 double scale_h, double scale_w, float* __restrict__ fs)
{
    const size_t i = (size_t)blockIdx.x * VG_THREADS + threadIdx.x;
    const size_t hw = (size_t)h * w;
    if (i >= (size_t)C * hw) return;
    const int c = (int)(i / hw);
    const int p = (int)(i % hw);
    const int y = p / w, x = p % w;
    int y0, y1, x0, x1;
    double ly, lx;
    vg_taps(scale_h, y, H, y0, y1, ly);
    vg_taps(scale_w, x, W, x0, x1, lx);
    const float* plane = rendered + (size_t)c * H * W;
    const double a = plane[(size_t)y0 * W + x0], b = plane[(size_t)y0 * W + x1];
    const double cc = plane[(size_t)y1 * W + x0], d = plane[(size_t)y1 * W + x1];
    const double top = (1.0 - lx) * a + lx * b, bot = (1.0 - lx) * cc + lx * d;
    fs[i] = (float)((1.0 - ly) * top + ly * bot);
}

// ---- mask sums: per (mask, tile) the pixel count and sum_p f_p / max(|g_m * f_p|, 1e-12) -----------------------------------------
// counts [M][T] and sums [M][T][C], T = ceil(h / VG_TILE_ROWS) * Wq tiles; one 64-thread workgroup per (tile, VG_MASK_GROUP masks):
// grid (T, ceil(M / VG_MASK_GROUP)).  sums of a tile whose count is 0 are not written (finalize skips them).
__global__ void __launch_bounds__(64) vg_mask_sums_kernel(int M, int C, int h, int w, int Wq, const uint64_t* __restrict__ eroded,
                                                          const float* __restrict__ fs, const float* __restrict__ gates, int T,
                                                          double* __restrict__ counts, double* __restrict__ sums)
{
    const int t = blockIdx.x;
    const int q = t % Wq, y0 = (t / Wq) * VG_TILE_ROWS;
    const int rows = min(VG_TILE_ROWS, h - y0);
    const int lane = threadIdx.x;
    const int x = min(64 * q + lane, w - 1);   // lanes past the row read its last pixel; their mask bits are 0
    const size_t hw = (size_t)h * w;
    const float* fpix = fs + (size_t)y0 * w + x;
    const int m_end = min(M, ((int)blockIdx.y + 1) * VG_MASK_GROUP);
    for (int m = blockIdx.y * VG_MASK_GROUP; m < m_end; m++) {
        const uint64_t wd = lane < rows ? eroded[((size_t)m * h + y0 + lane) * Wq + q] : 0ull;   // lane r: the word of row y0 + r
        const int n = (int)wave_sum((double)__popcll(wd));
        if (lane == 0) counts[(size_t)m * T + t] = (double)n;
        if (n == 0) continue;   // wave-uniform
        const float* g = gates + (size_t)m * C;
        double wgt[VG_TILE_ROWS];
#pragma unroll
        for (int r = 0; r < VG_TILE_ROWS; r++) {
            const uint64_t wr = __shfl(wd, r);
            wgt[r] = 0.0;
            if (wr == 0ull) continue;   // wave-uniform
            double d = 0.0;
#pragma unroll 8
            for (int c = 0; c < C; c++) {
                const double v = (double)g[c] * (double)fpix[(size_t)c * hw + (size_t)r * w];
                d = fma(v, v, d);
            }
            if ((wr >> lane) & 1ull) wgt[r] = 1.0 / fmax(sqrt(d), 1e-12);
        }
        for (int c0 = 0; c0 < C; c0 += VG_CHUNK) {
            double acc[VG_CHUNK];
#pragma unroll
            for (int j = 0; j < VG_CHUNK; j++) acc[j] = 0.0;
#pragma unroll
            for (int r = 0; r < VG_TILE_ROWS; r++) {
                if (__shfl(wd, r) == 0ull) continue;   // wave-uniform
#pragma unroll
                for (int j = 0; j < VG_CHUNK; j++) {
                    const int c = min(c0 + j, C - 1);
                    acc[j] = fma(wgt[r], (double)fpix[(size_t)c * hw + (size_t)r * w], acc[j]);
                }
            }
            double mine = 0.0;
#pragma unroll
            for (int j = 0; j < VG_CHUNK; j++) {
                const double s = wave_sum(acc[j]);
                mine = lane == j ? s : mine;
            }
            if (lane < VG_CHUNK && c0 + lane < C) sums[((size_t)m * T + t) * C + c0 + lane] = mine;
        }
    }
}

// ---- finalize: one workgroup per mask, one thread per channel, tiles in order ----------------------------------------------------
__global__ void __launch_bounds__(VG_THREADS) vg_mask_finalize_kernel(int C, int T, const double* __restrict__ counts,
                                                                      const double* __restrict__ sums, const float* __restrict__ gates,
                                                                      float* __restrict__ features, long long* __restrict__ out_counts)
{
    __shared__ double red[VG_THREADS];
    const int m = blockIdx.x, c = threadIdx.x;
    const double* cnt = counts + (size_t)m * T;
    double n = 0.0, s = 0.0;
    for (int t = 0; t < T; t++) {
        const double k = cnt[t];
        if (k == 0.0) continue;
        n += k;
        if (c < C) s += sums[((size_t)m * T + t) * C + c];
    }
    s = c < C ? (double)gates[(size_t)m * C + c] * s / (n + 1e-9) : 0.0;
    red[c] = s * s;
    __syncthreads();
    for (int half = VG_THREADS / 2; half > 0; half >>= 1) {
        if (c < half) red[c] += red[c + half];
        __syncthreads();
    }
    if (c < C) features[(size_t)m * C + c] = (float)(s / fmax(sqrt(red[0]), 1e-12));
    if (c == 0 && out_counts) out_counts[m] = (long long)n;
}

// ---- anchor bits ------------------------------------------------------------------------------------------------------------------
// One wave per (32 masks, 32 anchors): D[mask][anchor] = sum_c A[mask][c] B[c][anchor] on v_mfma_f32_32x32x2_f32, twice -- A = g phi,
// B = a for the numerator and A = g^2, B = a^2 for the squared norm.  Lane l gives A[l & 31][.] and B[.][l & 31] of a k-step and
// holds D[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31] in register r, so a __ballot over register r is the finished word of row
// (r & 3) + 8 (r >> 2) in its low half and of the row 4 below in its high half.  The order of the contraction is free as long as both
// operands share it: in a step of 32 channels lane half h owns channels 16 h .. 16 h + 15 (k-step t pairs channels t and 16 + t), so
// every lane reads 64 contiguous bytes of its row.  Both products (g phi, a^2, ...) are elementwise and need no other layout.
// grid (ceil(M / 128), words); no LDS, no barrier.  `wide`: C % 4 == 0 and 16-byte aligned tables.
typedef float vg_f32x16 __attribute__((ext_vector_type(16)));

__device__ inline void vg_load16(const float* __restrict__ row, int k, int C, bool wide, float (&v)[16])
{
    if (wide && k + 16 <= C) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float4 q = *(const float4*)(row + k + 4 * i);
            v[4 * i] = q.x, v[4 * i + 1] = q.y, v[4 * i + 2] = q.z, v[4 * i + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++) v[i] = k + i < C ? row[k + i] : 0.f;
    }
}

__global__ void __launch_bounds__(VG_THREADS) vg_anchor_bits_kernel(int M, int A, int C, const float* __restrict__ phi,
                                                                    const float* __restrict__ gates, const float* __restrict__ anchors,
                                                                    float threshold, int words, int wide, int* __restrict__ out)
{
    const int lane = threadIdx.x & 63, col = lane & 31, h = lane >> 5;
    const int m0 = (blockIdx.x * (VG_THREADS / 64) + (threadIdx.x >> 6)) * 32;
    const int word = blockIdx.y;
    if (m0 >= M) return;   // wave-uniform
    const int m = m0 + col, a = 32 * word + col;
    const bool mask_live = m < M, anchor_live = a < A;
    const float* grow = gates + (size_t)min(m, M - 1) * C;
    const float* prow = phi + (size_t)min(m, M - 1) * C;
    const float* arow = anchors + (size_t)min(a, A - 1) * C;
    vg_f32x16 num = {0.f}, den = {0.f};
    for (int k0 = 0; k0 < C; k0 += 32) {
        float g[16], p[16], b[16];
        vg_load16(grow, k0 + 16 * h, C, wide != 0, g);
        vg_load16(prow, k0 + 16 * h, C, wide != 0, p);
        vg_load16(arow, k0 + 16 * h, C, wide != 0, b);
#pragma unroll
        for (int t = 0; t < 16; t++) {
            const float gt = mask_live ? g[t] : 0.f, bt = anchor_live ? b[t] : 0.f;
            num = __builtin_amdgcn_mfma_f32_32x32x2f32(gt * p[t], bt, num, 0, 0, 0);
            den = __builtin_amdgcn_mfma_f32_32x32x2f32(gt * gt, bt * bt, den, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const float v = num[r] / fmaxf(sqrtf(den[r]), 1e-12f);
        const uint64_t bits = __ballot(anchor_live && v > threshold);   // a NaN is not greater
        const int row = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (col == 0 && row < M) out[(size_t)row * words + word] = (int)(uint32_t)(bits >> (32 * h));
    }
}

// one wave per row: counts[m] = the set bits of its words
__global__ void __launch_bounds__(VG_THREADS) vg_popcount_kernel(int M, int words, const int* __restrict__ bits, int* __restrict__ counts)
{
    const int m = blockIdx.x * (VG_THREADS / 64) + (threadIdx.x >> 6);
    if (m >= M) return;   // wave-uniform
    const int lane = threadIdx.x & 63;
    int n = 0;
    for (int i = lane; i < words; i += 64) n += __popc((unsigned)bits[(size_t)m * words + i]);
#pragma unroll
    for (int off = 32; off; off >>= 1) n += __shfl_xor(n, off);   // (not wave.h's wave_sum: the kernel's code would change)
    if (lane == 0) counts[m] = n;
}

// ---- CLIP relevancy ---------------------------------------------------------------------------------------------------------------
// out[n][p] = 1 / (1 + exp(10 (max_q e_n . neg_q - e_n . pos_p))), e_n = row / max(|row|, 1e-12) with normalize, else the row.
template <typename T>
__global__ void __launch_bounds__(VG_THREADS) vg_relevancy_kernel(int N, int D, int P, int Q, const T* __restrict__ embeds,
                                                                  const float* __restrict__ pos, const float* __restrict__ neg,
                                                                  int normalize, float* __restrict__ out)
{
    const int wave = blockIdx.x * (VG_THREADS / 64) + (threadIdx.x >> 6);
    const int n0 = wave * VG_CR_ROWS;
    if (n0 >= N) return;   // wave-uniform
    const int lane = threadIdx.x & 63;
    float e[VG_CR_ROWS][VG_CR_SLOTS];
    double inv[VG_CR_ROWS];
#pragma unroll
    for (int r = 0; r < VG_CR_ROWS; r++) {
        const int n = min(n0 + r, N - 1);
        double ss = 0.0;
#pragma unroll
        for (int i = 0; i < VG_CR_SLOTS; i++) {
            const int d = lane + 64 * i;
            e[r][i] = d < D ? (float)embeds[(size_t)n * D + d] : 0.f;
            ss = fma((double)e[r][i], (double)e[r][i], ss);
        }
        inv[r] = normalize ? 1.0 / fmax(sqrt(wave_sum(ss)), 1e-12) : 1.0;
    }
    double best[VG_CR_ROWS], dot[VG_CR_ROWS];
    // the negatives first (their maximum), then one output per positive
    for (int k = 0; k < Q + P; k++) {
        const float* trow = k < Q ? neg + (size_t)k * D : pos + (size_t)(k - Q) * D;
#pragma unroll
        for (int r = 0; r < VG_CR_ROWS; r++) dot[r] = 0.0;
#pragma unroll
        for (int i = 0; i < VG_CR_SLOTS; i++) {
            if (64 * i >= D) break;   // wave-uniform
            const int d = lane + 64 * i;
            const double tv = d < D ? (double)trow[d] : 0.0;
#pragma unroll
            for (int r = 0; r < VG_CR_ROWS; r++) dot[r] = fma((double)e[r][i], tv, dot[r]);
        }
#pragma unroll
        for (int r = 0; r < VG_CR_ROWS; r++) {
            const double s = wave_sum(dot[r]) * inv[r];
            if (k < Q) {
                best[r] = k == 0 ? s : fmax(best[r], s);
            } else if (lane == 0 && n0 + r < N) {
                out[(size_t)(n0 + r) * P + (k - Q)] = (float)(1.0 / (1.0 + exp(10.0 * (best[r] - s))));
            }
        }
    }
}

}  // namespace mirast
