// mask_sets.h -- set operations on bit-packed SAM masks (include/mi_mask_sets.h; DESIGN.md section 23;
// reference: clip_utils/sam_utils.py:123-187 and clip_utils/__init__.py:115, :206, :282, :380).
//
//   overlaps     : a GEMM over bits.  One workgroup per (64 x 64 tile of mask pairs on or above the diagonal, slice of the words).
//                  Per step 64 + 64 mask rows x 32 words are staged in LDS (rows padded to 33 words: the 16 rows a wave reads side by
//                  side fall on 16 different bank pairs), each lane accumulates a 4 x 4 register tile of AND + popcount in int32.
//                  The next step's words are fetched into registers meanwhile.  The slices add the entries on or above the diagonal
//                  into `inter` with integer atomics (exact, order-free); a second launch mirrors them into the lower triangle and
//                  copies the diagonal to the int64 areas.
//   boxes        : one workgroup per mask, one pass over its words: min / max of the rows and columns of the set bits (the column
//                  extremes from the lowest and highest bit of each word) and the popcount, reduced through LDS in a fixed order.
//   nms decision : ONE workgroup, lane j owns column j of the sorted intersection matrix and walks its rows (reads coalesced over
//                  the lanes, the matrix is symmetric): the three column maxima of sam_utils.py:160-165, every float operation
//                  separate and in f32, then the four tests and the three "none passed" fallbacks (__syncthreads_count).
//   score images : a workgroup of 16 waves owns 16 consecutive mask words (1024 pixels), one wave per word, one lane per pixel.  Per
//                  block of 128 masks the (128 x 16)-word slab is staged in LDS with 128-byte row reads -- not M strided 8-byte
//                  loads per word -- next to the masks' scores; a wave finds the masks that touch its word with one ballot per 64
//                  masks and visits only those, in ascending order, every K column from the one read.  No atomics.
#pragma once

#include "../../include/mi_mask_sets.h"
#include "packed_masks.h"

namespace mirast {

// ---- overlaps --------------------------------------------------------------------------------------------------------------------
constexpr int MSET_OV_TILE = 64;      // mask rows / columns per workgroup
constexpr int MSET_OV_CHUNK = 32;     // words staged per step
constexpr int MSET_OV_THREADS = 256;  // 16 x 16 lanes, 4 x 4 pairs each

// the number of tiles on or above the diagonal of a T x T tile grid (the kernel numbers them row by row)
__host__ __device__ inline int mset_upper_tiles(int T) { return T * (T + 1) / 2; }

__device__ inline const uint64_t* mset_row(const uint64_t* __restrict__ packed, const long long* __restrict__ order, int M, size_t NW, int r)
{
    if (r >= M) return nullptr;
    long long m = order ? order[r] : (long long)r;
    return (m >= 0 && m < M) ? packed + (size_t)m * NW : nullptr;   // an index outside the masks reads as an empty mask
}

__global__ void __launch_bounds__(MSET_OV_THREADS) mset_overlap_kernel(int M, size_t NW, size_t words_per_slice,
                                                                       const uint64_t* __restrict__ packed,
                                                                       const long long* __restrict__ order, int* __restrict__ inter)
{
    __shared__ uint64_t sa[MSET_OV_TILE][MSET_OV_CHUNK + 1];
    __shared__ uint64_t sb[MSET_OV_TILE][MSET_OV_CHUNK + 1];
    // tile (tr, tc), tr <= tc, from the linear index of the upper triangle
    const int T = (M + MSET_OV_TILE - 1) / MSET_OV_TILE;
    int tr = 0, left = (int)blockIdx.x;
    while (left >= T - tr) {
        left -= T - tr;
        tr++;
    }
    const int tc = tr + left;
    const int r0 = tr * MSET_OV_TILE, c0 = tc * MSET_OV_TILE;
    const size_t w_begin = (size_t)blockIdx.y * words_per_slice;
    const size_t w_end = w_begin + words_per_slice < NW ? w_begin + words_per_slice : NW;
    const int t = (int)threadIdx.x, ty = t >> 4, tx = t & 15;
    const int lk = t & (MSET_OV_CHUNK - 1), lr = t >> 5;   // staging: word lk of rows lr, lr + 8, ...

    const uint64_t* arow[MSET_OV_TILE / 8];
    const uint64_t* brow[MSET_OV_TILE / 8];
#pragma unroll
    for (int i = 0; i < MSET_OV_TILE / 8; i++) {
        arow[i] = mset_row(packed, order, M, NW, r0 + lr + 8 * i);
        brow[i] = mset_row(packed, order, M, NW, c0 + lr + 8 * i);
    }
    int acc[4][4] = {};
    // the next chunk's words wait in registers while this one is worked on: the loads' latency is hidden behind the popcounts
    uint64_t na[MSET_OV_TILE / 8], nb[MSET_OV_TILE / 8];
    auto fetch = [&](size_t w0) {
        const bool in = w0 + lk < w_end;   // the last chunk of a slice may be partial
#pragma unroll
        for (int i = 0; i < MSET_OV_TILE / 8; i++) {
            na[i] = (in && arow[i]) ? arow[i][w0 + lk] : 0ull;
            nb[i] = (in && brow[i]) ? brow[i][w0 + lk] : 0ull;
        }
    };
    fetch(w_begin);
    for (size_t w0 = w_begin; w0 < w_end; w0 += MSET_OV_CHUNK) {
#pragma unroll
        for (int i = 0; i < MSET_OV_TILE / 8; i++) {
            sa[lr + 8 * i][lk] = na[i];
            sb[lr + 8 * i][lk] = nb[i];
        }
        __syncthreads();
        fetch(w0 + MSET_OV_CHUNK);   // past w_end: zeros, nothing is read
#pragma unroll 4
        for (int k = 0; k < MSET_OV_CHUNK; k++) {
            uint64_t a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                a[i] = sa[ty + 16 * i][k];
                b[i] = sb[tx + 16 * i][k];
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[i][j] += __popcll(a[i] & b[j]);
        }
        __syncthreads();
    }
    // only entries on or above the diagonal are added (16 lanes side by side: 64-byte pieces of a row); the finish kernel mirrors
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int r = r0 + ty + 16 * i, c = c0 + tx + 16 * j;
            if (c < M && r <= c && acc[i][j] != 0) atomicAdd(inter + (size_t)r * M + c, acc[i][j]);
        }
}

// after the slices have added up: the lower triangle from the upper one, and the diagonal as the int64 areas
__global__ void mset_overlap_finish_kernel(int M, int* __restrict__ inter, long long* __restrict__ areas)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)M * M) return;
    const int r = (int)(i / M), c = (int)(i % M);
    if (r > c) inter[i] = inter[(size_t)c * M + r];
    if (r == c && areas) areas[r] = inter[i];
}

// ---- boxes and areas -------------------------------------------------------------------------------------------------------------
constexpr int MSET_BOX_THREADS = 512;

__global__ void __launch_bounds__(MSET_BOX_THREADS) mset_boxes_kernel(int H, int Wq, const uint64_t* __restrict__ packed,
                                                                      float* __restrict__ boxes, long long* __restrict__ areas)
{
    __shared__ int s_min[2][MSET_BOX_THREADS / 64], s_max[2][MSET_BOX_THREADS / 64];
    __shared__ long long s_area[MSET_BOX_THREADS / 64];
    const size_t NW = (size_t)H * Wq;
    const uint64_t* words = packed + (size_t)blockIdx.x * NW;
    int x_min = INT_MAX, y_min = INT_MAX, x_max = -1, y_max = -1;
    long long area = 0;
    for (size_t i = threadIdx.x; i < NW; i += MSET_BOX_THREADS) {
        const uint64_t wd = words[i];
        if (!wd) continue;
        const int y = (int)(i / Wq), x0 = 64 * (int)(i % Wq);
        y_min = min(y_min, y);
        y_max = max(y_max, y);
        x_min = min(x_min, x0 + __ffsll((long long)wd) - 1);
        x_max = max(x_max, x0 + 63 - __clzll((long long)wd));
        area += __popcll(wd);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        x_min = min(x_min, __shfl_xor(x_min, d));
        y_min = min(y_min, __shfl_xor(y_min, d));
        x_max = max(x_max, __shfl_xor(x_max, d));
        y_max = max(y_max, __shfl_xor(y_max, d));
        area += __shfl_xor(area, d);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_min[0][wave] = x_min;
        s_min[1][wave] = y_min;
        s_max[0][wave] = x_max;
        s_max[1][wave] = y_max;
        s_area[wave] = area;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < MSET_BOX_THREADS / 64; v++) {
            x_min = min(x_min, s_min[0][v]);
            y_min = min(y_min, s_min[1][v]);
            x_max = max(x_max, s_max[0][v]);
            y_max = max(y_max, s_max[1][v]);
            area += s_area[v];
        }
        float* box = boxes + 4 * (size_t)blockIdx.x;
        const bool empty = area == 0;
        const float nan = __int_as_float(0x7fc00000);
        box[0] = empty ? nan : (float)x_min;
        box[1] = empty ? nan : (float)y_min;
        box[2] = empty ? nan : (float)x_max;
        box[3] = empty ? nan : (float)y_max;
        if (areas) areas[blockIdx.x] = area;
    }
}

// ---- NMS decision ----------------------------------------------------------------------------------------------------------------
constexpr int MSET_NMS_MAX = 1024;   // one workgroup: a lane per mask
static_assert(MSET_NMS_MAX == PM_MAX_MASKS, "every set of packed masks fits the one workgroup");

// torch.max over a column: a NaN entry makes the maximum NaN
__device__ inline float mset_nanmax(float cur, float v) { return (v > cur || v != v) ? v : cur; }

__global__ void __launch_bounds__(MSET_NMS_MAX) mset_nms_kernel(int M, const int* __restrict__ inter, const long long* __restrict__ areas,
                                                                const float* __restrict__ scores, float iou_thr, float score_thr,
                                                                float inner_max, unsigned char* __restrict__ keep)
{
    __shared__ float s_area[MSET_NMS_MAX];
    __shared__ long long s_iarea[MSET_NMS_MAX];
    const int c = (int)threadIdx.x;
    if (c < M) {
        s_iarea[c] = areas[c];
        s_area[c] = (float)areas[c];
    }
    __syncthreads();
    bool k_iou = false, k_conf = false, k_u = false, k_l = false;
    if (c < M) {
        const float a_c = s_area[c];
        const long long ia_c = s_iarea[c];
        float iou_max = 0.f, in_u = 0.f, in_l = 0.f;
        // rows above the diagonal entry: the pairs (i = r, j = c)
        for (int r = 0; r < c; r++) {
            const int I = inter[(size_t)r * M + c];
            const float fi = (float)I;
            const float ri = fi / s_area[r], rj = fi / a_c;
            const float iou = fi / (float)(s_iarea[r] + ia_c - (long long)I);
            iou_max = mset_nanmax(iou_max, iou);
            if (ri < 0.5f && rj >= 0.85f) {
                const float v = 1.f - rj * ri;
                in_u = mset_nanmax(in_u, v);
                if (r == c - 1) in_l = mset_nanmax(in_l, v);   // tril(..., diagonal=1) keeps the first superdiagonal (:164)
            }
        }
        // rows below: the pairs (i = c, j = r), stored at [j, i] by :156-158
        for (int r = c + 1; r < M; r++) {
            const float fi = (float)inter[(size_t)r * M + c];
            const float ri = fi / a_c, rj = fi / s_area[r];
            if (ri >= 0.85f && rj < 0.5f) in_l = mset_nanmax(in_l, 1.f - rj * ri);
        }
        k_iou = iou_max <= iou_thr;
        k_conf = scores[c] > score_thr;
        k_u = in_u <= inner_max;
        k_l = in_l <= inner_max;
    }
    // :173-181 as meant: a test that no mask passes is switched on for the three best-scored masks
    const bool top = c < 3 && c < M;
    if (__syncthreads_count(k_conf) == 0) k_conf = top;
    if (__syncthreads_count(k_u) == 0) k_u = top;
    if (__syncthreads_count(k_l) == 0) k_l = top;
    if (c < M) keep[c] = (k_iou && k_conf && k_u && k_l) ? 1 : 0;
}

// ---- score images ----------------------------------------------------------------------------------------------------------------
constexpr int MSET_SI_WORDS = 16;                       // words (of 64 pixels) per workgroup: one per wave
constexpr int MSET_SI_THREADS = 64 * MSET_SI_WORDS;
constexpr int MSET_SI_MASKS = 128;                      // masks per staged slab
constexpr int MSET_SI_SUM = 0, MSET_SI_MEAN = 1, MSET_SI_MAX = 2;

template <int KT, int MODE>
__global__ void __launch_bounds__(MSET_SI_THREADS) mset_score_images_kernel(int M, int H, int W, int Wq, int K,
                                                                            const uint64_t* __restrict__ packed,
                                                                            const float* __restrict__ scores, float* __restrict__ out)
{
    __shared__ uint64_t slab[MSET_SI_MASKS][MSET_SI_WORDS + 1];   // rows of 17 words: a column read is free of bank conflicts
    __shared__ float sc[MSET_SI_MASKS][KT];
    const size_t NW = (size_t)H * Wq;
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t wi = (size_t)blockIdx.x * MSET_SI_WORDS + wave;   // this wave's word
    float acc[KT];
#pragma unroll
    for (int k = 0; k < KT; k++) acc[k] = MODE == MSET_SI_MAX ? -INFINITY : 0.f;
    int count = 0;
    for (int m0 = 0; m0 < M; m0 += MSET_SI_MASKS) {
        const int nm = min(MSET_SI_MASKS, M - m0);
        // stage: 16 consecutive lanes read the 16 words (128 bytes) of one mask
        for (int i = t; i < MSET_SI_MASKS * MSET_SI_WORDS; i += MSET_SI_THREADS) {
            const int m = i / MSET_SI_WORDS, r = i % MSET_SI_WORDS;
            const size_t w = (size_t)blockIdx.x * MSET_SI_WORDS + r;
            slab[m][r] = (m < nm && w < NW) ? packed[(size_t)(m0 + m) * NW + w] : 0ull;
        }
        for (int i = t; i < MSET_SI_MASKS * KT; i += MSET_SI_THREADS) {
            const int m = i / KT, k = i % KT;
            sc[m][k] = (m < nm && k < K) ? scores[(size_t)(m0 + m) * K + k] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int half = 0; half < MSET_SI_MASKS / 64; half++) {
            uint64_t touch = __ballot(slab[64 * half + lane][wave] != 0ull);   // the masks with a pixel in this word
            while (touch) {
                const int m = 64 * half + __ffsll((long long)touch) - 1;
                touch &= touch - 1;
                const bool bit = (slab[m][wave] >> lane) & 1ull;
                count += bit ? 1 : 0;
#pragma unroll
                for (int k = 0; k < KT; k++) {
                    const float s = sc[m][k];
                    if (MODE == MSET_SI_MAX)
                        acc[k] = bit ? fmaxf(acc[k], s) : acc[k];
                    else
                        acc[k] = bit ? acc[k] + s : acc[k];
                }
            }
        }
        __syncthreads();
    }
    if (wi >= NW) return;
    const int y = (int)(wi / Wq), x = 64 * (int)(wi % Wq) + lane;
    if (x >= W) return;
    const float n = (float)count;
#pragma unroll
    for (int k = 0; k < KT; k++) {
        float v = acc[k];
        if (MODE == MSET_SI_MEAN) v = count ? v / n : 0.f;
        if (MODE == MSET_SI_MAX) v = count < M ? fmaxf(v, 0.f) : v;   // a mask that misses the pixel contributes 0 (:206)
        if (k < K) out[((size_t)k * H + y) * W + x] = v;
    }
}

}  // namespace mirast
