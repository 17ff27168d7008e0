// viewer.h -- the viewer frame: feature moments for the PCA basis, and the fused display frame (include/mi_viewer.h;
// DESIGN.md section 25; reference: saga_gui.py:547-569, 590-599, 645-659, 701-724).
//
//   moments : a workgroup walks tiles of VIEW_MOM_B rows (tile t, t + gridDim.x, ...).  All 256 threads bring a tile into LDS as
//             [row][channel] (odd stride, channels padded with zeros to a multiple of 32), 8 lanes per row form |f|^2 and scale
//             the row in place, then each wave multiplies the tile into the 32 x 32 output blocks it owns on
//             v_mfma_f32_32x32x2_f32: A[i][k] = u[row k][32 bi + i], B[k][j] = u[row k][32 bj + j], one f32 fmaf chain of
//             VIEW_MOM_B rows per output, added into binary64 registers afterwards.  Only the upper block triangle is computed.
//             C <= 64 has at most 3 blocks, one per wave; above that a wave owns 3 and gridDim.y loops over groups of 12 (the
//             rows are re-read per group).  sum u: thread c adds column c of the tile in binary64.  The partial sums of a
//             workgroup go to the workspace, view_moments_reduce_kernel adds them in a fixed order (16 interleaved slices of
//             the workgroups, then the slices).
//   frame   : seg_image_kernel's layout -- a lane owns VEC adjacent pixels and walks the C planes -- with the row arithmetic of
//             seg_row.h, so mask and score are select's bits; three more fmaf chains per pixel for the PCA image; gates, queries
//             and the basis sit in LDS as broadcasts; the frame leaves as 3 VEC adjacent floats per lane.
#pragma once

#include "../../include/mi_viewer.h"
#include "seg_row.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mirast {

constexpr int VIEW_THREADS = 256;
constexpr int VIEW_MOM_B = 32;        // rows per tile = rows per f32 chain (16 k-steps of the 32x32x2 instruction)
constexpr int VIEW_MOM_STRIDE_MAX = MI_SEGMENT_MAX_CHANNELS + 1;

typedef float view_f32x16 __attribute__((ext_vector_type(16)));

__host__ __device__ constexpr int view_mom_blocks(int C) { return (C + 31) / 32; }
__host__ __device__ constexpr int view_mom_pairs(int C) { return view_mom_blocks(C) * (view_mom_blocks(C) + 1) / 2; }
__host__ __device__ constexpr int view_mom_pairs_per_wave(int C) { return C <= 64 ? 1 : 3; }
// workgroups along the rows: one per tile up to a cap of 4 per CU that also keeps the partial sums under 32 MiB
__host__ __device__ constexpr int view_mom_groups(int n, int C)
{
    const int tiles = (int)(((long long)n + VIEW_MOM_B - 1) / VIEW_MOM_B);
    const int by_bytes = 3072 / view_mom_pairs(C) > 64 ? 3072 / view_mom_pairs(C) : 64;
    const int cap = by_bytes < 1024 ? by_bytes : 1024;
    return tiles < cap ? tiles : cap;
}

struct ViewMomArgs {
    const float* feat;
    const long long* index;   // [n] or nullptr
    long long N;              // rows of the table (the plane stride of the image layout)
    int n, C, layout, pre;
    double* part_gram;        // [G][pairs][16][64]: register r of lane l of the block's accumulator
    double* part_sum;         // [G][32 blocks(C)]
};

template <int PW>
__global__ void __launch_bounds__(VIEW_THREADS) view_moments_kernel(ViewMomArgs a)
{
    __shared__ float su[VIEW_MOM_B * VIEW_MOM_STRIDE_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
    const int nb = view_mom_blocks(a.C), npairs = view_mom_pairs(a.C), CP = 32 * nb, CS = CP + 1;
    int pair[PW], bi[PW], bj[PW];
#pragma unroll
    for (int pi = 0; pi < PW; pi++) {   // pair p of the upper block triangle, rows first: (0,0) (0,1) .. (0,nb-1) (1,1) ..
        pair[pi] = ((int)blockIdx.y * PW + pi) * 4 + wave;
        int i = 0, rem = pair[pi];
        while (i < nb && rem >= nb - i) rem -= nb - i++;
        bi[pi] = i;
        bj[pi] = i + rem;
    }
    double g[PW][16];
#pragma unroll
    for (int pi = 0; pi < PW; pi++)
#pragma unroll
        for (int r = 0; r < 16; r++) g[pi][r] = 0.0;
    double msum = 0.0;
    const int tiles = (int)(((long long)a.n + VIEW_MOM_B - 1) / VIEW_MOM_B);
    const bool wide = a.layout == MI_SEGMENT_POINTS && a.C % 4 == 0 && (uintptr_t)a.feat % 16 == 0;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {   // workgroup-uniform
        __syncthreads();   // the previous tile has been read
        if (a.layout == MI_SEGMENT_POINTS) {
            const int row = tid >> 3, sub = tid & 7;
            const long long r = (long long)t * VIEW_MOM_B + row;
            const bool live = r < a.n;
            const float* p = a.feat + (size_t)(live ? (a.index ? a.index[r] : r) : 0) * a.C;
            float* dst = su + row * CS;
            if (wide) {
                for (int c = 4 * sub; c < CP; c += 32) {
                    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (live && c < a.C) x = *reinterpret_cast<const float4*>(p + c);
                    dst[c] = x.x, dst[c + 1] = x.y, dst[c + 2] = x.z, dst[c + 3] = x.w;
                }
            } else {
                for (int c = sub; c < CP; c += 8) dst[c] = (live && c < a.C) ? p[c] : 0.f;
            }
        } else {
            const int row = tid & 31, sub = tid >> 5;
            const long long r = (long long)t * VIEW_MOM_B + row;
            const bool live = r < a.n;
            const float* p = a.feat + (live ? (a.index ? a.index[r] : r) : 0);
            for (int c = sub; c < CP; c += 8) su[row * CS + c] = (live && c < a.C) ? p[(size_t)c * a.N] : 0.f;
        }
        __syncthreads();
        {   // 8 lanes per row, lane `sub` holds channels 4 sub .. 4 sub + 3 of every 32: u = f * scale in place
            const int row = tid >> 3, sub = tid & 7;
            float* dst = su + row * CS;
            float n1 = 0.f;
            for (int c0 = 4 * sub; c0 < CP; c0 += 32)
#pragma unroll
                for (int i = 0; i < 4; i++) n1 = fmaf(dst[c0 + i], dst[c0 + i], n1);
#pragma unroll
            for (int off = 1; off < 8; off <<= 1) n1 += __shfl_xor(n1, off);
            const float scale = seg_row_scale(n1, 0.f, a.pre, 0);
            for (int c0 = 4 * sub; c0 < CP; c0 += 32)
#pragma unroll
                for (int i = 0; i < 4; i++) dst[c0 + i] *= scale;
        }
        __syncthreads();
        if (blockIdx.y == 0 && tid < a.C)
#pragma unroll 8
            for (int r = 0; r < VIEW_MOM_B; r++) msum += (double)su[r * CS + tid];
#pragma unroll
        for (int pi = 0; pi < PW; pi++) {
            if (pair[pi] >= npairs) continue;   // wave-uniform
            const float* pa = su + h * CS + 32 * bi[pi] + col;
            const float* pb = su + h * CS + 32 * bj[pi] + col;
            view_f32x16 acc = {0.f};
#pragma unroll
            for (int s = 0; s < VIEW_MOM_B / 2; s++)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * s * CS], pb[2 * s * CS], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; r++) g[pi][r] += (double)acc[r];
        }
    }
#pragma unroll
    for (int pi = 0; pi < PW; pi++)
        if (pair[pi] < npairs) {
            double* out = a.part_gram + ((size_t)blockIdx.x * npairs + pair[pi]) * 1024 + lane;
#pragma unroll
            for (int r = 0; r < 16; r++) out[r * 64] = g[pi][r];
        }
    if (blockIdx.y == 0 && tid < CP) a.part_sum[(size_t)blockIdx.x * CP + tid] = msum;
}

// 16 outputs (i, j) per workgroup, 16 threads each: thread `slice` adds the partial sums of workgroups slice, slice + 16, ... in that
// order, thread 0 of the 16 then adds the 16 slices in order and forms mean and cov.  D[i][j] of a block sits in register
// (i & 3) + 4 (i >> 3) of lane j + 32 ((i >> 2) & 1).
constexpr int VIEW_RED_SLICES = 16;
__global__ void __launch_bounds__(VIEW_THREADS) view_moments_reduce_kernel(ViewMomArgs a, int G, double* __restrict__ mean,
                                                                           double* __restrict__ cov)
{
    constexpr int OUTS = VIEW_THREADS / VIEW_RED_SLICES;
    __shared__ double red[3][VIEW_RED_SLICES][OUTS];
    const int o = threadIdx.x % OUTS, slice = threadIdx.x / OUTS;
    const int idx = blockIdx.x * OUTS + o;
    const bool live = idx < a.C * a.C;
    const int i = live ? idx / a.C : 0, j = live ? idx % a.C : 0;
    const int nb = view_mom_blocks(a.C), npairs = view_mom_pairs(a.C), CP = 32 * nb;
    int ii = i, jj = j;
    if (ii / 32 > jj / 32) ii = j, jj = i;   // the lower block triangle is the mirror of the upper one
    const int bi = ii / 32, bj = jj / 32, li = ii % 32, lj = jj % 32;
    const int p = bi * nb - bi * (bi - 1) / 2 + (bj - bi);
    const int slot = ((li & 3) + 4 * (li >> 3)) * 64 + lj + 32 * ((li >> 2) & 1);
    double s = 0.0, si = 0.0, sj = 0.0;
    for (int g = slice; g < G; g += VIEW_RED_SLICES) {
        s += a.part_gram[((size_t)g * npairs + p) * 1024 + slot];
        si += a.part_sum[(size_t)g * CP + i];
        sj += a.part_sum[(size_t)g * CP + j];
    }
    red[0][slice][o] = s, red[1][slice][o] = si, red[2][slice][o] = sj;
    __syncthreads();
    if (!live || slice != 0) return;
    s = si = sj = 0.0;
    for (int k = 0; k < VIEW_RED_SLICES; k++) s += red[0][k][o], si += red[1][k][o], sj += red[2][k][o];
    const double n = (double)a.n, mi = si / n, mj = sj / n;
    cov[idx] = s / n - mi * mj;
    if (j == 0) mean[i] = mi;
}

// ---- the fused frame ---------------------------------------------------------------------------------------------------------------
struct ViewFrameArgs {
    const float* feat;      // [C][N]
    const float* rgb;       // [3][N]
    const float* cluster;   // [3][N] or nullptr
    const float* proj;      // [C][3]
    const float* q;         // [Q][C]
    const float* gates;     // [C] or nullptr
    long long N;
    int C, Q, modes, preview;
    float threshold;
    float* frame;           // [N][3]
    unsigned char* mask;
    float* score;
};

template <int VEC> struct ViewVec;
template <> struct ViewVec<1> { typedef float type; };
template <> struct ViewVec<2> { typedef float2 type; };
template <> struct ViewVec<4> { typedef float4 type; };

template <int VEC>
__device__ inline void view_load(const float* p, float (&x)[VEC])
{
    union {
        typename ViewVec<VEC>::type v;
        float f[VEC];
    } u;
    u.v = *reinterpret_cast<const typename ViewVec<VEC>::type*>(p);
#pragma unroll
    for (int v = 0; v < VEC; v++) x[v] = u.f[v];
}

__device__ inline float view_clamp(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

// the Jet map of saga_gui.py:272-292 at x = 8 s, s clamped to [0, 1] as np.interp clamps: every channel is the difference of two
// ramps of slope 1/2 per knot, and where one ramp moves the other is constant, so each subtraction inside a ramp is exact
__device__ inline void view_jet(float s, float& r, float& g, float& b)
{
    const float x = view_clamp(s, 0.f, 1.f) * 8.f;
    r = view_clamp((x - 3.f) * 0.5f, 0.f, 1.f) - view_clamp((x - 7.f) * 0.5f, 0.f, 0.5f);
    g = view_clamp((x - 1.f) * 0.5f, 0.f, 1.f) - view_clamp((x - 5.f) * 0.5f, 0.f, 1.f);
    b = view_clamp(x * 0.5f + 0.5f, 0.5f, 1.f) - view_clamp((x - 3.f) * 0.5f, 0.f, 1.f);
}

// N % VEC == 0 and features, rgb, cluster_rgb and frame aligned to VEC floats (the host picks VEC).  QT: queries padded to 0, 1, 4
// or 16 columns as in segment.h; PCA: the three projection chains.
template <int VEC, int QT, bool PCA>
__global__ void __launch_bounds__(VIEW_THREADS) view_frame_kernel(ViewFrameArgs a)
{
    constexpr int QA = QT ? QT : 1;
    __shared__ float sq[QT ? MI_SEGMENT_MAX_CHANNELS * QT : 1];
    __shared__ float sg[MI_SEGMENT_MAX_CHANNELS];
    __shared__ float sp[PCA ? MI_SEGMENT_MAX_CHANNELS * 3 : 1];
    if (QT) {   // gates (1 without) and queries as [c][QT], zero beyond Q
        for (int c = threadIdx.x; c < a.C; c += VIEW_THREADS) sg[c] = a.gates ? a.gates[c] : 1.f;
        for (int i = threadIdx.x; i < a.C * QT; i += VIEW_THREADS) {
            const int c = i / QA, k = i % QA;
            sq[i] = k < a.Q ? a.q[(size_t)k * a.C + c] : 0.f;
        }
    }
    if (PCA)
        for (int i = threadIdx.x; i < a.C * 3; i += VIEW_THREADS) sp[i] = a.proj[i];
    __syncthreads();
    const long long n0 = ((long long)blockIdx.x * VIEW_THREADS + threadIdx.x) * VEC;
    if (n0 >= a.N) return;
    float n1[VEC], n2[VEC], d[VEC][QA], pj[VEC][3];
#pragma unroll
    for (int v = 0; v < VEC; v++) {
        n1[v] = n2[v] = 0.f;
#pragma unroll
        for (int k = 0; k < QA; k++) d[v][k] = 0.f;
        pj[v][0] = pj[v][1] = pj[v][2] = 0.f;
    }
    if (QT || PCA) {
        const float* p = a.feat + n0;
#pragma unroll 4
        for (int c = 0; c < a.C; c++, p += a.N) {
            float x[VEC];
            view_load<VEC>(p, x);
#pragma unroll
            for (int v = 0; v < VEC; v++) {
                if constexpr (QT > 0) seg_accumulate<QT>(x[v], sg[c], sq + c * QT, n1[v], n2[v], d[v]);
                else n1[v] = fmaf(x[v], x[v], n1[v]);
                if (PCA) {
#pragma unroll
                    for (int j = 0; j < 3; j++) pj[v][j] = fmaf(x[v], sp[3 * c + j], pj[v][j]);
                }
            }
        }
    }
    float rgb[3][VEC], clu[3][VEC];
    const bool has_cluster = (a.modes & MI_VIEW_CLUSTER) && a.cluster;
    // rgb is shown by "rgb", by "cluster" without a cluster render and by "similarity" without queries: not read otherwise
    const bool need_rgb = (a.modes & MI_VIEW_RGB) || ((a.modes & MI_VIEW_CLUSTER) && !a.cluster) || ((a.modes & MI_VIEW_SIMILARITY) && !QT);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
#pragma unroll
        for (int v = 0; v < VEC; v++) rgb[ch][v] = clu[ch][v] = 0.f;
        if (need_rgb) view_load<VEC>(a.rgb + (size_t)ch * a.N + n0, rgb[ch]);
        if (has_cluster) view_load<VEC>(a.cluster + (size_t)ch * a.N + n0, clu[ch]);
    }
    const int count = __popc((unsigned)a.modes);
    float out[VEC * 3];
#pragma unroll
    for (int v = 0; v < VEC; v++) {
        bool any = false;
        float top = 0.f;
        if constexpr (QT > 0) {
            seg_select<QT>(d[v], seg_row_scale(n1[v], n2[v], MI_SEGMENT_PRE_EPS, 1), a.Q, 1, a.threshold, any, top);
            a.mask[n0 + v] = any ? 1 : 0;
            a.score[n0 + v] = top;
        }
        const bool gate = QT > 0 && a.preview;
        float comp[3], acc[3] = {0.f, 0.f, 0.f}, rs[3];
#pragma unroll
        for (int ch = 0; ch < 3; ch++) rs[ch] = gate ? rgb[ch][v] * (any ? 1.f : 0.f) : rgb[ch][v];
        if (a.modes & MI_VIEW_RGB) {
#pragma unroll
            for (int ch = 0; ch < 3; ch++) acc[ch] += rs[ch];
        }
        if (PCA) {
            const float scale = seg_row_scale(n1[v], 0.f, MI_SEGMENT_PRE_EPS, 0);
#pragma unroll
            for (int ch = 0; ch < 3; ch++) acc[ch] += view_clamp(pj[v][ch] * scale * 0.5f + 0.5f, 0.f, 1.f);
        }
        if (a.modes & MI_VIEW_CLUSTER) {
#pragma unroll
            for (int ch = 0; ch < 3; ch++) acc[ch] += has_cluster ? clu[ch][v] : rs[ch];
        }
        if (a.modes & MI_VIEW_SIMILARITY) {
            if (QT > 0) view_jet(top, comp[0], comp[1], comp[2]);
            else comp[0] = rs[0], comp[1] = rs[1], comp[2] = rs[2];
#pragma unroll
            for (int ch = 0; ch < 3; ch++) acc[ch] += comp[ch];
        }
#pragma unroll
        for (int ch = 0; ch < 3; ch++) out[3 * v + ch] = acc[ch] / (float)count;
    }
    float* dst = a.frame + 3 * n0;
    if (VEC == 4) {
#pragma unroll
        for (int i = 0; i < 3; i++) reinterpret_cast<float4*>(dst)[i] = make_float4(out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]);
    } else if (VEC == 2) {
#pragma unroll
        for (int i = 0; i < 3; i++) reinterpret_cast<float2*>(dst)[i] = make_float2(out[2 * i], out[2 * i + 1]);
    } else {
        dst[0] = out[0], dst[1] = out[1], dst[2] = out[2];
    }
}

}  // namespace mirast
