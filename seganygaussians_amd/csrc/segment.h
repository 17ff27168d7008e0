// segment.h -- scale-gated segmentation queries: scores, selection, cluster assignment (include/mi_segment.h; DESIGN.md section 16;
// reference: saga_gui.py:590-599, 633-659, 673-679, 524-543 and prompt_segmenting.ipynb).
//
// One row arithmetic for everything: a single pass over a feature row accumulates n1 = sum f^2, n2 = sum (f g)^2 and
// d_k = sum (f g) q_k as fmaf chains, and seg_row_scale() turns (n1, n2) into the factor that makes s_k = d_k * scale the
// gated, normalised similarity of the header.  Nothing of the row is kept, so the features are read exactly once.
//
//   stream, image  : a lane owns VEC adjacent pixels (dwordx4 / x2 / x1 loads, by the alignment of N and the base) and walks the
//                    C planes; every load of a wave is one contiguous run of a plane.
//   stream, points : 8 lanes share a row (dwordx4 each when C % 4 == 0, scalar otherwise), a workgroup walks SEG_POINT_ITERS
//                    groups of 32 rows, the partial sums meet in a 3-step __shfl_xor butterfly, lane 0 of the 8 finishes the row.
//                    Gates and queries sit in LDS as [c][k], read as broadcasts.  Serves scores, select and assign with K <= 16:
//                    the epilogue is a wave-uniform switch, so select and assign see the very numbers scores writes.
//   assign, K > 16 : (N x C) . (C x K) on v_mfma_f32_32x32x2_f32 -- an exact f32 fmaf chain, so no operand split is needed.  A wave
//                    keeps 32 gated feature rows as its B fragments (C / 2 registers, rounded up to 16 / 32 / 64 / 128 k-steps), the
//                    centres pass through LDS in blocks of seg_assign_block() rows of odd stride (conflict-free A reads), and
//                    the running (best, label) pair of a row lives in the two lanes that hold its column of the accumulator:
//                    strict > within a lane walks the centres upwards, the two halves meet at the end with the lower index
//                    winning a tie.  The arg-max is taken on d_k (scale > 0 does not move it); best = d * scale.
#pragma once

#include "../../include/mi_segment.h"
#include "seg_row.h"   // seg_row_scale, seg_accumulate, seg_select: shared with viewer.h
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mirast {

constexpr int SEG_THREADS = 256;
constexpr int SEG_POINT_LANES = 8;    // lanes per row, points layout
constexpr int SEG_POINT_ITERS = 8;    // row groups per workgroup: 8 x 32 = 256 rows share one staging of the queries
constexpr int SEG_GEMM_ROWS = 128;    // feature rows per workgroup of the MFMA kernel: 4 waves x 32
constexpr int SEG_GEMM_LDS_FLOATS = 16000;

enum SegMode { SEG_SCORES = 0, SEG_SELECT = 1, SEG_ASSIGN = 2 };

typedef float seg_f32x16 __attribute__((ext_vector_type(16)));

struct SegArgs {
    const float* feat;
    const float* q;        // [Q][C] queries or centres
    const float* gates;    // [C] or nullptr
    long long N;
    int C, Q;              // Q: queries, or centres K
    int pre, post, mode, half_shift;
    float threshold;
    float* out_f;          // scores [Q][N] | score [N] | best [N]
    unsigned char* mask;   // select
    int* labels;           // assign
};

__host__ __device__ constexpr int seg_assign_steps(int C) { return C <= 32 ? 16 : C <= 64 ? 32 : C <= 128 ? 64 : 128; }
__host__ __device__ constexpr int seg_assign_block(int NS)
{
    return SEG_GEMM_LDS_FLOATS / (2 * NS + 1) / 32 * 32 > 512 ? 512 : SEG_GEMM_LDS_FLOATS / (2 * NS + 1) / 32 * 32;
}

template <int QT>
__device__ inline void seg_finish(const SegArgs& a, long long n, float n1, float n2, const float (&d)[QT])
{
    const float scale = seg_row_scale(n1, n2, a.pre, a.post);
    if (a.mode == SEG_SCORES) {
#pragma unroll
        for (int k = 0; k < QT; k++)
            if (k < a.Q) a.out_f[(size_t)k * a.N + n] = d[k] * scale;
    } else if (a.mode == SEG_SELECT) {
        bool any;
        float top;
        seg_select<QT>(d, scale, a.Q, a.half_shift, a.threshold, any, top);
        a.mask[n] = any ? 1 : 0;
        a.out_f[n] = top;
    } else {
        float top = d[0] * scale;
        int label = 0;
#pragma unroll
        for (int k = 1; k < QT; k++)
            if (k < a.Q) {
                const float s = d[k] * scale;
                if (s > top) {
                    top = s;
                    label = k;
                }
            }
        a.labels[n] = label;
        a.out_f[n] = top;
    }
}

// gates (1 without) and queries as [c][QT], zero beyond Q
template <int QT>
__device__ inline void seg_stage_queries(const SegArgs& a, float* __restrict__ sq, float* __restrict__ sg)
{
    for (int c = threadIdx.x; c < a.C; c += SEG_THREADS) sg[c] = a.gates ? a.gates[c] : 1.f;
    for (int i = threadIdx.x; i < a.C * QT; i += SEG_THREADS) {
        const int c = i / QT, k = i % QT;
        sq[i] = k < a.Q ? a.q[(size_t)k * a.C + c] : 0.f;
    }
    __syncthreads();
}

template <int VEC> struct SegVec;
template <> struct SegVec<1> { typedef float type; };
template <> struct SegVec<2> { typedef float2 type; };
template <> struct SegVec<4> { typedef float4 type; };

// ---- streaming, image layout: N % VEC == 0 and the base aligned to VEC floats (the host picks VEC) ---------------------------------
template <int VEC, int QT>
__global__ void __launch_bounds__(SEG_THREADS) seg_image_kernel(SegArgs a)
{
    __shared__ float sq[MI_SEGMENT_MAX_CHANNELS * QT];
    __shared__ float sg[MI_SEGMENT_MAX_CHANNELS];
    seg_stage_queries<QT>(a, sq, sg);
    const long long n0 = ((long long)blockIdx.x * SEG_THREADS + threadIdx.x) * VEC;
    if (n0 >= a.N) return;
    float n1[VEC], n2[VEC], d[VEC][QT];
#pragma unroll
    for (int v = 0; v < VEC; v++) {
        n1[v] = n2[v] = 0.f;
#pragma unroll
        for (int k = 0; k < QT; k++) d[v][k] = 0.f;
    }
    const float* p = a.feat + n0;
#pragma unroll 4
    for (int c = 0; c < a.C; c++, p += a.N) {
        union {
            typename SegVec<VEC>::type v;
            float f[VEC];
        } x;
        x.v = *reinterpret_cast<const typename SegVec<VEC>::type*>(p);
        const float g = sg[c];
#pragma unroll
        for (int v = 0; v < VEC; v++) seg_accumulate<QT>(x.f[v], g, sq + c * QT, n1[v], n2[v], d[v]);
    }
#pragma unroll
    for (int v = 0; v < VEC; v++) seg_finish<QT>(a, n0 + v, n1[v], n2[v], d[v]);
}

// ---- streaming, points layout ------------------------------------------------------------------------------------------------------
template <int QT>
__global__ void __launch_bounds__(SEG_THREADS) seg_points_kernel(SegArgs a, int wide)
{
    __shared__ float sq[MI_SEGMENT_MAX_CHANNELS * QT];
    __shared__ float sg[MI_SEGMENT_MAX_CHANNELS];
    seg_stage_queries<QT>(a, sq, sg);
    constexpr int rows = SEG_THREADS / SEG_POINT_LANES;
    const int sub = threadIdx.x % SEG_POINT_LANES;
    for (int it = 0; it < SEG_POINT_ITERS; it++) {
        const long long base = ((long long)blockIdx.x * SEG_POINT_ITERS + it) * rows;
        if (base >= a.N) break;   // workgroup-uniform
        const long long n = base + threadIdx.x / SEG_POINT_LANES;
        const bool live = n < a.N;
        float n1 = 0.f, n2 = 0.f, d[QT];
#pragma unroll
        for (int k = 0; k < QT; k++) d[k] = 0.f;
        if (live) {
            const float* p = a.feat + (size_t)n * a.C;
            if (wide) {   // C % 4 == 0 and the base 16-byte aligned
#pragma unroll 2
                for (int c = 4 * sub; c < a.C; c += 4 * SEG_POINT_LANES) {
                    const float4 x = *reinterpret_cast<const float4*>(p + c);
                    seg_accumulate<QT>(x.x, sg[c], sq + c * QT, n1, n2, d);
                    seg_accumulate<QT>(x.y, sg[c + 1], sq + (c + 1) * QT, n1, n2, d);
                    seg_accumulate<QT>(x.z, sg[c + 2], sq + (c + 2) * QT, n1, n2, d);
                    seg_accumulate<QT>(x.w, sg[c + 3], sq + (c + 3) * QT, n1, n2, d);
                }
            } else {
                for (int c = sub; c < a.C; c += SEG_POINT_LANES) seg_accumulate<QT>(p[c], sg[c], sq + c * QT, n1, n2, d);
            }
        }
#pragma unroll
        for (int off = 1; off < SEG_POINT_LANES; off <<= 1) {
            n1 += __shfl_xor(n1, off);
            n2 += __shfl_xor(n2, off);
#pragma unroll
            for (int k = 0; k < QT; k++) d[k] += __shfl_xor(d[k], off);
        }
        if (live && sub == 0) seg_finish<QT>(a, n, n1, n2, d);
    }
}

// ---- assign, K > 16: f32 MFMA with the arg-max fused -------------------------------------------------------------------------------
// D[centre][row] = sum_c A[centre][c] B[c][row] on v_mfma_f32_32x32x2_f32: lane l gives A[l & 31][l >> 5] and B[l >> 5][l & 31] of a
// k-step and holds D[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31] in register r.  Channel 2 s + (l >> 5) is k-step s; channels beyond C
// are zero on both sides.
template <int NS, bool IMAGE>
__global__ void __launch_bounds__(SEG_THREADS) seg_assign_mfma_kernel(SegArgs a)
{
    constexpr int CP = 2 * NS, CS = CP + 1, KB = seg_assign_block(NS);
    __shared__ float sc[KB * CS];
    __shared__ float sg[CP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, h = lane >> 5;
    for (int c = tid; c < CP; c += SEG_THREADS) sg[c] = c < a.C ? (a.gates ? a.gates[c] : 1.f) : 0.f;
    __syncthreads();
    const long long n = (long long)blockIdx.x * SEG_GEMM_ROWS + wave * 32 + col;
    const bool live = n < a.N;
    float b[NS];
    float n1 = 0.f, n2 = 0.f;
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const int c = 2 * s + h;
        float f = 0.f;
        if (live && c < a.C) f = IMAGE ? a.feat[(size_t)c * a.N + n] : a.feat[(size_t)n * a.C + c];
        b[s] = f * sg[c];
        n1 = fmaf(f, f, n1);
        n2 = fmaf(b[s], b[s], n2);
    }
    n1 += __shfl_xor(n1, 32);
    n2 += __shfl_xor(n2, 32);
    float top = -INFINITY;
    int label = 0;
    for (int k0 = 0; k0 < a.Q; k0 += KB) {
        const int kb = min(KB, a.Q - k0), kb32 = (kb + 31) & ~31;
        __syncthreads();   // the previous block has been read
        for (int r = wave; r < kb32; r += SEG_THREADS / 64) {
            const float* src = a.q + (size_t)(k0 + r) * a.C;
            for (int c = lane; c < CP; c += 64) sc[r * CS + c] = (r < kb && c < a.C) ? src[c] : 0.f;
        }
        __syncthreads();
        for (int t0 = 0; t0 < kb32; t0 += 32) {
            const float* arow = sc + (t0 + col) * CS + h;
            seg_f32x16 acc = {0.f};
#pragma unroll
            for (int s = 0; s < NS; s++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[2 * s], b[s], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int k = k0 + t0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (k < a.Q && acc[r] > top) {
                    top = acc[r];
                    label = k;
                }
            }
        }
    }
    const float otop = __shfl_xor(top, 32);
    const int olabel = __shfl_xor(label, 32);
    if (otop > top || (otop == top && olabel < label)) {
        top = otop;
        label = olabel;
    }
    if (live && h == 0) {
        a.labels[n] = label;
        a.out_f[n] = top * seg_row_scale(n1, n2, a.pre, 1);
    }
}

}  // namespace mirast
