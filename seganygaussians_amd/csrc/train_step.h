// train_step.h -- what follows loss.backward() in the RGB training (train_scene.py:126-138): the Adam step over all parameter
// groups in one launch, the densification statistics in one launch, and densify_and_prune as plan / scan / map / gather kernels
// (DESIGN.md section 18).  Plain loads and stores only: no atomics anywhere, LDS only for the rank of a row inside its workgroup.
// Every result is a function of the inputs alone, so reruns are bit-identical.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "row_compact.h"   // block_rank, the scan of the block counts, the gather: shared with model_edit.h

namespace mirast {

constexpr int TS_THREADS = RC_THREADS;
constexpr int TS_WAVES = RC_WAVES;

// ---- (a) multi-tensor Adam ----------------------------------------------------------------------------------------------------
// A tensor is cut into tiles of TS_THREADS * ADAM_VEC float4 (4096 floats).  The table carries, per tensor, the first tile's global
// number; a workgroup finds the tensor of its tile by walking that table ONCE per tile (uniform, at most 16 scalar compares per 4096
// elements), never per element.  `head` floats come before the first 16-byte boundary of p; g, m and v must share p's offset modulo 16
// for the float4 body, else head = ADAM_SCALAR and the tile is walked float by float.  Tile 0 of a tensor also does head and tail.
constexpr int ADAM_MAX_TENSORS = 16;
constexpr int ADAM_VEC = 4;
constexpr unsigned ADAM_TILE_VEC = TS_THREADS * ADAM_VEC;     // float4 per tile
constexpr unsigned ADAM_TILE = ADAM_TILE_VEC * 4;             // floats per tile
constexpr unsigned ADAM_SCALAR = 0xffffffffu;
constexpr int ADAM_MAX_GRID = 2048;

struct AdamEntry {
    float* p;
    const float* g;
    float* m;
    float* v;
    unsigned long long n;
    float step_size;     // lr / (1 - beta1^t)
    unsigned head;       // 0..3 floats before the float4 body, or ADAM_SCALAR
};

struct AdamTable {
    AdamEntry t[ADAM_MAX_TENSORS];
    unsigned tile_begin[ADAM_MAX_TENSORS + 1];
    int n;
};

struct AdamScalars {
    float inv_sqrt_bc2;   // 1 / sqrt(1 - beta2^t)
    float omb1;           // 1 - beta1, rounded once from double
    float beta2, omb2;    // beta2 and 1 - beta2, each rounded once from double
    float eps;
};

// binary32, every operation rounded on its own (the library is built with -ffp-contract=off)
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float step_size, const AdamScalars& s)
{
    m = m + (g - m) * s.omb1;
    v = s.beta2 * v + (s.omb2 * g) * g;
    p = p - step_size * (m / (sqrtf(v) * s.inv_sqrt_bc2 + s.eps));
}

__device__ __forceinline__ void adam_scalar_at(const AdamEntry& e, unsigned long long i, const AdamScalars& s)
{
    float p = e.p[i], m = e.m[i], v = e.v[i];
    adam_update(p, e.g[i], m, v, e.step_size, s);
    e.p[i] = p;
    e.m[i] = m;
    e.v[i] = v;
}

__global__ void __launch_bounds__(TS_THREADS) adam_kernel(const AdamTable T, const AdamScalars s)
{
    const unsigned total = T.tile_begin[T.n];
    const unsigned tid = threadIdx.x;
    for (unsigned tile = blockIdx.x; tile < total; tile += gridDim.x) {
        int k = 0;
        while (tile >= T.tile_begin[k + 1]) k++;      // an empty tensor owns no tile and is stepped over here
        const AdamEntry e = T.t[k];
        const unsigned long long lt = tile - T.tile_begin[k];
        if (e.head == ADAM_SCALAR) {
            const unsigned long long base = lt * ADAM_TILE;
            for (unsigned j = tid; j < ADAM_TILE; j += TS_THREADS)
                if (base + j < e.n) adam_scalar_at(e, base + j, s);
            continue;
        }
        const unsigned long long nvec = (e.n - e.head) >> 2;
        float4* p4 = reinterpret_cast<float4*>(e.p + e.head);
        const float4* g4 = reinterpret_cast<const float4*>(e.g + e.head);
        float4* m4 = reinterpret_cast<float4*>(e.m + e.head);
        float4* v4 = reinterpret_cast<float4*>(e.v + e.head);
#pragma unroll
        for (int u = 0; u < ADAM_VEC; u++) {
            const unsigned long long c = lt * ADAM_TILE_VEC + (unsigned)u * TS_THREADS + tid;
            if (c < nvec) {
                float4 p = p4[c], m = m4[c], v = v4[c];
                const float4 g = g4[c];
                adam_update(p.x, g.x, m.x, v.x, e.step_size, s);
                adam_update(p.y, g.y, m.y, v.y, e.step_size, s);
                adam_update(p.z, g.z, m.z, v.z, e.step_size, s);
                adam_update(p.w, g.w, m.w, v.w, e.step_size, s);
                p4[c] = p;
                m4[c] = m;
                v4[c] = v;
            }
        }
        if (lt == 0) {      // at most 3 floats before the body and 3 after it
            const unsigned long long tail_begin = e.head + 4 * nvec;
            if (tid < e.head)
                adam_scalar_at(e, tid, s);
            else if (tid >= 4 && tail_begin + (tid - 4) < e.n)
                adam_scalar_at(e, tail_begin + (tid - 4), s);
        }
    }
}

// ---- (b) densification statistics ---------------------------------------------------------------------------------------------
// train_scene.py:126 and scene/gaussian_model.py:582-584 for the rows with radii > 0; every other row is not touched.
__global__ void __launch_bounds__(TS_THREADS) densify_stats_kernel(int P, const int* __restrict__ radii, const float* __restrict__ grad,
                                                                   float* accum, float* denom, float* max_radii)
{
    const int i = blockIdx.x * TS_THREADS + threadIdx.x;
    if (i >= P) return;
    const int r = radii[i];
    if (r <= 0) return;
    const float gx = grad[3 * (size_t)i], gy = grad[3 * (size_t)i + 1];
    accum[i] = accum[i] + sqrtf(gx * gx + gy * gy);
    denom[i] = denom[i] + 1.f;
    if (max_radii) max_radii[i] = fmaxf(max_radii[i], (float)r);
}

// ---- (c) densify and prune ----------------------------------------------------------------------------------------------------
enum : int { DN_CLONE = 1, DN_SPLIT = 2, DN_KEEP_ORIG = 4, DN_KEEP_CLONE = 8, DN_KEEP_CHILD = 16 };
enum : int { DC_CLONES = 0, DC_SPLITS, DC_KEEP_ORIG, DC_KEEP_CLONE, DC_KEEP_CHILD, DC_N };
enum : int { DK_COPY = 0, DK_MOMENT = 1, DK_XYZ = 2, DK_SCALING = 3, DK_ROTATION = 4 };
constexpr int DN_MAX_TENSORS = RC_MAX_TENSORS;

struct DensifyThresholds {      // each rounded to binary32 once, as a comparison of a float32 tensor with a Python number is
    float max_grad;
    float dense;                // percent_dense * extent
    float min_opacity;
    float world;                // 0.1 * extent
    int use_screen;             // max_screen_size given (and not 0)
};

__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
// log(exp(s) / (0.8 N)), N = 2, with the division as a multiplication by the binary32 reciprocal: that is how the device evaluates
// `tensor / 1.6`; a true division can differ in the last bit
__device__ __forceinline__ float child_log_scale(float s) { return logf(expf(s) * (1.f / 1.6f)); }

// One thread per row: the row's class and what survives the final prune (scene/gaussian_model.py:566-578, N = 2), and the
// workgroup's count of each.  The reference zeroes max_radii2D in densification_postfix before it evaluates
// `max_radii2D > max_screen_size`, so that term is false for every row and is not evaluated here; what max_screen_size decides is
// only whether the world-space test `max exp(s) > 0.1 extent` applies.  A child is tested with its NEW scale.
__global__ void __launch_bounds__(TS_THREADS) densify_plan_kernel(int P, const float* __restrict__ accum, const float* __restrict__ denom,
                                                                  const float* __restrict__ scaling, const float* __restrict__ opacity,
                                                                  DensifyThresholds th, unsigned char* flags, int* block_counts)
{
    __shared__ int lds[TS_WAVES];
    const int i = blockIdx.x * TS_THREADS + threadIdx.x;
    int f = 0;
    if (i < P) {
        float g = accum[i] / denom[i];
        if (g != g) g = 0.f;
        const float s0 = scaling[3 * (size_t)i], s1 = scaling[3 * (size_t)i + 1], s2 = scaling[3 * (size_t)i + 2];
        const float smax = max3(expf(s0), expf(s1), expf(s2));
        const bool sel = g >= th.max_grad, big = smax > th.dense;
        const bool low = 1.f / (1.f + expf(-opacity[i])) < th.min_opacity;
        const bool gone = low || (th.use_screen && smax > th.world);
        if (sel && !big) f |= DN_CLONE | (gone ? 0 : DN_KEEP_CLONE);
        if (sel && big) {
            const float cmax = max3(expf(child_log_scale(s0)), expf(child_log_scale(s1)), expf(child_log_scale(s2)));
            f |= DN_SPLIT | ((low || (th.use_screen && cmax > th.world)) ? 0 : DN_KEEP_CHILD);
        } else if (!gone)
            f |= DN_KEEP_ORIG;
        flags[i] = (unsigned char)f;
    }
    for (int k = 0; k < DC_N; k++) {
        int total;
        block_rank((f >> k) & 1, lds, total);
        if (threadIdx.x == 0) block_counts[blockIdx.x * DC_N + k] = total;
    }
}

// One thread per row: where the row, its clone and its children go.  Output rows: kept originals, kept clones, kept first children,
// kept second children; src_of[output row] = input row.  rank_of[kept child pair] and split_rows[split] tell which normal samples
// belong to a split row (the samples are drawn for every split row, also those whose children the prune deletes).
__global__ void __launch_bounds__(TS_THREADS) densify_map_kernel(int P, const unsigned char* __restrict__ flags, const int* __restrict__ block_offsets,
                                                                 const int* __restrict__ totals, int* src_of, int* rank_of, long long* split_rows)
{
    __shared__ int lds[TS_WAVES];
    const int i = blockIdx.x * TS_THREADS + threadIdx.x;
    const int f = i < P ? flags[i] : 0;
    const int* off = block_offsets + blockIdx.x * DC_N;
    int unused;
    const int r_split = off[DC_SPLITS] + block_rank(f & DN_SPLIT, lds, unused);
    const int r_orig = off[DC_KEEP_ORIG] + block_rank(f & DN_KEEP_ORIG, lds, unused);
    const int r_clone = off[DC_KEEP_CLONE] + block_rank(f & DN_KEEP_CLONE, lds, unused);
    const int r_child = off[DC_KEEP_CHILD] + block_rank(f & DN_KEEP_CHILD, lds, unused);
    const int n_orig = totals[DC_KEEP_ORIG], n_clone = totals[DC_KEEP_CLONE], n_child = totals[DC_KEEP_CHILD];
    if (f & DN_SPLIT) split_rows[r_split] = i;
    if (f & DN_KEEP_ORIG) src_of[r_orig] = i;
    if (f & DN_KEEP_CLONE) src_of[n_orig + r_clone] = i;
    if (f & DN_KEEP_CHILD) {
        src_of[n_orig + n_clone + r_child] = i;
        src_of[n_orig + n_clone + n_child + r_child] = i;
        rank_of[r_child] = r_split;
    }
}

// The gather itself is row_gather_kernel<true> of row_compact.h.  Parameters: every output row is its source row, bit for bit (a
// child's xyz and scaling are overwritten by densify_children_kernel).  Moments (zero_new): kept originals copy theirs, every new
// row is 0.

// One thread per kept pair of children: xyz = R(q / |q|) sample + xyz_parent (utils/general_utils.py:78-99, the bmm's order of
// summation), scaling = log(exp(s) / 1.6).
__global__ void __launch_bounds__(TS_THREADS) densify_children_kernel(int P, int n_split, int n_child, int first_child, const int* __restrict__ src_of,
                                                                      const int* __restrict__ rank_of, const float* __restrict__ xyz,
                                                                      const float* __restrict__ scaling, const float* __restrict__ rotation,
                                                                      const float* __restrict__ samples, float* new_xyz, float* new_scaling)
{
    const int t = blockIdx.x * TS_THREADS + threadIdx.x;
    if (t >= n_child) return;
    int src = src_of[first_child + t], rank = rank_of[t];
    if ((unsigned)src >= (unsigned)P) src = 0;
    if ((unsigned)rank >= (unsigned)n_split) rank = 0;
    const float* q = rotation + 4 * (size_t)src;
    const float norm = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float r = q[0] / norm, x = q[1] / norm, y = q[2] / norm, z = q[3] / norm;
    const float R[9] = {1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y),
                        2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x),
                        2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)};
    float ls[3], c[3];
    for (int k = 0; k < 3; k++) {
        ls[k] = child_log_scale(scaling[3 * (size_t)src + k]);
        c[k] = xyz[3 * (size_t)src + k];
    }
    for (int h = 0; h < 2; h++) {
        const float* sm = samples + 3 * ((size_t)h * n_split + rank);
        const size_t o = 3 * ((size_t)first_child + (size_t)h * n_child + t);
        for (int k = 0; k < 3; k++) {
            new_xyz[o + k] = ((R[3 * k] * sm[0] + R[3 * k + 1] * sm[1]) + R[3 * k + 2] * sm[2]) + c[k];
            new_scaling[o + k] = ls[k];
        }
    }
}

}  // namespace mirast
