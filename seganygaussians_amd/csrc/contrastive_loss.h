// contrastive_loss.h -- SAGA's contrastive loss: SAM-mask targets and the pair loss (include/mi_contrastive.h; DESIGN.md section 14;
// reference: train_contrastive_feature.py:145-226 and :255-299).
//
//   pack    : bool (M, H, W) -> (M, H, Wq) 64-bit words, Wq = ceil(W / 64); bit b of word q = pixel x = 64 q + b (padding bits 0).
//   cover   : one streaming pass over the packed masks: exact integer per-mask areas (64-bit atomics, order-free) and
//             sampled_ray = (any mask covers the pixel) && ray_rand < rate.
//   targets : one wave per sampled ray: the covering masks in sorted order as a bitset (Wd = ceil(M / 64) words, one per lane),
//             the area-weighted mean mask size a (the reference's f32 sum in sorted order), and per sampled scale the gt bitset:
//             every covering mask of sorted index > si plus the highest-index covering mask <= si (all covering masks when the
//             scale is an upper bound or si = -1).  gt_corr[n][h][j] = (g_h[n] & g_j[n]) != 0.
//   classes : one workgroup per row h: the consistent-positive / consistent-negative / inconsistent counts over the full S x S
//             matrix, diagonal included (the reference's sum_0 classes).
//   loss    : forward one workgroup per row h over the pairs j > h (plus j = h for the cosine statistics), per-row partials, and
//             one workgroup that adds the rows up in a fixed order; backward one workgroup per row h over all j != h, writing
//             dL/dfeatures[:, h, :] with no atomics.  Both passes take every per-pair decision through cl_pair_corr and
//             cl_pair_select, so they agree bit for bit.
#pragma once

#include "../../include/mi_contrastive.h"
#include "packed_masks.h"

namespace mirast {

constexpr int CL_THREADS = 256;
constexpr int CL_MAX_WORDS = PM_MAX_MASKS / 64;
constexpr int CL_ROW_STATS = 8;   // per-row partials: pos sum, neg sum, pos pairs, neg pairs, cos+ sum, cos+ count, cos- sum, cos- count

// ---- pack --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CL_THREADS) cl_pack_kernel(int M, int H, int W, int Wq, const uint8_t* __restrict__ masks,
                                                             uint64_t* __restrict__ packed)
{
    const size_t i = (size_t)blockIdx.x * CL_THREADS + threadIdx.x;
    if (i >= (size_t)M * H * Wq) return;
    const int q = (int)(i % Wq);
    const uint8_t* row = masks + (i / Wq) * (size_t)W;   // i / Wq = m H + y
    const int x0 = q * 64, n = min(64, W - x0);
    uint64_t word = 0;
    if (n == 64 && ((uintptr_t)(row + x0) & 7) == 0) {
        // 8 bytes of 0/1 per load; (v * 0x0102040810204080) >> 56 gathers the low bit of byte b into bit b
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint64_t v = *reinterpret_cast<const uint64_t*>(row + x0 + 8 * k) & 0x0101010101010101ull;
            word |= ((v * 0x0102040810204080ull) >> 56) << (8 * k);
        }
    } else {
        for (int b = 0; b < n; b++) word |= (uint64_t)(row[x0 + b] != 0) << b;
    }
    packed[i] = word;
}

// ---- cover -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CL_THREADS) cl_cover_kernel(int M, int H, int W, int Wq, const uint64_t* __restrict__ packed,
                                                              const float* __restrict__ ray_rand, float rate,
                                                              uint8_t* __restrict__ sampled_ray, unsigned long long* __restrict__ area)
{
    const size_t HWq = (size_t)H * Wq;
    const size_t i = (size_t)blockIdx.x * CL_THREADS + threadIdx.x;
    const bool live = i < HWq;
    const int lane = threadIdx.x & 63;
    uint64_t cov = 0;
    for (int m = 0; m < M; m++) {
        const uint64_t wd = live ? packed[(size_t)m * HWq + i] : 0ull;
        cov |= wd;
        int c = __popcll(wd);
#pragma unroll
        for (int off = 32; off; off >>= 1) c += __shfl_xor(c, off);   // (not wave.h's wave_sum: the kernel's code would change)
        if (lane == 0 && c) atomicAdd(&area[m], (unsigned long long)c);
    }
    if (!live) return;
    const int y = (int)(i / Wq), x0 = (int)(i % Wq) * 64, n = min(64, W - x0);
    const size_t p = (size_t)y * W + x0;
    for (int b = 0; b < n; b++) sampled_ray[p + b] = (uint8_t)(((cov >> b) & 1ull) && ray_rand[p + b] < rate);
}

// ---- targets -----------------------------------------------------------------------------------------------------------------
// acc layout (unsigned long long, zeroed by the caller): [0..2] class counts (cons_pos, cons_neg, incons), [3] max bits of a,
// [4] ~(min bits of a) (a > 0, so the float order is the unsigned order of its bits), [5 .. 5+M) per-mask areas (original order).
constexpr int CL_ACC_CLASSES = 0, CL_ACC_AMAX = 3, CL_ACC_NAMIN = 4, CL_ACC_AREA = 5;

__global__ void __launch_bounds__(CL_THREADS) cl_targets_kernel(int M, int H, int Wq, const uint64_t* __restrict__ packed,
                                                                const int64_t* __restrict__ sort_idx, int S,
                                                                const int* __restrict__ ray_yx, int N, const int* __restrict__ scale_si,
                                                                const int* __restrict__ scale_ub, int Wd, uint64_t* __restrict__ gt,
                                                                float* __restrict__ a_out, unsigned long long* __restrict__ acc)
{
    const int s = (int)(((size_t)blockIdx.x * CL_THREADS + threadIdx.x) >> 6);   // one wave per ray: wave-uniform exit
    const int lane = threadIdx.x & 63;
    if (s >= S) return;
    const int y = ray_yx[2 * s], x = ray_yx[2 * s + 1];
    const unsigned long long* area = acc + CL_ACC_AREA;
    // lane w ends up holding word w of the covering set, bit k = sorted mask 64 w + k
    uint64_t bits = 0;
    for (int it = 0; it < Wd; it++) {
        const int k = it * 64 + lane;
        int bit = 0;
        if (k < M) bit = (int)pm_bit(packed + ((size_t)sort_idx[k] * H + y) * Wq, x);
        const uint64_t b = __ballot(bit);
        if (lane == it) bits = b;
    }
    // per_pixel_mask_size.sum(0) / (sam_masks.sum(0) + 1e-9) (:181-183): f32 sum of the covering masks' areas in sorted order
    float sum = 0.f;
    int cnt = 0;
    for (int w = 0; w < Wd; w++) {
        uint64_t b = (uint64_t)__shfl((unsigned long long)bits, w);
        while (b) {
            const int k = w * 64 + __builtin_ctzll(b);
            b &= b - 1;
            sum = sum + (float)area[sort_idx[k]];
            cnt++;
        }
    }
    const float a = sum / ((float)cnt + 1e-9f);
    if (lane == 0) {
        a_out[s] = a;
        const unsigned int ab = __float_as_uint(a);
        atomicMax(&acc[CL_ACC_AMAX], (unsigned long long)ab);
        atomicMax(&acc[CL_ACC_NAMIN], (unsigned long long)(~ab));
    }
    // gt_vec per sampled scale (:207-218)
    const int lo = lane * 64;
    for (int n = 0; n < N; n++) {
        const int si = scale_si[n];
        uint64_t g = bits;
        if (!scale_ub[n] && si >= 0) {
            const int first_above = si + 1;   // sorted indices >= first_above are kept whole
            const uint64_t above = first_above <= lo ? ~0ull : (first_above >= lo + 64 ? 0ull : (~0ull << (first_above - lo)));
            const uint64_t below = bits & ~above;
            const uint64_t owners = __ballot(below != 0);
            g = bits & above;
            if (owners && lane == 63 - __builtin_clzll(owners)) g |= 1ull << (63 - __builtin_clzll(below));
        }
        if (lane < Wd) gt[((size_t)s * N + n) * Wd + lane] = g;
    }
}

__device__ __forceinline__ bool cl_gt(const uint64_t* __restrict__ gh, const uint64_t* __restrict__ gj, int Wd)
{
    uint64_t any = 0;
    for (int w = 0; w < Wd; w++) any |= gh[w] & gj[w];
    return any != 0;
}

template <typename T>
__device__ __forceinline__ void cl_block_sum(T* vals, int nvals, T* sm /* [CL_THREADS * nvals] */)
{
    // fixed-order tree over the workgroup's threads: the same inputs give the same bits (an LDS tree, not wave.h's butterfly: another order)
    for (int k = 0; k < nvals; k++) sm[k * CL_THREADS + threadIdx.x] = vals[k];
    __syncthreads();
    for (int off = CL_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            for (int k = 0; k < nvals; k++) sm[k * CL_THREADS + threadIdx.x] += sm[k * CL_THREADS + threadIdx.x + off];
        __syncthreads();
    }
    for (int k = 0; k < nvals; k++) vals[k] = sm[k * CL_THREADS];
}

__global__ void __launch_bounds__(CL_THREADS) cl_classes_kernel(int S, int N, int Wd, const uint64_t* __restrict__ gt,
                                                                unsigned long long* __restrict__ acc)
{
    __shared__ uint64_t s_gh[32 * CL_MAX_WORDS];
    __shared__ unsigned long long s_red[3 * CL_THREADS];
    const int h = blockIdx.x;
    for (int t = threadIdx.x; t < N * Wd; t += CL_THREADS) s_gh[t] = gt[(size_t)h * N * Wd + t];
    __syncthreads();
    unsigned long long c[3] = {0ull, 0ull, 0ull};
    for (int j = h + (int)threadIdx.x; j < S; j += CL_THREADS) {
        int k = 0;
        for (int n = 0; n < N; n++) k += cl_gt(s_gh + n * Wd, gt + ((size_t)j * N + n) * Wd, Wd);
        const unsigned long long mult = j == h ? 1ull : 2ull;   // (h, j) and (j, h)
        c[k == N ? 0 : (k == 0 ? 1 : 2)] += mult;
    }
    cl_block_sum(c, 3, s_red);
    if (threadIdx.x == 0)
        for (int k = 0; k < 3; k++)
            if (c[k]) atomicAdd(&acc[CL_ACC_CLASSES + k], c[k]);
}

// ---- loss: the per-pair functions both passes share ---------------------------------------------------------------------------
// corr[n][h][j] = <f_h, f_j> over the C channels, in channel order, one fused multiply-add per channel.  The product is
// commutative, so cl_pair_corr(f_h, f_j) and cl_pair_corr(f_j, f_h) give the same bits.
__device__ __forceinline__ float cl_pair_corr(const float* __restrict__ fa, const float* __restrict__ fb, int C)
{
    float acc = 0.f;
    if ((C & 3) == 0) {
        for (int c = 0; c < C; c += 4) {
            const float4 u = *reinterpret_cast<const float4*>(fa + c);
            const float4 v = *reinterpret_cast<const float4*>(fb + c);
            acc = fmaf(u.x, v.x, acc);
            acc = fmaf(u.y, v.y, acc);
            acc = fmaf(u.z, v.z, acc);
            acc = fmaf(u.w, v.w, acc);
        }
    } else {
        for (int c = 0; c < C; c++) acc = fmaf(fa[c], fb[c], acc);
    }
    return acc;
}

struct ClConst {
    float ptp_max, den, t_pos, t_neg;
};

// The reference's f32 scalar chain from the device accumulators: ptp_max = max(a_h a_j) = fl(amax amax) (rounding is monotone);
// min w = 1; max w = max(fl(ptp_max / fl(amin amin)), 1) (:186-190); thresholds f32(f32(incons) / 2) / f32(count) (:262-270).
__device__ __forceinline__ ClConst cl_consts(const unsigned long long* __restrict__ acc)
{
    ClConst k;
    const float amax = __uint_as_float((unsigned int)acc[CL_ACC_AMAX]);
    const float amin = __uint_as_float(~(unsigned int)acc[CL_ACC_NAMIN]);
    k.ptp_max = amax * amax;
    const float wmax = fmaxf(k.ptp_max / (amin * amin), 1.0f);
    k.den = wmax - 1.0f;
    const float sampled_num = (float)acc[CL_ACC_CLASSES + 2] / 2.0f;
    k.t_pos = sampled_num / (float)acc[CL_ACC_CLASSES + 0];
    k.t_neg = sampled_num / (float)acc[CL_ACC_CLASSES + 1];
    return k;
}

// per_pixel_weight[h][j] (:186-190), the reference's f32 operation order
__device__ __forceinline__ float cl_weight(const ClConst& k, float ah, float aj)
{
    const float r = k.ptp_max / (ah * aj);
    const float w = fmaxf(r, 1.0f);
    return (w - 1.0f) / k.den * 9.0f + 1.0f;
}

// The pair's selections (:262-289) from corr[n] (n = 0 .. N-1 at stride `cstride`) and the gt bits; gtmask bit n = gt_corr[n].
// Returns bit 0 = in sampled_mask_positive, bit 1 = in sampled_mask_negative (h != j; the caller passes rand[min][max]).
__device__ __forceinline__ int cl_pair_select(int N, const float* corr, int cstride, uint32_t gtmask, float r, const ClConst& k)
{
    bool pos_hint = false, neg_hint = false;
    for (int n = 0; n < N; n++) {
        const float c = corr[n * cstride];
        const bool g = (gtmask >> n) & 1u;
        pos_hint |= g && c < 0.75f;
        neg_hint |= !g && c > 0.5f;
    }
    const int ng = __popc(gtmask);
    const bool cons_pos = ng == N, cons_neg = ng == 0, incons = !cons_pos && !cons_neg;
    const bool sp = (cons_pos && r < k.t_pos) || pos_hint || incons;
    const bool sn = (cons_neg && r < k.t_neg) || neg_hint || incons;
    return (sp ? 1 : 0) | (sn ? 2 : 0);
}

__device__ __forceinline__ uint32_t cl_gt_mask(int N, int Wd, const uint64_t* gh /* row h, [N][Wd] */, const uint64_t* gj)
{
    uint32_t m = 0;
    for (int n = 0; n < N; n++) m |= (uint32_t)cl_gt(gh + n * Wd, gj + n * Wd, Wd) << n;
    return m;
}

// ---- loss forward: one workgroup per row h --------------------------------------------------------------------------------------
// dynamic LDS: corr [N][CL_THREADS] floats, then the row's gt words [N][Wd], then the reduction area [CL_ROW_STATS][CL_THREADS] doubles
__global__ void __launch_bounds__(CL_THREADS) cl_loss_fwd_kernel(int S, int N, int C, int Wd, const float* __restrict__ feats,
                                                                 const uint64_t* __restrict__ gt, const float* __restrict__ a,
                                                                 const unsigned long long* __restrict__ acc, const float* __restrict__ rand,
                                                                 double* __restrict__ partials)
{
    extern __shared__ __align__(16) unsigned char cl_smem[];
    double* s_red = reinterpret_cast<double*>(cl_smem);
    float* s_corr = reinterpret_cast<float*>(s_red + CL_ROW_STATS * CL_THREADS);
    uint64_t* s_gh = reinterpret_cast<uint64_t*>(s_corr + N * CL_THREADS);
    const int h = blockIdx.x, t = threadIdx.x;
    for (int i = t; i < N * Wd; i += CL_THREADS) s_gh[i] = gt[(size_t)h * N * Wd + i];
    __syncthreads();
    const ClConst k = cl_consts(acc);
    const float ah = a[h];
    const size_t SC = (size_t)S * C;
    double v[CL_ROW_STATS];
#pragma unroll
    for (int q = 0; q < CL_ROW_STATS; q++) v[q] = 0.0;
    float* my = s_corr + t;
    for (int j = h + t; j < S; j += CL_THREADS) {
        const uint32_t gm = cl_gt_mask(N, Wd, s_gh, gt + (size_t)j * N * Wd);
        for (int n = 0; n < N; n++) my[n * CL_THREADS] = cl_pair_corr(feats + n * SC + (size_t)h * C, feats + n * SC + (size_t)j * C, C);
        // cosine_pos / cosine_neg over the full matrix (:297-298): (h, j) and (j, h) off the diagonal
        const double mult = j == h ? 1.0 : 2.0;
        for (int n = 0; n < N; n++) {
            const float c = my[n * CL_THREADS];
            if ((gm >> n) & 1u) { v[4] += mult * (double)c; v[5] += mult; }
            else                { v[6] += mult * (double)c; v[7] += mult; }
        }
        if (j == h) continue;
        const int sel = cl_pair_select(N, my, CL_THREADS, gm, rand[(size_t)h * S + j], k);
        if (!sel) continue;
        const float w = cl_weight(k, ah, a[j]);
        // (-w * gt * corr) and (w * (1 - gt) * relu(corr)) (:293-294), f32 terms, summed in double
        if (sel & 1) {
            v[2] += 1.0;
            for (int n = 0; n < N; n++) {
                const float gtf = (float)((gm >> n) & 1u);
                v[0] += (double)((-w * gtf) * my[n * CL_THREADS]);
            }
        }
        if (sel & 2) {
            v[3] += 1.0;
            for (int n = 0; n < N; n++) {
                const float gtf = (float)((gm >> n) & 1u);
                v[1] += (double)((w * (1.0f - gtf)) * fmaxf(my[n * CL_THREADS], 0.0f));
            }
        }
    }
    cl_block_sum(v, CL_ROW_STATS, s_red);
    if (t == 0)
        for (int q = 0; q < CL_ROW_STATS; q++) partials[(size_t)h * CL_ROW_STATS + q] = v[q];
}

// One workgroup: the rows' partials in a fixed order.  out_f32 = {loss, cosine_pos, cosine_neg}; out_i64 = {n_pos, n_neg}
// (selected pairs h < j of sampled_mask_positive / _negative).
__global__ void __launch_bounds__(CL_THREADS) cl_loss_final_kernel(int S, int N, const double* __restrict__ partials,
                                                                   float* __restrict__ out_f32, long long* __restrict__ out_i64)
{
    __shared__ double s_red[CL_ROW_STATS * CL_THREADS];
    double v[CL_ROW_STATS];
#pragma unroll
    for (int q = 0; q < CL_ROW_STATS; q++) v[q] = 0.0;
    for (int h = threadIdx.x; h < S; h += CL_THREADS)
        for (int q = 0; q < CL_ROW_STATS; q++) v[q] += partials[(size_t)h * CL_ROW_STATS + q];
    cl_block_sum(v, CL_ROW_STATS, s_red);
    if (threadIdx.x == 0) {
        // .mean() of an empty selection is 0 / 0 = NaN, as in the reference
        const float pos = (float)(v[0] / ((double)N * v[2]));
        const float neg = (float)(v[1] / ((double)N * v[3]));
        out_f32[0] = pos + neg;
        out_f32[1] = (float)(v[4] / v[5]);
        out_f32[2] = (float)(v[6] / v[7]);
        out_i64[0] = (long long)v[2];
        out_i64[1] = (long long)v[3];
    }
}

// ---- loss backward: one workgroup per row h, dL/dfeatures[:, h, :] written in full ----------------------------------------------
// dcorr[n][h][j] for h < j: fl(fl(g / numel_pos) * fl(-w * gt)) where positive-selected, plus fl(g / numel_neg) * fl(w * (1 - gt))
// where negative-selected and corr > 0 (mean, mul and relu backward); dF[n][h] = sum_j dcorr[n][min(h,j)][max(h,j)] f[n][j].
// dynamic LDS: dcorr [N][CL_THREADS] floats, then the row's gt words [N][Wd]
__global__ void __launch_bounds__(CL_THREADS) cl_loss_bwd_kernel(int S, int N, int C, int Wd, const float* __restrict__ feats,
                                                                 const uint64_t* __restrict__ gt, const float* __restrict__ a,
                                                                 const unsigned long long* __restrict__ acc, const float* __restrict__ rand,
                                                                 const long long* __restrict__ n_sel, const float* __restrict__ g_loss,
                                                                 float* __restrict__ dfeats)
{
    extern __shared__ __align__(16) unsigned char cl_smem[];
    float* s_d = reinterpret_cast<float*>(cl_smem);
    uint64_t* s_gh = reinterpret_cast<uint64_t*>(s_d + N * CL_THREADS);
    const int h = blockIdx.x, t = threadIdx.x;
    for (int i = t; i < N * Wd; i += CL_THREADS) s_gh[i] = gt[(size_t)h * N * Wd + i];
    const ClConst k = cl_consts(acc);
    const float g = *g_loss;
    const float gp = g / (float)((long long)N * n_sel[0]);
    const float gn = g / (float)((long long)N * n_sel[1]);
    const size_t SC = (size_t)S * C;
    for (int o = t; o < N * C; o += CL_THREADS) dfeats[(o / C) * SC + (size_t)h * C + (o % C)] = 0.f;
    __syncthreads();
    float* my = s_d + t;
    for (int base = 0; base < S; base += CL_THREADS) {
        const int j = base + t;
        if (j < S && j != h) {
            const uint32_t gm = cl_gt_mask(N, Wd, s_gh, gt + (size_t)j * N * Wd);
            for (int n = 0; n < N; n++) my[n * CL_THREADS] = cl_pair_corr(feats + n * SC + (size_t)h * C, feats + n * SC + (size_t)j * C, C);
            const int lo = min(h, j), hi = max(h, j);
            const int sel = cl_pair_select(N, my, CL_THREADS, gm, rand[(size_t)lo * S + hi], k);
            const float w = sel ? cl_weight(k, a[lo], a[hi]) : 0.f;
            for (int n = 0; n < N; n++) {
                const float c = my[n * CL_THREADS];
                const float gtf = (float)((gm >> n) & 1u);
                float d = 0.f;
                if (sel & 1) d = gp * (-w * gtf);
                if ((sel & 2) && c > 0.f) d = (sel & 1) ? d + gn * (w * (1.0f - gtf)) : gn * (w * (1.0f - gtf));
                my[n * CL_THREADS] = d;
            }
        } else {
            for (int n = 0; n < N; n++) my[n * CL_THREADS] = 0.f;
        }
        __syncthreads();
        const int cnt = min(CL_THREADS, S - base);
        for (int o = t; o < N * C; o += CL_THREADS) {
            const int n = o / C, c = o % C;
            const float* fcol = feats + n * SC + (size_t)base * C + c;
            const float* dn = s_d + n * CL_THREADS;
            float sum = 0.f;
            for (int q = 0; q < cnt; q++) sum = fmaf(dn[q], fcol[(size_t)q * C], sum);
            dfeats[n * SC + (size_t)h * C + c] += sum;
        }
        __syncthreads();
    }
}

}  // namespace mirast
