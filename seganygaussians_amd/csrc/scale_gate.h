// scale_gate.h -- scale conditioning (train_contrastive_feature.py:42-62, 228, 240-245): the quantile table
// of scikit-learn's QuantileTransformer, its uniform transform, and the scale gates with the backward for their parameters.
//
// Fit and transform restate numpy's percentile and interp OPERATION BY OPERATION in binary64 (one float32 subtraction, as numpy's
// _lerp makes it on a float32 array): the results are those of the library bit for bit.  That holds because the build passes
// -ffp-contract=off (build.py, HIPCC_FLAGS): every product and every sum below rounds on its own, as numpy's loops do; a fused
// multiply-add anywhere in them would change last bits.  Plain loads and stores, no atomics; every result is a function of the
// inputs alone.
#pragma once

#include "wave.h"

namespace mirast {

constexpr int SG_MAX_QUANTILES = 1024;   // one workgroup fits the table; 16 KB of LDS hold it with its references
constexpr int SG_MAX_CHANNELS = 256;
constexpr int SG_THREADS = 256;          // forward: scales per workgroup; backward: threads per channel
constexpr int SG_WAVES = SG_THREADS / 64;
constexpr int SG_DIRECT_MAX = 64;        // up to this many scales the two searches read the table where it lies (L2)
enum : int { SG_MODE_NONE = 0, SG_MODE_LEARNED = 1, SG_MODE_FIXED = 2 };

// np.maximum: a NaN on either side is the result
__device__ __forceinline__ double sg_max_nan(double a, double b) { return (a != a || a >= b) ? a : b; }

// One workgroup of SG_MAX_QUANTILES threads, thread i makes quantile i of np.nanpercentile(s, references * 100) with the default
// (linear) method, then np.maximum.accumulate over i.  s [n]: float32 ascending with the NaNs last (torch.sort); the count m of the
// values in front of them is found here by bisection.  m == 0: every quantile is NaN.
__global__ void __launch_bounds__(SG_MAX_QUANTILES) scale_quantile_fit_kernel(int n, const float* __restrict__ s, int nq,
                                                                              const double* __restrict__ references, double* __restrict__ quantiles)
{
    __shared__ double wave_max[SG_MAX_QUANTILES / 64];
    const int i = threadIdx.x, lane = i & 63, wave = i >> 6;
    int first = 0, last = n;      // the first NaN is in [first, last]
    while (first < last) {
        const int mid = first + (last - first) / 2;
        const float t = s[mid];
        if (t != t) last = mid;
        else first = mid + 1;
    }
    const int m = first;
    double value = __builtin_nan("");
    if (i < nq && m > 0) {
        const double q = (references[i] * 100.0) / 100.0;
        const double v = (double)(m - 1) * q;
        const double fl = floor(v);
        const double g = v - fl;
        int lo = (int)fl;
        lo = lo < 0 ? 0 : lo > m - 1 ? m - 1 : lo;      // q is in [0, 1]: never taken, and no read leaves s whatever the table holds
        const int hi = lo + 1 < m - 1 ? lo + 1 : m - 1;
        const float a = s[lo], b = s[hi];
        const float d = b - a;
        const double a64 = a, b64 = b, d64 = d;
        value = d == 0.f ? a64 : g >= 0.5 ? b64 - d64 * (1.0 - g) : a64 + d64 * g;
    }
    // inclusive running maximum: inside the wave, then over the waves in front (the maximum is exact, so the order is free)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double t = __shfl_up(value, o, 64);
        if (lane >= o) value = sg_max_nan(t, value);
    }
    if (lane == 63) wave_max[wave] = value;
    __syncthreads();
    for (int w = 0; w < wave; w++) value = sg_max_nan(wave_max[w], value);
    if (i < nq) quantiles[i] = value;
}

// numpy's interp(x, Q, R) minus interp(-x, -Q[::-1], -R[::-1]), halved: QuantileTransformer._transform_col with the uniform output,
// for one float32 value.  Both searches run on the table as it lies: the second interp's "largest k with -Q[nq-1-k] <= -x" is the
// smallest i with Q[i] >= x, and its operands are the negated ones of the unreversed table, which changes no rounding.
__device__ __forceinline__ float scale_quantile_transform(float xf, int nq, const double* Q, const double* R)
{
    if (xf != xf) return xf;
    const double x = xf;
    const double q_first = Q[0], q_last = Q[nq - 1];
    int lo = 0, hi = nq;      // j + 1: the first index with Q > x
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (Q[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    const int j = lo - 1;
    lo = 0, hi = nq;          // i: the first index with Q >= x
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (Q[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    const int i = lo;
    double A, B;
    if (x > q_last) A = R[nq - 1];
    else if (x < q_first) A = R[0];
    else {
        const int jj = j < 0 ? 0 : j;      // a table of NaNs leaves j == -1; no read leaves the table
        const double qj = Q[jj], rj = R[jj];
        if (jj >= nq - 1 || qj == x) A = rj;
        else {
            const double slope = (R[jj + 1] - rj) / (Q[jj + 1] - qj);
            A = slope * (x - qj) + rj;
        }
    }
    if (x < q_first) B = -R[0];
    else if (x > q_last) B = -R[nq - 1];
    else {
        const int ii = i > nq - 1 ? nq - 1 : i;
        const double qi = Q[ii], ri = R[ii];
        if (ii <= 0 || qi == x) B = -ri;
        else {
            const double slope = (ri - R[ii - 1]) / (qi - Q[ii - 1]);
            B = slope * (qi - x) + -ri;
        }
    }
    float y = (float)(0.5 * (A - B));
    if (x == q_last) y = 1.f;
    if (x == q_first) y = 0.f;
    return y;
}

// Workgroup b takes the scales [b * SG_THREADS, ...): one thread per scale makes u, then the threads write the workgroup's
// rows * C gates in memory order.  STAGED: the table is copied to LDS first; otherwise (a launch of a few scales) it is read
// where it lies.  mode NONE writes u alone; LEARNED sigmoid(fl(fl(w_c u) + b_c)) with the accurate expf; FIXED
// c < C - dim + trunc(fl(fl(1 - u) dim)) as 1 / 0, and a NaN row for a NaN scale.  u NULL: not written.
template <bool STAGED>
__global__ void __launch_bounds__(SG_THREADS) scale_gate_forward_kernel(int n, const float* __restrict__ scales, int nq, const double* __restrict__ quantiles,
                                                                        const double* __restrict__ references, int mode, int C,
                                                                        const float* __restrict__ weight, const float* __restrict__ bias, int dim,
                                                                        float* __restrict__ u_out, float* __restrict__ gates)
{
    __shared__ double sQ[STAGED ? SG_MAX_QUANTILES : 1], sR[STAGED ? SG_MAX_QUANTILES : 1];
    __shared__ float su[SG_THREADS], sw[SG_MAX_CHANNELS], sb[SG_MAX_CHANNELS];
    const int t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * SG_THREADS;
    const int rows = (size_t)n - base < (size_t)SG_THREADS ? (int)((size_t)n - base) : SG_THREADS;
    if (STAGED) {
        for (int k = t; k < nq; k += SG_THREADS) {
            sQ[k] = quantiles[k];
            sR[k] = references[k];
        }
    }
    if (mode == SG_MODE_LEARNED)
        for (int c = t; c < C; c += SG_THREADS) {
            sw[c] = weight[c];
            sb[c] = bias[c];
        }
    __syncthreads();
    if (t < rows) {
        const float u = STAGED ? scale_quantile_transform(scales[base + t], nq, sQ, sR) : scale_quantile_transform(scales[base + t], nq, quantiles, references);
        su[t] = u;
        if (u_out) u_out[base + t] = u;
    }
    if (mode == SG_MODE_NONE) return;
    __syncthreads();
    float* out = gates + base * (size_t)C;
    const int total = rows * C;      // at most 256 * 256
    for (int k = t; k < total; k += SG_THREADS) {
        const int r = k / C, c = k - r * C;
        const float u = su[r];
        float gate;
        if (mode == SG_MODE_LEARNED) {
            const float z = sw[c] * u + sb[c];
            gate = 1.f / (1.f + expf(-z));
        } else if (u != u) gate = u;
        else gate = c < C - dim + (int)((1.f - u) * (float)dim) ? 1.f : 0.f;
        out[k] = gate;
    }
}

// Workgroup c sums channel c over the n scales: d_bias[c] = sum_n g[n][c] s'(z), d_weight[c] = sum_n g[n][c] s'(z) u[n], with
// z = w_c u[n] + b_c and s' = sigmoid' evaluated in binary64 from the float32 operands.  Thread t adds the rows t, t + 256, ... in
// that order, the wave sums by a fixed butterfly, thread 0 adds the four waves in order: the same bits every run.
__global__ void __launch_bounds__(SG_THREADS) scale_gate_backward_kernel(int n, int C, const float* __restrict__ u, const float* __restrict__ weight,
                                                                         const float* __restrict__ bias, const float* __restrict__ d_gates,
                                                                         float* __restrict__ d_weight, float* __restrict__ d_bias)
{
    __shared__ double part_w[SG_WAVES], part_b[SG_WAVES];
    const int c = blockIdx.x, t = threadIdx.x;
    const double w = weight[c], b = bias[c];
    double acc_w = 0.0, acc_b = 0.0;
    for (int r = t; r < n; r += SG_THREADS) {
        const double ur = u[r];
        const double z = w * ur + b;
        const double e = exp(-fabs(z));      // sigmoid'(z) = e / (1 + e)^2, even in z, without cancellation
        const double term = (double)d_gates[(size_t)r * C + c] * (e / ((1.0 + e) * (1.0 + e)));
        acc_b += term;
        acc_w += term * ur;
    }
    acc_w = wave_sum(acc_w);
    acc_b = wave_sum(acc_b);
    if ((t & 63) == 0) {
        part_w[t >> 6] = acc_w;
        part_b[t >> 6] = acc_b;
    }
    __syncthreads();
    if (t == 0) {
        double sum_w = part_w[0], sum_b = part_b[0];
        for (int k = 1; k < SG_WAVES; k++) {
            sum_w += part_w[k];
            sum_b += part_b[k];
        }
        d_weight[c] = (float)sum_w;
        d_bias[c] = (float)sum_b;
    }
}

}  // namespace mirast
