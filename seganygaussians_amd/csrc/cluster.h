// cluster.h -- HDBSCAN* on the device: core distances and the Boruvka rounds of the minimum spanning tree of
// the mutual-reachability graph.  Both passes run ONE all-pairs tile loop (cl_all_pairs): a workgroup of 4 waves owns 64 rows, lane
// l of every wave holds row l of the block in registers (a chunk of CH words at a time), wave w takes columns [w J, (w + 1) J) of
// every tile of 4 J columns, and the tile goes through LDS, where all lanes of a wave read the same address (a broadcast).  The n x n
// matrix is never formed.  Included by mi_cluster.hip only.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace mirast {

constexpr int CL_THREADS = 256;
constexpr int CL_WAVES = 4;
constexpr int CL_ROWS = 64;          // rows per workgroup: one per lane, shared by the 4 waves
constexpr int CL_PAIR_WORDS = 512;   // CH * J: words of one wave's slice of a tile
constexpr int CL_MAX_K = 64;
constexpr unsigned CL_NO_WEIGHT = 0xFFFFFFFFu;
constexpr unsigned long long CL_NO_PAIR = ~0ull;

struct ClArgs {
    const uint32_t* rows;   // [n][width]: f32 bits (euclidean) or packed bit sets (jaccard)
    int n, width;
    const int* cnt;         // [n] popcount of every row (jaccard)
    int core_k;
    float* core_out;        // core pass: [n]
    const float* core;      // Boruvka round: [n]
    const int* comp;        // Boruvka round: [n] component of every row
    unsigned* row_w;        // Boruvka round: [n] bits of the least outgoing weight of the row (weights are >= 0: ordered as unsigned)
    int* row_j;             // Boruvka round: [n] the column of that edge, -1 without one
    unsigned* comp_w;       // Boruvka round: [n] atomicMin of row_w over the rows of a component, at the component's own index
};

// ---- the two pair functors --------------------------------------------------------------------------------------------------------
// euclidean: the squared distance, sum_c (x_c - y_c)^2 in channel order with one rounding per channel (fma).  (x - y)^2 and (y - x)^2
// are the same bits, so d(i, j) == d(j, i) bit for bit, and d(i, i) = 0.  The square root is taken once per pair, correctly rounded.
struct ClEuclid {
    typedef float acc_t;
    static constexpr bool jaccard = false;
    static __device__ __forceinline__ float zero() { return 0.f; }
    static __device__ __forceinline__ float step(float acc, uint32_t x, uint32_t y)
    {
        const float d = __uint_as_float(x) - __uint_as_float(y);
        return __builtin_fmaf(d, d, acc);
    }
};

// jaccard: the size of the intersection as an integer
struct ClJaccard {
    typedef int acc_t;
    static constexpr bool jaccard = true;
    static __device__ __forceinline__ int zero() { return 0; }
    static __device__ __forceinline__ int step(int acc, uint32_t x, uint32_t y) { return acc + __popc(x & y); }
};

// float32(1 - I / (|a| + |b| - I + 1e-6)), the quotient and the difference in binary64 and one rounding to binary32
__device__ __forceinline__ float cl_jaccard_dist(int inter, int ca, int cb)
{
    const double den = (double)(ca + cb - inter) + 1e-6;
    return (float)(1.0 - (double)inter / den);
}

// ---- the all-pairs tile loop ------------------------------------------------------------------------------------------------------
// Calls sink(col, acc) once for every column col < n, in ascending order of col within a lane, with the functor's accumulator over the
// whole width for (row of this lane, col).  Rows past n are computed on a copy of row n - 1; the caller drops them.
// smem: at least 4 * CL_PAIR_WORDS words.
template <class M, int CH, class Sink>
__device__ __forceinline__ void cl_all_pairs(const ClArgs& a, uint32_t* smem, int row, int wave, Sink&& sink)
{
    constexpr int J = CL_PAIR_WORDS / CH;          // columns per wave and tile
    constexpr int TC = CL_WAVES * J;               // columns per tile
    constexpr int PER = TC * CH / CL_THREADS;      // words a thread stages per tile and chunk
    const int n = a.n, width = a.width;
    const int nchunk = (width + CH - 1) / CH;
    const int nstage = ((n + TC - 1) / TC) * nchunk;
    const size_t row_off = (size_t)(row < n ? row : n - 1) * (size_t)width;

    uint32_t x[CH];
    auto load_x = [&](int chunk) {
#pragma unroll
        for (int c = 0; c < CH; c++) {
            const int gc = chunk * CH + c;
            x[c] = gc < width ? a.rows[row_off + gc] : 0u;   // zero padding adds nothing to either accumulator
        }
    };
    uint32_t g[PER];
    auto fetch = [&](int stage) {
        const int tile = stage / nchunk, chunk = stage - tile * nchunk;
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const int e = (int)threadIdx.x + k * CL_THREADS;
            const int col = tile * TC + e / CH, gc = chunk * CH + e % CH;
            g[k] = (col < n && gc < width) ? a.rows[(size_t)col * (size_t)width + gc] : 0u;
        }
    };
    if (nchunk == 1) load_x(0);
    fetch(0);
    typename M::acc_t acc[J];
#pragma unroll
    for (int j = 0; j < J; j++) acc[j] = M::zero();
    int tile = 0, chunk = 0;
    for (int stage = 0; stage < nstage; stage++) {
        __syncthreads();   // the previous stage has been read
#pragma unroll
        for (int k = 0; k < PER; k++) smem[threadIdx.x + k * CL_THREADS] = g[k];
        __syncthreads();
        if (stage + 1 < nstage) fetch(stage + 1);   // in flight while this stage is computed
        if (nchunk > 1) load_x(chunk);
        const uint32_t* t = smem + wave * (J * CH);
#pragma unroll
        for (int j = 0; j < J; j++) {
#pragma unroll
            for (int c = 0; c < CH; c++) acc[j] = M::step(acc[j], x[c], t[j * CH + c]);
        }
        if (++chunk == nchunk) {
#pragma unroll
            for (int j = 0; j < J; j++) {
                const int col = tile * TC + wave * J + j;
                if (col < n) sink(col, acc[j]);
                acc[j] = M::zero();
            }
            chunk = 0;
            tile++;
        }
    }
    __syncthreads();   // smem is free for the caller
}

// ---- core pass ------------------------------------------------------------------------------------------------------------------
// top[] ascending; v < top[K - 1].  new[s] = median(top[s - 1], top[s], v) for a sorted list.
template <int K>
__device__ __forceinline__ void cl_insert(float (&top)[K], float v)
{
#pragma unroll
    for (int s = K - 1; s > 0; s--) top[s] = fmaxf(top[s - 1], fminf(top[s], v));
    top[0] = fminf(top[0], v);
}

// core[i] = the core_k-th smallest of d(i, j) over all j (j = i included), 1 <= core_k <= K.  Every lane keeps the K smallest values
// of its quarter of the columns in registers (squared distances for euclidean: the root is monotone); the 4 lanes of a row merge
// through LDS into wave 0.
template <class M, int CH, int K>
__global__ void __launch_bounds__(CL_THREADS) cl_core_kernel(ClArgs a)
{
    constexpr int SM = 4 * CL_PAIR_WORDS > CL_ROWS * K ? 4 * CL_PAIR_WORDS : CL_ROWS * K;
    __shared__ uint32_t smem[SM];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int row = blockIdx.x * CL_ROWS + lane;
    constexpr bool jac = M::jaccard;
    const int ca = jac ? a.cnt[row < a.n ? row : a.n - 1] : 0;
    float top[K];
#pragma unroll
    for (int s = 0; s < K; s++) top[s] = __builtin_inff();
    cl_all_pairs<M, CH>(a, smem, row, wave, [&](int col, typename M::acc_t acc) {
        float v;
        if constexpr (jac) v = cl_jaccard_dist((int)acc, ca, a.cnt[col]);
        else v = (float)acc;
        if (v < top[K - 1]) cl_insert<K>(top, v);
    });
    float* buf = reinterpret_cast<float*>(smem);   // [K][64]
    for (int w = 1; w < CL_WAVES; w++) {
        if (wave == w) {
#pragma unroll
            for (int s = 0; s < K; s++) buf[s * CL_ROWS + lane] = top[s];
        }
        __syncthreads();
        if (wave == 0) {
            for (int s = 0; s < K; s++) {
                const float v = buf[s * CL_ROWS + lane];
                if (v < top[K - 1]) cl_insert<K>(top, v);
            }
        }
        __syncthreads();
    }
    if (wave == 0 && row < a.n) {
        float r = top[0];
#pragma unroll
        for (int s = 1; s < K; s++) r = (s == a.core_k - 1) ? top[s] : r;
        a.core_out[row] = jac ? r : sqrtf(r);
    }
}

// ---- Boruvka round --------------------------------------------------------------------------------------------------------------
// Per row i: the least edge (w, min(i, j), max(i, j)) to a row j of another component, w = max(core_i, core_j, d(i, j)).  For a fixed i
// that order is (w, j); a lane meets its columns in ascending order, so `w < best` keeps the lowest j among equal weights.  The row's
// weight also goes into its component's atomicMin (integer keys: the result does not depend on the order of arrival).
template <class M, int CH>
__global__ void __launch_bounds__(CL_THREADS) cl_row_min_kernel(ClArgs a)
{
    __shared__ uint32_t smem[4 * CL_PAIR_WORDS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int row = blockIdx.x * CL_ROWS + lane;
    const int rr = row < a.n ? row : a.n - 1;
    constexpr bool jac = M::jaccard;
    const int ca = jac ? a.cnt[rr] : 0;
    const int ci = a.comp[rr];
    const float core_i = a.core[rr];
    float bw = __builtin_inff();
    int bj = -1;
    cl_all_pairs<M, CH>(a, smem, row, wave, [&](int col, typename M::acc_t acc) {
        if (a.comp[col] != ci) {
            float d;
            if constexpr (jac) d = cl_jaccard_dist((int)acc, ca, a.cnt[col]);
            else d = sqrtf((float)acc);
            const float w = fmaxf(fmaxf(core_i, a.core[col]), d);
            if (w < bw) {
                bw = w;
                bj = col;
            }
        }
    });
    float* sw = reinterpret_cast<float*>(smem);          // [4][64]
    int* sj = reinterpret_cast<int*>(smem) + CL_WAVES * CL_ROWS;
    sw[wave * CL_ROWS + lane] = bw;
    sj[wave * CL_ROWS + lane] = bj;
    __syncthreads();
    if (wave == 0 && row < a.n) {
        for (int w = 1; w < CL_WAVES; w++) {   // ascending waves hold ascending columns of a tile, but tiles interleave: compare (w, j)
            const float ow = sw[w * CL_ROWS + lane];
            const int oj = sj[w * CL_ROWS + lane];
            if (oj >= 0 && (bj < 0 || ow < bw || (ow == bw && oj < bj))) {
                bw = ow;
                bj = oj;
            }
        }
        a.row_w[row] = __float_as_uint(bw);
        a.row_j[row] = bj;
        if (bj >= 0) atomicMin(&a.comp_w[ci], __float_as_uint(bw));
    }
}

// ---- the small kernels of a round -----------------------------------------------------------------------------------------------
__global__ void cl_popcount_kernel(const uint32_t* rows, int n, int width, int* cnt)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int c = 0;
    for (int k = 0; k < width; k++) c += __popc(rows[(size_t)i * (size_t)width + k]);
    cnt[i] = c;
}

__global__ void cl_components_init_kernel(int n, int* comp, int* parent)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) comp[i] = parent[i] = i;
}

__global__ void cl_round_init_kernel(int n, unsigned* comp_w, unsigned long long* comp_pair, int* merged)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        comp_w[i] = CL_NO_WEIGHT;
        comp_pair[i] = CL_NO_PAIR;
    }
    if (i == 0) *merged = 0;
}

// among the rows that reached their component's least weight: the least (min(i, j), max(i, j))
__global__ void cl_pair_min_kernel(int n, const int* comp, const unsigned* row_w, const int* row_j, const unsigned* comp_w,
                                   unsigned long long* comp_pair)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int j = row_j[i], c = comp[i];
    if (j < 0 || row_w[i] != comp_w[c]) return;
    const unsigned lo = (unsigned)(i < j ? i : j), hi = (unsigned)(i < j ? j : i);
    atomicMin(&comp_pair[c], ((unsigned long long)lo << 32) | hi);
}

// Every component hangs itself below the component at the other end of its edge and records the edge at its own index; of two
// components that chose the same edge the one with the lower index stays a root.  The order on edges is strict and total, so these
// pairs are the only cycles.  A component's index is a root only until it is merged: every index records at most one edge, ever.
__global__ void cl_hook_kernel(int n, const int* comp, const unsigned* comp_w, const unsigned long long* comp_pair, int* parent,
                               int* tmp_a, int* tmp_b, float* tmp_w, int* merged)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n || comp[c] != c) return;
    const unsigned long long p = comp_pair[c];
    if (p == CL_NO_PAIR) return;
    const int lo = (int)(p >> 32), hi = (int)(p & 0xFFFFFFFFu);
    const int clo = comp[lo], chi = comp[hi];
    const int other = clo == c ? chi : clo;
    if (comp_pair[other] == p && c < other) return;
    parent[c] = other;
    tmp_a[c] = lo;
    tmp_b[c] = hi;
    tmp_w[c] = __uint_as_float(comp_w[c]);
    atomicAdd(merged, 1);
}

// pointer jumping in place: a concurrent update only moves parent[p] further up the same chain
__global__ void cl_jump_kernel(int n, int* parent)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const int p = parent[c];
    const int gp = parent[p];
    if (gp != p) parent[c] = gp;
}

__global__ void cl_relabel_kernel(int n, int* comp, const int* parent)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int r = comp[i];
    for (int p = parent[r], hops = 0; p != r && hops < n; p = parent[r], hops++) r = p;   // one step after enough jumps
    comp[i] = r;
}

// the n - 1 recorded edges in ascending order of the index that recorded them (all but the last root)
__global__ void cl_emit_kernel(int n, const int* comp, const int* tmp_a, const int* tmp_b, const float* tmp_w, int* edge_a, int* edge_b,
                               float* edge_w)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int root = comp[0];
    if (c >= n || c == root) return;
    const int slot = c < root ? c : c - 1;
    edge_a[slot] = tmp_a[c];
    edge_b[slot] = tmp_b[c];
    edge_w[slot] = tmp_w[c];
}

}  // namespace mirast
