// row_compact.h -- stream compaction of table rows, shared by densify_and_prune (train_step.h) and the model
// cut (model_edit.h, section 26): the rank of a row inside its workgroup, the one-workgroup scan of the workgroups' counts, and the
// gather of up to 32 float32 tensors through a row map in one launch.  Plain loads and stores only: no atomics, LDS only for the
// rank and the scan.  Every result is a function of the inputs alone.  The kernels are templates, so that each host file that
// includes this header instantiates its own without a second definition at link time.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>

namespace mirast {

constexpr int RC_THREADS = 256;
constexpr int RC_WAVES = RC_THREADS / 64;
constexpr int RC_MAX_TENSORS = 32;
constexpr int RC_MAX_GATHER_GRID = 2048;

// the number of lanes below this one, and in the waves before this one, whose predicate holds; `lds` has RC_WAVES ints
__device__ __forceinline__ int block_rank(bool pred, int* lds, int& block_total)
{
    const unsigned long long mask = __ballot(pred);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();     // the previous use of lds is over
    if (lane == 0) lds[wave] = __popcll(mask);
    __syncthreads();
    int before = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
    for (int w = 0; w < RC_WAVES; w++) {
        const int c = lds[w];
        if (w < wave) before += c;
        total += c;
    }
    block_total = total;
    return before;
}

// One workgroup: exclusive scan of the per-workgroup counts block_counts[block * NK + class], class by class, and the totals.
template <int NK>
__global__ void __launch_bounds__(RC_THREADS) block_scan_kernel(int nblocks, const int* __restrict__ block_counts, int* block_offsets, int* totals)
{
    __shared__ int part[RC_THREADS];
    const int tid = threadIdx.x;
    const int per = (nblocks + RC_THREADS - 1) / RC_THREADS;
    const int b0 = min(tid * per, nblocks), b1 = min(b0 + per, nblocks);
    for (int k = 0; k < NK; k++) {
        int sum = 0;
        for (int b = b0; b < b1; b++) sum += block_counts[b * NK + k];
        __syncthreads();
        part[tid] = sum;
        __syncthreads();
        for (int d = 1; d < RC_THREADS; d <<= 1) {
            const int add = tid >= d ? part[tid - d] : 0;
            __syncthreads();
            part[tid] += add;
            __syncthreads();
        }
        int run = part[tid] - sum;
        for (int b = b0; b < b1; b++) {
            block_offsets[b * NK + k] = run;
            run += block_counts[b * NK + k];
        }
        if (tid == RC_THREADS - 1) totals[k] = part[tid];
    }
}

struct GatherEntry {
    const float* src;
    float* dst;
    int cols;
    int zero_new;     // read only by the ZERO_NEW instantiation: output rows from n_copied on are 0, not gathered
};

struct GatherTable {
    GatherEntry t[RC_MAX_TENSORS];
};

// blockIdx.y = tensor; grid-stride over its new_rows * cols elements.  Every output row is row src_of[row] of the source, bit for
// bit, as 4-byte words.  A src_of entry outside [0, P) reads row 0: a map that is not the plan's cannot make a read leave the tensor.
template <bool ZERO_NEW>
__global__ void __launch_bounds__(RC_THREADS) row_gather_kernel(const GatherTable T, int P, int new_rows, int n_copied, const int* __restrict__ src_of)
{
    const GatherEntry e = T.t[blockIdx.y];
    const size_t total = (size_t)new_rows * e.cols;
    for (size_t x = (size_t)blockIdx.x * RC_THREADS + threadIdx.x; x < total; x += (size_t)gridDim.x * RC_THREADS) {
        const int j = (int)(x / e.cols), c = (int)(x - (size_t)j * e.cols);
        float val = 0.f;
        if (!ZERO_NEW || !e.zero_new || j < n_copied) {
            int s = src_of[j];
            if ((unsigned)s >= (unsigned)P) s = 0;
            val = e.src[(size_t)s * e.cols + c];
        }
        e.dst[x] = val;
    }
}

inline unsigned gather_grid_x(size_t longest)
{
    const size_t gx = (longest + RC_THREADS - 1) / RC_THREADS;
    return (unsigned)(gx > (size_t)RC_MAX_GATHER_GRID ? RC_MAX_GATHER_GRID : gx);
}

}  // namespace mirast
