// model_edit.h -- the cut of a Gaussian model by a selection (scene/gaussian_model.py:376-428, scene/gaussian_model_ff.py:257-285;
// DESIGN.md section 26): which original rows are current, which of those the mask selects, and the row map of the cut.  The rank
// inside a workgroup, the scan of the workgroups' counts and the gather are those of densify_and_prune (row_compact.h).  Plain
// loads and stores only; every result is a function of the inputs alone.
#pragma once

#include "row_compact.h"

namespace mirast {

enum : int { ME_CURRENT = 1, ME_SELECTED = 2 };     // flags of an original row
enum : int { MT_CURRENT = 0, MT_SELECTED = 1, MT_N = 2 };     // the totals the two scans leave on the device

// nothing selected means everything kept; the map kernel and the counts call both go by this
__host__ __device__ __forceinline__ int edit_kept(int current, int selected) { return selected > 0 ? selected : current; }

// One thread per original row: the workgroup's number of current rows.
__global__ void __launch_bounds__(RC_THREADS) edit_current_kernel(int P0, const float* __restrict__ level, float current_level, int* block_counts)
{
    __shared__ int lds[RC_WAVES];
    const int i = blockIdx.x * RC_THREADS + threadIdx.x;
    int total;
    block_rank(i < P0 && level[i] == current_level, lds, total);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

// One thread per original row: a current row's rank r among the current rows finds its mask byte; flags and the workgroup's number
// of selected rows.  A current row past the caller's n_rows (a model that is not in the state `level` describes) is not selected
// and its mask byte is not read.
__global__ void __launch_bounds__(RC_THREADS) edit_select_kernel(int P0, const float* __restrict__ level, float current_level, int n_rows,
                                                                 const unsigned char* __restrict__ mask, const int* __restrict__ current_offsets,
                                                                 unsigned char* flags, int* block_counts)
{
    __shared__ int lds[RC_WAVES];
    const int i = blockIdx.x * RC_THREADS + threadIdx.x;
    const bool current = i < P0 && level[i] == current_level;
    int total;
    const int r = current_offsets[blockIdx.x] + block_rank(current, lds, total);
    const bool selected = current && (unsigned)r < (unsigned)n_rows && mask[r] != 0;
    if (i < P0) flags[i] = (unsigned char)((current ? ME_CURRENT : 0) | (selected ? ME_SELECTED : 0));
    block_rank(selected, lds, total);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

// One thread per original row: src_of[output row] = the row's rank among the current rows, ascending, and level + 1 for every kept
// row.  Kept = selected, or current when the plan selected nothing.  An output row past n_out is not written.
__global__ void __launch_bounds__(RC_THREADS) edit_map_kernel(int P0, const unsigned char* __restrict__ flags, const int* __restrict__ current_offsets,
                                                              const int* __restrict__ selected_offsets, const int* __restrict__ totals, int n_out,
                                                              float* level, int* src_of)
{
    __shared__ int lds[RC_WAVES];
    const int i = blockIdx.x * RC_THREADS + threadIdx.x;
    const int f = i < P0 ? flags[i] : 0;
    const bool all = totals[MT_SELECTED] == 0;
    const bool current = f & ME_CURRENT, kept = all ? current : (f & ME_SELECTED) != 0;
    int unused;
    const int r = current_offsets[blockIdx.x] + block_rank(current, lds, unused);
    const int out = all ? r : selected_offsets[blockIdx.x] + block_rank(kept, lds, unused);
    if (kept) {
        if ((unsigned)out < (unsigned)n_out) src_of[out] = r;
        if (level) level[i] = level[i] + 1.f;
    }
}

}  // namespace mirast
