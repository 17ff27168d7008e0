// xcd_runs.h -- how the blend kernels' workgroups map to tiles: one contiguous run of tiles per XCD, its second half a work queue.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mirast {

// Workgroup b of a 1-D grid runs on XCD b % 8 (tools/xcc_probe.hip), and every XCD has its own L2.  Neighbouring tiles share most
// of their Gaussians.  The backward blend therefore gives every XCD a CONTIGUOUS run of tiles (row major:
// an eighth of the image, a band of whole tile rows): the records and feature rows neighbouring tiles share come through one L2,
// and the gradient atomics of a Gaussian hit lines that L2 already holds instead of lines that travel between L2s -- backward
// blend 0.647 -> 0.565 ms on cfg3.
//   static:              workgroup id = 8 j + x is the j-th tile of XCD x's run.  The kernel time is then the busiest XCD's.
//   dynamic (xcd_grab_runs): the backward blend's cost per tile is the scene's density, and a static split would hand one XCD the
//                        empty sky.  There the second half of every run is a QUEUE: a wave takes its item from the queue of
//                        the XCD it runs on (one returning atomic on that XCD's counter; HW_REG_XCC_ID says which) and, when
//                        that is empty, from the next XCD's.  As many such waves as queued items, each takes exactly one:
//                        every item is taken exactly once.  (All of a run queued: 0.597 ms instead of 0.565 -- the counter's
//                        answer is a round trip in front of every wave's work; persistent waves that request the next item
//                        ahead of time: 0.63, spills and an uneven tail.)
__host__ __device__ __forceinline__ uint32_t xcd_run_start(uint32_t x, uint32_t n) { return (uint32_t)(((uint64_t)x * n) >> 3); }
constexpr int XCD_QUEUE_STRIDE = 16;  // uint32 words between the eight queue counters (one 64-byte line each)
constexpr uint32_t XCD_QUEUE_DIV = 2;  // the queued part of a run is its last 1 / XCD_QUEUE_DIV
// WORK-balanced runs (round 5).  Equal tile counts per XCD are equal TIME only on a scene whose density does not vary over the image:
// on the second synthetic law (opaque surfaces + floaters; real scenes are of this kind) the slowest XCD ended 20-23 % behind the
// mean in both blend kernels (profiles/r04_xcd_balance.md), and nothing lets a fast XCD take more -- the dispatcher hands workgroup b
// to XCD b % 8 whatever the XCDs' progress.  The range scan (tile_ranges.h: tile_ranges_kernel) therefore cuts the row-major tile
// sequence into eight contiguous runs of equal MODELLED work, sum(min(list length, 768) + 128) -- the list LENGTH alone is the wrong
// weight: an opaque surface ends a long list early --, and leaves the nine boundaries in the image buffer for both blend kernels
// (profiles/r05_xcd_balance.md: cfg3s +7 %).  (Cutting the backward's runs at equal sums of what the forward really WALKED instead,
// one more launch behind the forward blend, gained nothing in round 6 and was removed: DESIGN.md section 11.)  A run holds at most
// XCD_MAX_RUN_FACTOR times the equal share: that bounds the grid the (stateless) backward launches -- ids beyond a run's length exit
// at once.
constexpr uint32_t XCD_MAX_RUN_FACTOR = 2;
struct XcdRuns {
    uint32_t b[9];   // run x = tiles [b[x], b[x + 1])
};
__host__ __device__ inline uint32_t xcd_max_run(uint32_t n)
{
    const uint32_t m = XCD_MAX_RUN_FACTOR * ((n + 7u) >> 3);
    return m < n ? m : n;
}
__host__ __device__ inline uint32_t xcd_static_len_max(uint32_t n)
{
    const uint32_t longest = xcd_max_run(n);
    return longest - longest / XCD_QUEUE_DIV;
}
__host__ __device__ inline uint32_t xcd_queued_tiles_max(uint32_t n) { return n / XCD_QUEUE_DIV; }   // >= sum over the runs of len / DIV
__device__ __forceinline__ XcdRuns xcd_load_runs(const uint32_t* __restrict__ bounds)
{
    XcdRuns r;
#pragma unroll
    for (int k = 0; k < 9; k++) r.b[k] = bounds[k];   // wave-uniform address: scalar loads
    return r;
}
// Clamps eight proposed boundaries (s_bound[1..7], any values) so that every run holds at most xcd_max_run(n) tiles and the runs
// partition [0, n): one thread.
__device__ __forceinline__ void xcd_clamp_runs(uint32_t* s_bound, uint32_t n)
{
    const uint32_t maxrun = xcd_max_run(n);
    s_bound[0] = 0u;
    s_bound[8] = n;
    for (uint32_t k = 1; k < 8u; k++) {
        const uint32_t prev = s_bound[k - 1];
        const uint32_t need = (8u - k) * maxrun;               // what the runs behind boundary k can hold at most
        const uint32_t lo = max(prev, n > need ? n - need : 0u);
        const uint32_t hi = min(n, prev + maxrun);
        s_bound[k] = min(max(s_bound[k], lo), hi);
    }
}
// xcd_grab over given runs: as above; takers beyond the queued items of all eight runs (the grid is sized for the longest runs the
// clamp allows) find every queue empty after eight probes and get 0xFFFFFFFF.
__device__ __forceinline__ uint32_t xcd_grab_runs(uint32_t* __restrict__ counters, const XcdRuns& runs, uint32_t per)
{
    const uint32_t x0 = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 7u;  // HW_REG_XCC_ID[3:0]
    const bool first = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u;
    for (uint32_t k = 0; k < 8u; k++) {
        const uint32_t x = (x0 + k) & 7u;
        uint32_t start = runs.b[0], end = runs.b[1];
#pragma unroll
        for (uint32_t j = 1; j < 8u; j++) {
            start = x == j ? runs.b[j] : start;
            end = x == j ? runs.b[j + 1] : end;
        }
        const uint32_t len = end - start;
        uint32_t got = 0;
        if (first) got = atomicAdd(&counters[x * XCD_QUEUE_STRIDE], 1u);
        got = __builtin_amdgcn_readfirstlane(got);
        if (got < (len / XCD_QUEUE_DIV) * per) return (start + len - len / XCD_QUEUE_DIV) * per + got;
    }
    return 0xFFFFFFFFu;
}

}  // namespace mirast
