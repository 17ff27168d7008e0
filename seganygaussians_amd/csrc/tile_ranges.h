// tile_ranges.h -- the range scan: one workgroup turns the per-tile entry totals of either count pass (bin_full.h, bin_lean.h) into
// ranges[tile] and leaves, in the words behind the image buffer's num_rendered field (NR_*), what the later stages and the host need:
// R, the longest list, the number of depth-key bits that differ (for tile_sort.h) and the blend kernels' XCD run boundaries
// (xcd_runs.h).
#pragma once

#include "common.h"
#include "wave.h"
#include "xcd_runs.h"

namespace mirast {

// Writes ranges[tile] = [base, base+count) (== identifyTileRanges' result, rasterizer_impl.cu:116-138, including
// {0,0} for empty tiles as left by the reference's cudaMemset), R and the longest list.
constexpr int BIN_MAX_TILES_TOTAL = 40 * 1024 - 128;  // tile_ranges_kernel scans all tile totals in one workgroup's LDS

// Words behind the R partial sums of the image buffer's num_rendered field (mi_rast.hip: ImgPtrs)
constexpr int NR_TOTAL = 0, NR_LONGEST = 1, NR_VERIFY = 2, NR_KEY_BITS = 3, NR_RUN_BOUNDS = 4;

__global__ void __launch_bounds__(1024) tile_ranges_kernel(int ntiles_all, const uint32_t* __restrict__ tile_total,
                                                           uint2* __restrict__ ranges, int* __restrict__ num_rendered,
                                                           const int* __restrict__ r_slots, int* __restrict__ host_out = nullptr,
                                                           uint32_t* __restrict__ zero_a = nullptr, uint32_t* __restrict__ zero_b = nullptr,
                                                           uint32_t* __restrict__ run_bounds = nullptr /* [9]: the blend kernels' XCD runs
                                                               (xcd_runs.h): equal tile counts, or equal MODELLED work when run_cap > 0 */,
                                                           uint32_t run_cap = 0, uint32_t run_fix = 0)
{
    // The totals are staged in LDS (coalesced), thread t scans the contiguous items [t*per, (t+1)*per) in place,
    // one workgroup scan joins the pieces, and the ranges leave coalesced again.
    // More than BIN_MAX_TILES_TOTAL items (images beyond 10 Mpx) are walked in segments of that many, one after the other, the
    // running total carried along: ONE pass of the loop below for every image up to 4096 x 2544.
    // run_cap > 0 (images of one segment): the XCD runs of the blend kernels are cut at equal sums of the
    // MODELLED cost of a tile, min(list length, run_cap) + run_fix -- a list is walked until its pixels are opaque, which takes about
    // run_cap entries where the scene is dense, and to its end where it is sparse; what a walk really covers is only known behind the
    // forward blend -- the second prefix sum rides on the first, at the granularity of the threads'
    // pieces (registers only); the thread whose piece holds a boundary walks its few tiles.
    // Also left for the per-tile sort: the number of low key bits in which the view's depth keys differ at all (NR_KEY_BITS) --
    // min and max key share every bit above, and so does every key between them.
    extern __shared__ uint32_t s_val[];  // [min(ntiles_all, BIN_MAX_TILES_TOTAL) + 1]
    __shared__ uint32_t s_wave[16];
    __shared__ uint32_t s_wave_w[16];
    __shared__ uint32_t s_bound[9];
    const bool weighted = run_bounds != nullptr && run_cap > 0u && ntiles_all <= BIN_MAX_TILES_TOTAL;   // (one segment)
    __shared__ uint32_t s_maxcount;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 9) s_bound[tid] = xcd_run_start((uint32_t)tid, (uint32_t)ntiles_all);   // equal tile counts unless the model says otherwise
    if (tid == 0) s_maxcount = 0;
    if (wave == 15 && r_slots != nullptr) {   // (a wave that has the least to do below)
        uint32_t inv_min = (uint32_t)r_slots[(lane % R_SLOTS) * R_SLOT_STRIDE + 1];
        uint32_t mx = (uint32_t)r_slots[(lane % R_SLOTS) * R_SLOT_STRIDE + 2];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            inv_min = max(inv_min, (uint32_t)__shfl_xor((int)inv_min, o, 64));
            mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
        }
        const uint32_t kmin = ~inv_min;   // no visible Gaussian: kmin = 0xFFFFFFFF > mx = 0
        const uint32_t diff = mx >= kmin ? (mx ^ kmin) : 0u;
        if (lane == 0) num_rendered[NR_KEY_BITS] = diff ? 32 - __builtin_clz(diff) : 0;
    }
    uint32_t carry = 0;   // entries in front of the segment (the same in every thread)
    for (int seg0 = 0; seg0 < ntiles_all; seg0 += BIN_MAX_TILES_TOTAL) {
        const int ntiles = min(BIN_MAX_TILES_TOTAL, ntiles_all - seg0);
        for (int i = tid; i < ntiles; i += 1024) s_val[i] = tile_total[seg0 + i];
        __syncthreads();
        const int per = (ntiles + 1023) / 1024;
        const int i0 = min(ntiles, tid * per), i1 = min(ntiles, i0 + per);
        uint32_t sum = 0, mx = 0, wsum = 0;
        for (int i = i0; i < i1; i++) {
            const uint32_t c = s_val[i];
            s_val[i] = sum;  // exclusive prefix inside the piece
            sum += c;
            mx = max(mx, c);
            wsum += min(c, run_cap) + run_fix;
        }
        const uint32_t incl = wave_inclusive_scan(sum, lane);
        const uint32_t incl_w = weighted ? wave_inclusive_scan(wsum, lane) : 0u;
        if (lane == 63) {
            s_wave[wave] = incl;
            s_wave_w[wave] = incl_w;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
        __syncthreads();
        if (lane == 0 && mx) atomicMax(&s_maxcount, mx);
        uint32_t woff = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) {
            const uint32_t c = s_wave[w];
            woff += w < wave ? c : 0u;
            total += c;
        }
        const uint32_t piece_base = carry + woff + incl - sum;
        for (int i = i0; i < i1; i++) s_val[i] += piece_base;
        if (tid == 0) s_val[ntiles] = carry + total;
        uint32_t woff_w = 0, total_w = 0;
        if (weighted) {
#pragma unroll
            for (int w = 0; w < 16; w++) {
                const uint32_t c = s_wave_w[w];
                woff_w += w < wave ? c : 0u;
                total_w += c;
            }
        }
        __syncthreads();
        if (weighted && total_w > 0u) {
            // boundary k = first tile i with 8 W(i) >= k W_total, W(i) = modelled work in front of tile i: it lies in (i0, i1] of exactly
            // one piece -- the one with 8 W(i0) < k W_total <= 8 W(i1) -- whose thread walks its tiles (list lengths = differences of
            // the finished prefix)
            const uint64_t w_lo = 8ull * (uint64_t)(woff_w + incl_w - wsum), w_hi = 8ull * (uint64_t)(woff_w + incl_w);
#pragma unroll
            for (uint32_t k = 1; k < 8u; k++) {
                const uint64_t want = (uint64_t)k * (uint64_t)total_w;
                if (w_lo < want && want <= w_hi) {
                    uint64_t wacc = w_lo;
                    int i = i0;
                    for (; i < i1; i++) {
                        wacc += 8ull * (uint64_t)(min(s_val[i + 1] - s_val[i], run_cap) + run_fix);
                        if (wacc >= want) break;
                    }
                    s_bound[k] = (uint32_t)min(i + 1, i1);
                }
            }
        }
        for (int i = tid; i < ntiles; i += 1024) {
            const uint32_t lo = s_val[i], hi = s_val[i + 1];
            ranges[seg0 + i] = hi > lo ? make_uint2(lo, hi) : make_uint2(0u, 0u);
            if (zero_a != nullptr) {   // per-tile words a later kernel accumulates into with atomicMax (blend_fwd_wave.h)
                zero_a[seg0 + i] = 0u;
                zero_b[seg0 + i] = 0u;
            }
        }
        carry += total;
        __syncthreads();   // s_val / s_wave are rewritten by the next segment
    }
    if (run_bounds != nullptr) {
        const uint32_t n = (uint32_t)ntiles_all;   // (s_bound: behind the barrier that ends the segment loop)
        if (tid == 0) {   // the clamp in registers (xcd_clamp_runs on LDS words would be seven dependent round trips)
            uint32_t bb[9];
#pragma unroll
            for (int k = 1; k < 8; k++) bb[k] = s_bound[k];
            const uint32_t maxrun = xcd_max_run(n);
            bb[0] = 0u;
            bb[8] = n;
#pragma unroll
            for (uint32_t k = 1; k < 8u; k++) {
                const uint32_t prev = bb[k - 1], need = (8u - k) * maxrun;
                bb[k] = min(max(bb[k], max(prev, n > need ? n - need : 0u)), min(n, prev + maxrun));
            }
#pragma unroll
            for (int k = 0; k < 9; k++) {
                run_bounds[k] = bb[k];
                if (host_out != nullptr) host_out[NR_RUN_BOUNDS + k] = (int)bb[k];   // the forward's grid is sized for its longest run
            }
        }
    }
    if (tid == 0) {
        num_rendered[NR_TOTAL] = (int)carry;         // R (the host already has it from the preprocess pass; kept for checks)
        num_rendered[NR_LONGEST] = (int)s_maxcount;  // longest list
        if (host_out != nullptr) {                   // the same two words straight into the host's pinned buffer (no copy command)
            host_out[NR_TOTAL] = (int)carry;
            host_out[NR_LONGEST] = (int)s_maxcount;
        }
    }
}

}  // namespace mirast
