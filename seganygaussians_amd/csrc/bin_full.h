// bin_full.h -- count and emit passes of the FULL lists (the reference's `debug` flag, MI_RAST_FULL_LISTS, MI_RAST_NO_CULL: parity
// tests), never the product path (bin_lean.h).  Contract: the Gaussians are dealt to <= BIN_MAX_WG workgroups in 64-index chunks
// ("slices"); bin_count_kernel leaves partial[slice][tile], scan_partials_kernel turns it into every slice's offset inside every
// tile's segment plus the tile totals (no global atomics), tile_ranges_kernel (tile_ranges.h) makes the ranges, and bin_ranks_kernel
// stores one 8-byte entry {depth bits, id | quadrant mask << 28} per overlap of the reference's rects, in arbitrary order inside a
// tile's segment (LDS cursors start at ranges[tile].x + the slice's offset).  Both passes take the rects from the same records with
// the same code, so the counts cannot disagree with the emission.  Images with more than BIN_MAX_TILES tiles are walked in bands of
// tile rows, one launch per band.
#pragma once

#include "blend_rec.h"
#include "common.h"
#include "cull.h"
#include "wave.h"

namespace mirast {

constexpr int BIN_MAX_WG = 256;        // workgroups of the count / emit passes (slices of the Gaussians): one per CU, all resident at once
constexpr int BIN_THREADS = 1024;
constexpr int BIN_MAX_TILES = 22 * 1024 - 64;  // per launch of the count / emit passes: one LDS counter per tile + 61 KB of hand-off
                                               // arrays must fit in 160 KB; larger images are walked in bands of tile rows

// Row of partial[][] (= position of the slice inside every tile's segment) of workgroup b.  Workgroup b runs on XCD b % 8
// (tools/xcc_probe.hip) and each XCD has its own L2: with the slices of one XCD next to each other, the entries that
// share a 128-byte line of a tile's segment are mostly stored from ONE XCD instead of eight (measured: emit 0.086 -> 0.074 ms;
// the HBM write bytes of the pass did not change).  Any bijection is correct -- count, scan and emit only have to agree on it.
__device__ __forceinline__ uint32_t slice_row(uint32_t b, uint32_t nwg)
{
    return (nwg & 7u) ? b : (b & 7u) * (nwg >> 3) + (b >> 3);
}

// ---- workgroup-balanced enumeration of tile rects (full lists only: parity tests, the reference's `debug` flag) ----------
// Each of the 1024 threads owns one Gaussian with `count` tiles (0 if culled) in rect [rmin, rmax).  Tile counts
// are extremely skewed (BASELINE cfg3: median 6 tiles, 99.9th percentile 484, maximum 4056), so the WORKGROUP walks the
// concatenation of all 1024 rects with every thread busy: item k belongs to the thread whose inclusive prefix first
// exceeds k (binary search in an LDS copy of the prefix), and its tile follows from k's offset inside that rect.
struct RectWork {
    uint32_t* prefix;  // LDS [NT] inclusive prefix of counts
    uint32_t* rx;      // LDS [NT] rect_min.x | width << 16
    uint32_t* ry;      // LDS [NT] rect_min.y
    uint32_t* wsum;    // LDS [16]
};

// Contains workgroup barriers: call from all NT threads.  f(owner_thread, tile_x, tile_y) handles one item.
template <int NT = 1024, typename F>
__device__ __forceinline__ void for_each_tile_balanced(const RectWork& rw, int tid, uint2 rmin, uint2 rmax, uint32_t count, F&& f)
{
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t incl = wave_inclusive_scan(count, lane);
    if (lane == 63) rw.wsum[wave] = incl;
    __syncthreads();
    uint32_t woff = 0, total = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; w++) {
        const uint32_t c = rw.wsum[w];
        woff += w < wave ? c : 0u;
        total += c;
    }
    incl += woff;
    rw.prefix[tid] = incl;
    rw.rx[tid] = rmin.x | ((rmax.x - rmin.x) << 16);
    rw.ry[tid] = rmin.y;
    __syncthreads();
    for (uint32_t k = (uint32_t)tid; k < total; k += NT) {
        // first thread o with prefix[o] > k
        int lo = 0;
#pragma unroll
        for (int step = NT / 2; step >= 1; step >>= 1)
            if (rw.prefix[lo + step - 1] <= k) lo += step;
        const uint32_t packed = rw.rx[lo];
        const uint32_t w = packed >> 16, x0 = packed & 0xFFFFu, y0 = rw.ry[lo];
        const uint32_t prev = lo == 0 ? 0u : rw.prefix[lo - 1];
        const uint32_t i = k - prev;
        // row = i / w without an integer divide: (i + 0.5) / w is never within float error of an integer
        // boundary for i < 2^14 * w (a Gaussian covers at most grid_x * grid_y tiles)
        const uint32_t row = (uint32_t)(((float)i + 0.5f) * __builtin_amdgcn_rcpf((float)w));
        const uint32_t col = i - row * w;
        f((uint32_t)lo, x0 + col, y0 + row);
    }
    __syncthreads();  // LDS hand-off arrays are reused by the next call
}

inline int bin_workgroups(int P)
{
    const int blocks = (P + BIN_THREADS - 1) / BIN_THREADS;
    return blocks < 1 ? 1 : (blocks > BIN_MAX_WG ? BIN_MAX_WG : blocks);
}

// Emit pass of the FULL lists (the reference's `debug` flag, MI_RAST_FULL_LISTS: parity tests): every overlap of the
// reference's rects is stored, with the quadrant mask the lean lists would give it (cull.h: span_tile_mask; 0 = culled) in
// the top 4 bits -- the per-tile sort then reproduces the reference's point_list (the low 28 bits of the blend list), and the blend
// kernels skip the entries without a mask bit.  NOCULL (testing aid, MI_RAST_NO_CULL): every overlap is kept with all four quadrant bits.
template <bool NOCULL = false>
__global__ void __launch_bounds__(BIN_THREADS) bin_ranks_kernel(int P, const BlendRec* __restrict__ index_rec,
                                                                const uint32_t* __restrict__ depth_key,
                                                                const uint32_t* __restrict__ partial,
                                                                const uint2* __restrict__ ranges,
                                                                uint2* __restrict__ entries, uint32_t gx, uint32_t gy,
                                                                uint32_t by0, uint32_t by1)
{
    // One launch covers the tile rows [by0, by1) (the whole image unless it has more tiles than LDS counters: then the host
    // walks it in bands); the LDS cursors are indexed relative to the band, everything in memory by the global tile id.
    extern __shared__ uint32_t s_dyn[];  // [band tiles] cursors, then the rect hand-off arrays
    const int ntiles = (int)(gx * (by1 - by0));
    const int tile0 = (int)(gx * by0);
    const int ntiles_all = (int)(gx * gy);
    uint32_t* s_cnt = s_dyn;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t* s_rw = s_dyn + ((ntiles + 3) & ~3);  // 16-byte aligned
    RectWork rw{s_rw, s_rw + 1024, s_rw + 2048, s_rw + 3072};
    float2* s_xy = reinterpret_cast<float2*>(s_rw + 3088);          // the owners' means ...
    float4* s_co = reinterpret_cast<float4*>(s_rw + 3088 + 2048);   // ... conics + opacities ...
    uint32_t* s_rad = s_rw + 3088 + 6144;                           // ... radii ...
    uint32_t* s_key = s_rw + 3088 + 7168;                           // ... and depth bits
    const uint32_t* my_partial = partial + (size_t)slice_row(blockIdx.x, gridDim.x) * ntiles_all + tile0;
    for (int t = tid; t < ntiles; t += BIN_THREADS) s_cnt[t] = ranges[tile0 + t].x + my_partial[t];
    __syncthreads();
    // 64-index chunks are dealt round robin over all the waves of all the workgroups: chunk c belongs to workgroup
    // c % nwg, wave slot (c / nwg) % 16, round (c / nwg) / 16
    const int nwg = (int)gridDim.x;
    const int rounds = ((P + 63) / 64 + 16 * nwg - 1) / (16 * nwg);
    for (int it = 0; it < rounds; it++) {
        const int r = ((it * 16 + wave) * nwg + (int)blockIdx.x) * 64 + lane;
        uint2 rmin = make_uint2(0, 0), rmax = make_uint2(0, 0);
        uint32_t count = 0;
        if (r < P) {
            const uint32_t key = depth_key[r];
            if (key != 0xFFFFFFFFu) {   // visible (geometry.h: radius > 0), so its record was written
                const BlendRec rec = index_rec[r];
                getRect(rec.xy.x, rec.xy.y, (int)rec.pm, rmin, rmax, gx, gy);
                rmin.y = max(rmin.y, by0);  // this band's rows only
                rmax.y = min(rmax.y, by1);
                count = rmax.y > rmin.y ? (rmax.x - rmin.x) * (rmax.y - rmin.y) : 0u;
                s_xy[tid] = rec.xy;
                s_co[tid] = rec.co;
                s_rad[tid] = rec.pm;
                s_key[tid] = key;
            }
        }
        for_each_tile_balanced(rw, tid, rmin, rmax, count, [&](uint32_t owner, uint32_t tx, uint32_t ty) {
            const uint32_t qmask = NOCULL ? 15u : span_tile_mask(s_xy[owner], s_co[owner], (int)s_rad[owner], tx, ty, gx, gy);
            const uint32_t id = (uint32_t)(((it * 16 + (int)(owner >> 6)) * nwg + (int)blockIdx.x) * 64 + (int)(owner & 63u));
            const uint32_t slot = atomicAdd(&s_cnt[(ty - by0) * gx + tx], 1u);
            entries[slot] = make_uint2(s_key[owner], id | (qmask << ID_BITS));
        });
    }
}

// Count pass without enumerating the overlaps: every rect adds +1 / -1 / -1 / +1 at its four corners of a
// (gy + 1) x (gx + 1) difference grid in LDS (four LDS atomics per Gaussian instead of one per covered tile plus a
// ten-step owner search), and a 2-D prefix sum of the grid is the number of rects covering each tile -- exactly what
// an enumeration would count.  Same slices (index chunks dealt round robin) and the same rects as bin_ranks_kernel: the count
// pass of the FULL lists.
__global__ void __launch_bounds__(BIN_THREADS) bin_count_kernel(int P, const BlendRec* __restrict__ index_rec,
                                                                const uint32_t* __restrict__ depth_key,
                                                                uint32_t* __restrict__ partial, uint32_t gx, uint32_t gy_all,
                                                                uint32_t by0, uint32_t by1, const int* __restrict__ r_slots,
                                                                int* __restrict__ host_r)
{
    // tile rows [by0, by1) of the image (see bin_ranks_kernel); the difference grid covers the band only
    extern __shared__ int s_grid[];  // [(band rows + 1) * stride]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the partial sums of R for the host (see bin_spans_kernel)
    if (host_r != nullptr && blockIdx.x == 0 && tid < R_SLOTS) host_r[tid * R_SLOT_STRIDE] = r_slots[tid * R_SLOT_STRIDE];
    const int stride = count_grid_stride(gx);
    const uint32_t gy = by1 - by0;
    const int cells = (int)(gy + 1) * stride;
    for (int c = tid; c < cells; c += BIN_THREADS) s_grid[c] = 0;
    __syncthreads();
    const int nwg = (int)gridDim.x;
    const int rounds = ((P + 63) / 64 + 16 * nwg - 1) / (16 * nwg);
    for (int it = 0; it < rounds; it++) {
        const int r = ((it * 16 + wave) * nwg + (int)blockIdx.x) * 64 + lane;  // same dealing as bin_ranks_kernel
        if (r >= P) continue;
        if (depth_key[r] == 0xFFFFFFFFu) continue;
        const BlendRec rec = index_rec[r];
        uint2 rmin, rmax;
        getRect(rec.xy.x, rec.xy.y, (int)rec.pm, rmin, rmax, gx, gy_all);
        rmin.y = max(rmin.y, by0);
        rmax.y = min(rmax.y, by1);
        if (rmax.x <= rmin.x || rmax.y <= rmin.y) continue;
        rmin.y -= by0;
        rmax.y -= by0;
        atomicAdd(&s_grid[rmin.y * stride + rmin.x], 1);
        atomicAdd(&s_grid[rmin.y * stride + rmax.x], -1);
        atomicAdd(&s_grid[rmax.y * stride + rmin.x], -1);
        atomicAdd(&s_grid[rmax.y * stride + rmax.x], 1);
    }
    __syncthreads();
    // prefix along x: one wave per row, 64 cells at a time with a carry
    for (int y = wave; y < (int)gy; y += BIN_THREADS / 64) {
        int carry = 0;
        for (int x0 = 0; x0 < (int)gx; x0 += 64) {
            const int x = x0 + lane;
            int v = x < (int)gx ? s_grid[y * stride + x] : 0;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {   // (not wave_inclusive_scan: the kernel's code would change)
                const int t = __shfl_up(v, o, 64);
                if (lane >= o) v += t;
            }
            v += carry;
            if (x < (int)gx) s_grid[y * stride + x] = v;
            carry = __shfl(v, 63, 64);
        }
    }
    __syncthreads();
    // prefix along y: one thread per column; the running sums are the per-tile counts of this slice
    uint32_t* my_partial = partial + (size_t)slice_row(blockIdx.x, gridDim.x) * (gx * gy_all) + (size_t)gx * by0;
    for (int x = tid; x < (int)gx; x += BIN_THREADS) {
        int run = 0;
        for (int y = 0; y < (int)gy; y++) {
            run += s_grid[y * stride + x];
            s_grid[y * stride + x] = run;
        }
    }
    __syncthreads();
    for (int t = tid; t < (int)(gx * gy); t += BIN_THREADS) my_partial[t] = (uint32_t)s_grid[(t / (int)gx) * stride + (t % (int)gx)];
}

// Per tile: exclusive prefix of partial[slice][tile] over the slices (in place) and tile_total[tile].
// One workgroup handles 64 tiles x 16 groups of slices; every load is coalesced along the tile axis.
__global__ void __launch_bounds__(1024) scan_partials_kernel(int ntiles, int nwg, uint32_t* __restrict__ partial,
                                                             uint32_t* __restrict__ tile_total)
{
    __shared__ uint32_t s_sum[16][64];
    const int tl = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + tl;
    const int wpg = (nwg + 15) / 16;
    const int w0 = g * wpg, w1 = min(nwg, w0 + wpg);
    uint32_t sum = 0;
    if (t < ntiles)
        for (int w = w0; w < w1; w++) sum += partial[(size_t)w * ntiles + t];
    s_sum[g][tl] = sum;
    __syncthreads();
    uint32_t run = 0;
    for (int gg = 0; gg < g; gg++) run += s_sum[gg][tl];
    if (t < ntiles) {
        for (int w = w0; w < w1; w++) {
            const uint32_t c = partial[(size_t)w * ntiles + t];
            partial[(size_t)w * ntiles + t] = run;
            run += c;
        }
        if (g == 15) tile_total[t] = run;
    }
}

}  // namespace mirast
