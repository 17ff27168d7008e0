// bin_lean.h -- count and emit passes of the LEAN lists (the product default): only the (Gaussian, tile) overlaps that can reach
// alpha >= 1/255 in the tile, found from closed-form row spans (cull.h) without a per-tile test.  Contract: the preprocess pass
// (geometry.h) leaves one bit per (band of tile rows, Gaussian) and the Gaussians per band; band_plan deals the workgroups to the bands;
// bin_spans_kernel<false> counts per (workgroup, tile of its band) and takes each workgroup's offset inside a tile's segment with one
// atomic on tile_total[tile] -- no table of slices, no scan; tile_ranges_kernel (tile_ranges.h) makes the ranges; bin_spans_kernel<true>
// re-takes the same decisions and stores one 8-byte entry {depth bits, id | quadrant mask << 28} per overlap.  A tile is counted iff an
// entry is stored for it: the counts are the lists' exact lengths.  Order inside a segment is arbitrary; tile_sort.h orders it.
#pragma once

#include "blend_rec.h"
#include "common.h"
#include "cull.h"
#include "wave.h"

namespace mirast {

constexpr int BIN_LEAN_WG = 256;       // workgroups of the LEAN count / emit passes (dealt to the bands by load: band_plan)

// ---- bands of tile rows (lean count / emit passes) ----------------------------------------------------------------------------
// The lean passes walk the image in <= MAX_BANDS bands of band_h tile rows.  A workgroup belongs to ONE band: its LDS counters / cursors
// cover that band's tiles only, and -- the point -- the entries it stores go to a few hundred tile segments instead of all of them:
// ~22 consecutive entries per (workgroup, tile) on cfg3 instead of 1.4, which the L2 of the workgroup's XCD merges into whole lines
// (tools/write_combine_probe.hip: the same 2.93 M eight-byte stores take 16.5 us banded, 30 us with every workgroup storing into every
// tile's segment; WRITE_SIZE of rounds 2-5 was 64 bytes per entry).  The preprocess pass leaves, per band, one bit per Gaussian (band_bits[band][index chunk]:
// a wave's ballot) and the number of Gaussians per band (r_slots); a band gets workgroups in proportion to that number (band_plan), every workgroup an
// equal share of the Gaussian INDEX range, of which it picks the Gaussians with its band's bit (64 Gaussians per word).
__host__ __device__ inline bool band_geometry(uint32_t gx, uint32_t gy, uint32_t max_head_words, uint32_t& band_h, uint32_t& nbands)
{
    band_h = (gy + 15u) / 16u;
    if (band_h < 1u) band_h = 1u;
    while (band_h > 1u && (band_h + 1u) * (gx + 2u) > max_head_words) band_h--;   // (+ 1: the count pass's difference grid has an odd stride >= gx + 1)
    nbands = (gy + band_h - 1u) / band_h;
    return nbands <= (uint32_t)MAX_BANDS && (band_h + 1u) * (gx + 2u) <= max_head_words;
}

// s_plan[b] = first workgroup of band b, s_plan[nbands] = workgroups in use (<= nwg): one workgroup per band plus the rest in
// proportion to the bands' Gaussian counts.  Call from one whole wave; every kernel that needs the plan recomputes it from the same
// counters with this same code.
__device__ __forceinline__ void band_plan(const int* __restrict__ r_slots, uint32_t nbands, uint32_t nwg, uint32_t* s_plan, int lane)
{
    uint32_t cnt = 0;
    if ((uint32_t)lane < nbands)
        for (int k = 0; k < R_SLOTS; k++) cnt += (uint32_t)r_slots[k * R_SLOT_STRIDE + R_SLOT_BANDS + lane];
    const uint32_t total = wave_sum(cnt);
    const uint32_t avail = nwg > nbands ? nwg - nbands : 0u;
    uint32_t n = (uint32_t)lane < nbands ? 1u + (total ? (uint32_t)(((uint64_t)cnt * avail) / total) : 0u) : 0u;
    if (nwg < nbands) n = (uint32_t)lane < nwg ? 1u : 0u;   // (never launched so: the host gives at least one workgroup per band)
    const uint32_t incl = wave_inclusive_scan(n, lane);
    if ((uint32_t)lane < nbands) s_plan[lane] = incl - n;
    if ((uint32_t)lane == nbands) s_plan[nbands] = incl;   // (lanes >= nbands hold the grand total: n = 0 there)
}

// ---- lean lists from row spans (the product default) ------------------------------------------------------------
// The count and emit passes of the lean lists without a single per-tile test, WAVE-GRANULAR (round 6).  A wave takes a chunk of
// 64 consecutive Gaussians (the next chunk of its workgroup's slice from an LDS counter; its records are requested one chunk
// ahead), and walks
//   level 1: the (Gaussian, tile row) items of the chunk, 64 at a time, balanced over the lanes (a Gaussian covers 1 .. 68
//            rows): item k belongs to the lane whose inclusive prefix of row counts first exceeds k (wave.h: wave_owner, one
//            LDS round trip and a DPP scan).  Each item evaluates the two closed-form column intervals of its row's upper
//            and lower 8-pixel band (cull.h: band_columns) and gets the tile span [x0, x1) that holds them;
//   COUNT (EMIT = false): +1 / -1 at the two ends of the span in a per-row difference grid in LDS (shared by the workgroup's
//            16 waves: LDS atomics); the prefix along x is the number of spans covering each tile -- this slice's share of the
//            tile's segment, EXACTLY: a tile is counted iff the emit pass stores an entry for it;
//   EMIT:    level 2, the tiles of the 64 spans of a window, balanced again: the quadrant mask of a tile is read off the two
//            column intervals (four range tests on integers), the slot comes from the LDS cursor of the tile.
// The waves of a workgroup share nothing but the counters / cursors: no workgroup barrier between the first store of a
// counter and the last (rounds 2-5 ran this as 1024-thread phases between workgroup barriers: count 0.036 ms, emit 0.071 ms
// on cfg3, ~1 us per phase whatever it computed).  Hand-offs between the lanes of a wave go through wave-private LDS words;
// LDS operations of one wave execute in program order, the wavefront fences keep the compiler from reordering them.
// Measured on cfg3: 2.27 M (Gaussian, row) items, 2.93 M entries.
constexpr int BW_WORDS = 64 * 18;  // LDS words per wave: prefix, rect, depth bits, id, owner scratch, two float4 of span constants + mean, the ids of a chunk; emit: span prefix, two bands' columns, span origin
__host__ __device__ constexpr size_t span_lds_bytes(size_t head_words) { return (((head_words + 3) & ~(size_t)3) + 4 + 16 * BW_WORDS) * sizeof(uint32_t); }
constexpr uint32_t SPAN_MAX_HEAD_WORDS = 40 * 1024 - 16 * BW_WORDS - 64;   // counters / cursors of one band: what is left of 160 KB

template <bool EMIT>
__global__ void __launch_bounds__(1024) bin_spans_kernel(int P, const BlendRec* __restrict__ index_rec,
                                                         const uint32_t* __restrict__ depth_key, const unsigned long long* __restrict__ band_bits,
                                                         uint32_t* __restrict__ partial, uint32_t* __restrict__ tile_total, const uint2* __restrict__ ranges,
                                                         uint2* __restrict__ entries, uint32_t gx, uint32_t gy_all,
                                                         uint32_t band_h, uint32_t nbands, const int* __restrict__ r_slots,
                                                         int* __restrict__ host_r)
{
    // COUNT: s_dyn = difference grid [band rows][stride] (ints), then the chunk counter and the waves' hand-off words
    // EMIT : s_dyn = cursors [band tiles], then the same
    extern __shared__ uint32_t s_dyn[];
    __shared__ uint32_t s_plan[MAX_BANDS + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // The first kernel behind the preprocess pass hands the partial sums of R to the host: plain stores into its pinned buffer
    // (a copy command of 8 KB costs a 5-us blit kernel on the stream); the event behind this kernel tells the host they are there.
    if (!EMIT && host_r != nullptr && blockIdx.x == 0 && tid < R_SLOTS) host_r[tid * R_SLOT_STRIDE] = r_slots[tid * R_SLOT_STRIDE];
    if (wave == 0) band_plan(r_slots, nbands, gridDim.x, s_plan, lane);
    __syncthreads();
    if (blockIdx.x >= s_plan[nbands]) return;   // (workgroups the plan leaves over)
    uint32_t band = 0;
    while (band + 1u < nbands && s_plan[band + 1u] <= blockIdx.x) band++;
    const uint32_t nsub = s_plan[band + 1u] - s_plan[band], sub = blockIdx.x - s_plan[band];
    const uint32_t by0 = band * band_h, by1 = min(gy_all, by0 + band_h);
    const uint32_t band_bit = 1u << band;
    const uint32_t gy = by1 - by0;
    const int stride = count_grid_stride(gx);
    const int ntiles = (int)(gx * gy);
    const int tile0 = (int)(gx * by0);
    const int head = EMIT ? ((ntiles + 3) & ~3) : (((int)gy * stride + 3) & ~3);
    uint32_t* s_cnt = s_dyn;
    int* s_grid = reinterpret_cast<int*>(s_dyn);
    uint32_t* s_next = s_dyn + head;   // [4]: next group of mask chunks of this workgroup's share
    uint32_t* wb = s_dyn + head + 4 + wave * BW_WORDS;
    uint32_t* w_pre = wb;              // inclusive prefix of the lanes' row counts
    uint32_t* w_rect = wb + 64;        // clip columns x0 | x1 << 10, first row << 21
    uint32_t* w_key = wb + 128;        // depth bits
    uint32_t* w_own = wb + 192;        // scratch of wave_owner
    float4* w_c0 = reinterpret_cast<float4*>(wb + 256);   // span constants of the Gaussian (cull.h: SpanPre): B, 1/A, 2 tau A, det
    float4* w_c1 = reinterpret_cast<float4*>(wb + 512);   //   ey (negative: no culling), y*, mean x, mean y
    uint32_t* w_tpre = wb + 768;       // EMIT, per span of the window: inclusive prefix of the spans' widths
    uint32_t* w_q0 = wb + 832;         //   upper band's columns lo | hi << 11, owner lane << 22
    uint32_t* w_q1 = wb + 896;         //   lower band's columns lo | hi << 11
    uint32_t* w_sx = wb + 960;         //   first tile column | tile row << 10
    uint32_t* w_id = wb + 1024;        // Gaussian id of the lane's record
    uint32_t* w_queue = wb + 1088;     // [64]: ids of the chunk being put together
    uint32_t* my_partial = partial + (size_t)blockIdx.x * (band_h * gx);   // [workgroup][tile of its band]
    if (EMIT) {
        for (int t = tid; t < ntiles; t += 1024) s_cnt[t] = ranges[tile0 + t].x + my_partial[t];
    } else {
        for (int c = tid; c < (int)gy * stride; c += 1024) s_grid[c] = 0;
    }
    if (tid == 0) s_next[0] = 0u;
    __syncthreads();
    // This workgroup's share of the Gaussians: index chunks (64 consecutive indices) [mc0, mc1) of the view's, an equal part of the
    // index range for each of the band's workgroups.
    const uint32_t nchunks_all = ((uint32_t)P + 63u) / 64u;
    const uint32_t mc0 = (uint32_t)(((uint64_t)sub * nchunks_all) / nsub), mc1 = (uint32_t)(((uint64_t)(sub + 1u) * nchunks_all) / nsub);
    // The band's Gaussians come as bit words: band_bits[band][c] = which of the 64 Gaussians of index chunk c reach this band
    // (geometry.h).  A wave takes UNITS of 32 words (2048 Gaussians) from the workgroup's LDS counter, one unit requested ahead; the
    // set bits of a unit are ranked (popcount + DPP scan over the lanes' words), and a chunk of <= 64 Gaussians is the next 64 ranks:
    // every lane whose word holds some of them walks its set bits and leaves the ids in the wave's queue.
    constexpr uint32_t UNIT = 32;
    const unsigned long long* my_bits = band_bits + (size_t)band * nchunks_all;
    uint32_t g_unit = 0, g_next;                    // first index chunk of the unit being sifted / of the one requested ahead
    unsigned long long word = 0ull, nword;          // lane L < 32: the word of chunk g_unit + L
    uint32_t cnt = 0, incl = 0, total = 0, r0 = 0;  // the lane's set bits, their inclusive prefix over the lanes, the unit's sum, ranks taken so far
    auto request_unit = [&]() __attribute__((always_inline)) {
        uint32_t u = 0;
        if (lane == 0) u = atomicAdd(s_next, 1u);
        g_next = mc0 + UNIT * (uint32_t)__builtin_amdgcn_readfirstlane(u);
        nword = my_bits[min(g_next + (uint32_t)lane, nchunks_all - 1u)];   // (unconditional, clamped; validity is applied in next_unit)
    };
    auto next_unit = [&]() __attribute__((always_inline)) {
        g_unit = g_next;
        word = ((uint32_t)lane < UNIT && g_unit + (uint32_t)lane < mc1) ? nword : 0ull;
        request_unit();
        cnt = (uint32_t)__builtin_popcountll(word);
        incl = wave_inclusive_scan_dpp(cnt);
        total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        r0 = 0;
    };
    // next chunk of <= 64 Gaussians of this band -> id (0xFFFFFFFF: lane without one); false: this workgroup's share is exhausted
    auto take_chunk = [&](uint32_t& id) __attribute__((always_inline)) -> bool {
        uint32_t qn = 0;
        while (qn < 64u) {
            if (r0 == total) {
                if (g_next >= mc1) break;
                next_unit();
                continue;
            }
            const uint32_t t = min(64u - qn, total - r0);
            uint32_t rk = incl - cnt;   // rank of this lane's first set bit
            if (incl > r0 && rk < r0 + t) {
                for (unsigned long long w = word; w != 0ull; w &= w - 1ull, rk++)
                    if (rk >= r0 && rk < r0 + t) w_queue[qn + rk - r0] = (g_unit + (uint32_t)lane) * 64u + (uint32_t)__builtin_ctzll(w);
            }
            r0 += t;
            qn += t;
        }
        if (qn == 0u) return false;
        wave_lds_fence();
        id = (uint32_t)lane < qn ? w_queue[lane] : 0xFFFFFFFFu;
        wave_lds_fence();
        return true;
    };
    request_unit();
    uint32_t nid = 0xFFFFFFFFu;
    bool have = take_chunk(nid);
    BlendRec nrec = index_rec[nid == 0xFFFFFFFFu ? 0u : nid];
    while (have) {
        const uint32_t id = nid;
        const BlendRec rec = nrec;
        // the next chunk's ids, and its records requested before this chunk's items are walked
        nid = 0xFFFFFFFFu;
        have = take_chunk(nid);
        nrec = index_rec[nid == 0xFFFFFFFFu ? 0u : nid];
        uint32_t h = 0;
        if (id != 0xFFFFFFFFu) {   // visible (its band bit was set): radius > 0, record written (geometry.h)
            const int rad = (int)rec.pm;
            uint2 rmin, rmax;
            getRect(rec.xy.x, rec.xy.y, rad, rmin, rmax, gx, gy_all);
            shrink_rect(rec.xy, rec.co, rad, rmin, rmax);
            rmin.y = max(rmin.y, by0);
            rmax.y = min(rmax.y, by1);
            if (rmax.x > rmin.x && rmax.y > rmin.y) {
                h = rmax.y - rmin.y;
                // the span constants ONCE per Gaussian (two square roots, a logarithm, three reciprocals), not once per row item
                const SpanPre pre = span_prepare(rec.co, rad);
                w_c0[lane] = make_float4(pre.B, pre.rcpA, pre.twotauA, pre.det);
                w_c1[lane] = make_float4(pre.cull ? pre.ey : -1.0f, pre.ystar, rec.xy.x, rec.xy.y);
                w_rect[lane] = rmin.x | (rmax.x << 10) | (rmin.y << 21);
                if (EMIT) {
                    w_key[lane] = rec.id;   // depth bits (BlendRec)
                    w_id[lane] = id;
                }
            }
        }
        const uint32_t hincl = wave_inclusive_scan_dpp(h);
        const uint32_t rows_total = (uint32_t)__builtin_amdgcn_readlane((int)hincl, 63);
        w_pre[lane] = hincl;
        wave_lds_fence();
        for (uint32_t w0 = 0; w0 < rows_total; w0 += 64) {  // windows of 64 (Gaussian, tile row) items
            const uint32_t k = w0 + (uint32_t)lane;
            uint32_t width = 0;
            const uint32_t g = wave_owner(w_own, hincl - h, hincl, w0, lane);
            if (k < rows_total) {
                const uint32_t prev = g == 0u ? 0u : w_pre[g - 1];
                const uint32_t packed = w_rect[g];
                const float4 c0 = w_c0[g], c1 = w_c1[g];
                const uint32_t cx0 = packed & 1023u, cx1 = (packed >> 10) & 2047u, ty = (packed >> 21) + (k - prev);
                SpanPre pre;
                pre.B = c0.x;
                pre.rcpA = c0.y;
                pre.twotauA = c0.z;
                pre.det = c0.w;
                pre.cull = c1.x >= 0.f;
                pre.ey = c1.x;
                pre.ystar = c1.y;
                const float2 xy = make_float2(c1.z, c1.w);
                int lo0, hi0, lo1, hi1;
                band_columns(pre, xy, (float)(ty * TILE_Y), (int)(2u * cx0), (int)(2u * cx1), lo0, hi0);
                band_columns(pre, xy, (float)(ty * TILE_Y + 8u), (int)(2u * cx0), (int)(2u * cx1), lo1, hi1);
                if (hi0 > lo0 || hi1 > lo1) {
                    const int lo = hi0 > lo0 ? (hi1 > lo1 ? min(lo0, lo1) : lo0) : lo1;
                    const int hi = hi0 > lo0 ? (hi1 > lo1 ? max(hi0, hi1) : hi0) : hi1;
                    const uint32_t sx0 = (uint32_t)lo >> 1, sx1 = ((uint32_t)hi + 1u) >> 1;
                    if (EMIT) {
                        width = sx1 - sx0;
                        w_q0[lane] = (uint32_t)lo0 | ((uint32_t)hi0 << 11) | (g << 22);
                        w_q1[lane] = (uint32_t)lo1 | ((uint32_t)hi1 << 11);
                        w_sx[lane] = sx0 | (ty << 10);
                    } else {
                        // EXACT counts: a tile is counted iff one of the two intervals has a column in it, i.e. iff the emit
                        // pass finds a non-zero mask there -- the two bands' tile ranges separately when a gap lies between them
                        int* row = s_grid + (ty - by0) * stride;
                        const int a0 = lo0 >> 1, b0 = (hi0 + 1) >> 1, a1 = lo1 >> 1, b1 = (hi1 + 1) >> 1;
                        if (hi0 > lo0 && hi1 > lo1 && (b0 < a1 || b1 < a0)) {
                            atomicAdd(&row[a0], 1);
                            atomicAdd(&row[b0], -1);
                            atomicAdd(&row[a1], 1);
                            atomicAdd(&row[b1], -1);
                        } else {
                            atomicAdd(&row[sx0], 1);
                            atomicAdd(&row[sx1], -1);
                        }
                    }
                }
            }
            if (EMIT) {
                const uint32_t tincl = wave_inclusive_scan_dpp(width);
                const uint32_t tiles_total = (uint32_t)__builtin_amdgcn_readlane((int)tincl, 63);
                w_tpre[lane] = tincl;
                wave_lds_fence();
                for (uint32_t t0 = 0; t0 < tiles_total; t0 += 64) {   // windows of 64 tiles of the spans
                    const uint32_t kk = t0 + (uint32_t)lane;
                    const uint32_t o = wave_owner(w_own, tincl - width, tincl, t0, lane);
                    if (kk < tiles_total) {
                        const uint32_t prevt = o == 0u ? 0u : w_tpre[o - 1];
                        const uint32_t q0 = w_q0[o], q1 = w_q1[o], sx = w_sx[o];
                        const uint32_t tx = (sx & 1023u) + (kk - prevt), ty = sx >> 10;
                        const uint32_t lo0 = q0 & 2047u, n0 = ((q0 >> 11) & 2047u) - lo0, lo1 = q1 & 2047u, n1 = ((q1 >> 11) & 2047u) - lo1;
                        const uint32_t c = 2u * tx;
                        const uint32_t qmask = (uint32_t)(c - lo0 < n0) | ((uint32_t)(c + 1u - lo0 < n0) << 1) |
                                               ((uint32_t)(c - lo1 < n1) << 2) | ((uint32_t)(c + 1u - lo1 < n1) << 3);
                        if (qmask != 0u) {
                            const uint32_t gg = q0 >> 22;
                            const uint32_t slot = atomicAdd(&s_cnt[(ty - by0) * gx + tx], 1u);
                            entries[slot] = make_uint2(w_key[gg], w_id[gg] | (qmask << ID_BITS));
                        }
                    }
                }
                wave_lds_fence();   // the spans' words are rewritten by the next window
            }
        }
        wave_lds_fence();   // the Gaussians' words are rewritten by the next chunk
    }
    if (!EMIT) {
        __syncthreads();
        // prefix along x: one wave per row, 64 cells at a time with a carry -> the per-tile counts of this workgroup
        for (int y = wave; y < (int)gy; y += 16) {
            int carry = 0;
            for (int x0 = 0; x0 < (int)gx; x0 += 64) {
                const int x = x0 + lane;
                int v = x < (int)gx ? s_grid[y * stride + x] : 0;
                v = (int)wave_inclusive_scan_dpp((uint32_t)v) + carry;   // (two's complement: the signed differences add up like unsigned words)
                // this workgroup's entries of the tile take the next v slots of the tile's segment: one returning atomic per
                // (workgroup, non-empty tile) on the tile's total -- ~130 K of them per cfg3 view, ~18 per address, in place of a
                // partial[slice][tile] table and its scan (the order of the workgroups inside a segment is whatever the atomics
                // make it: the per-tile sort does not care)
                if (x < (int)gx) my_partial[y * (int)gx + x] = v != 0 ? atomicAdd(&tile_total[tile0 + y * (int)gx + x], (uint32_t)v) : 0u;
                carry = __builtin_amdgcn_readlane(v, 63);
            }
        }
    }
}

}  // namespace mirast
