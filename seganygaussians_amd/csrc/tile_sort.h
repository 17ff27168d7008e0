// tile_sort.h -- per-tile sort: orders the 8-byte entries {depth bits, id | quadrant mask << 28} of every tile's segment by (depth
// bits, Gaussian id) -- the reference's order of point_list -- and writes the tile's BLEND LIST, four bytes per entry.  Lists of up
// to TILE_SORT_WAVE_MAX entries: one wave per tile, a bitonic network in registers (three length classes); longer ones: one workgroup
// per tile, LSD radix sort in LDS or, beyond its capacity, ping-pong in HBM.  Also verify_entries_kernel (MI_RAST_VERIFY_LISTS).
#pragma once

#include "blend_rec.h"
#include "wave.h"

namespace mirast {

// ---- per-tile LDS radix sort of the entries by depth bits ------------------------------------------------
// (key, value) pair storage: two LDS arrays, or one uint2 array in HBM
struct LdsPairs {
    uint32_t* k;
    uint32_t* v;
    __device__ __forceinline__ uint32_t key(int i) const { return k[i]; }
    __device__ __forceinline__ uint32_t val(int i) const { return v[i]; }
    __device__ __forceinline__ void set(int i, uint32_t kk, uint32_t vv) const
    {
        k[i] = kk;
        v[i] = vv;
    }
};
struct GlobalPairs {
    uint2* p;
    __device__ __forceinline__ uint32_t key(int i) const { return p[i].x; }
    __device__ __forceinline__ uint32_t val(int i) const { return p[i].y; }
    __device__ __forceinline__ void set(int i, uint32_t kk, uint32_t vv) const { p[i] = make_uint2(kk, vv); }
};

// One workgroup (256 threads for short lists, 1024 for long ones) per tile; handles tiles with LO < n <= CAP in LDS; when GLOBAL_FALLBACK is set it
// also handles n > CAP by ping-ponging between `entries` and `scratch` in HBM with the same code.
// LSD radix over the depth bits, 8-bit digits, ceil(key_bits / 8) passes (key_bits: the low bits in which the view's keys differ,
// from the range scan).  Each wave owns a contiguous share of the tile's list; per pass: per-wave digit histograms -> workgroup scan
// over (digit, wave) -> each wave scatters its share 64 pairs at a time with a stable ballot-match rank.  Three workgroup barriers per pass.
// MAXB > 0 (lists held in LDS: a wave's share is at most MAXB batches of 64 pairs): the pairs and their match results
// (rank among the wave's equal digits, size of that group) stay in registers between the histogram and the scatter
// phase -- the eight-ballot match is evaluated once per pair and pass instead of twice.  MAXB = 0: any length (the
// HBM fallback), everything re-read and re-matched in the scatter phase.
template <int NW, int MAXB, typename Src, typename Dst>
__device__ __forceinline__ void radix_pass(Src src, Dst dst, int n, int shift, uint32_t (*s_hist)[256], int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
    // contiguous share per wave (NW waves), in multiples of 64 keys
    const int chunks = (n + 63) >> 6;
    const int cpw = (chunks + NW - 1) / NW;
    const int begin = min(n, wave * cpw * 64), end = min(n, (wave + 1) * cpw * 64);
    for (int d = tid; d < NW * 256; d += NW * 64) (&s_hist[0][0])[d] = 0;
    __syncthreads();

    auto match = [&](uint32_t digit, bool active, uint32_t& rank_in_wave, uint32_t& cnt) {
        uint64_t m = ballot64(active);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const uint64_t bal = ballot64(active && ((digit >> b) & 1u));
            m &= ((digit >> b) & 1u) ? bal : ~bal;
        }
        rank_in_wave = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        cnt = (uint32_t)__builtin_popcountll(m);
    };

    constexpr int NB = MAXB > 0 ? MAXB : 1;
    uint32_t c_key[NB], c_val[NB], c_rk[NB], c_cnt[NB];
    // (a) per-wave histogram of this digit
    if (MAXB > 0) {
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const int i0 = begin + 64 * j;
            if (i0 >= end) break;  // wave-uniform
            const int i = i0 + lane;
            const bool active = i < end;
            c_key[j] = active ? src.key(i) : 0u;
            c_val[j] = active ? src.val(i) : 0u;
            const uint32_t digit = (c_key[j] >> shift) & 0xFFu;
            match(digit, active, c_rk[j], c_cnt[j]);
            if (active && c_rk[j] == 0) s_hist[wave][digit] += c_cnt[j];  // one lane per distinct digit, wave-private row
        }
    } else {
        for (int i0 = begin; i0 < end; i0 += 64) {
            const int i = i0 + lane;
            const bool active = i < end;
            const uint32_t key = active ? src.key(i) : 0u;
            const uint32_t digit = (key >> shift) & 0xFFu;
            uint32_t rk, cnt;
            match(digit, active, rk, cnt);
            if (active && rk == 0) s_hist[wave][digit] += cnt;
        }
    }
    __syncthreads();
    // (b) exclusive scan over (digit major, wave minor): thread d < 256 owns digit d
    {
        __shared__ uint32_t s_wsum[4];
        uint32_t tot = 0, incl = 0;
        if (tid < 256) {
#pragma unroll
            for (int w = 0; w < NW; w++) tot += s_hist[w][tid];
            // workgroup exclusive scan of tot over the 256 digit threads
            incl = wave_inclusive_scan(tot, lane);
            if (lane == 63) s_wsum[wave] = incl;
        }
        __syncthreads();
        if (tid < 256) {
            uint32_t woff = 0;
            for (int w = 0; w < wave; w++) woff += s_wsum[w];
            uint32_t run = woff + incl - tot;
#pragma unroll
            for (int w = 0; w < NW; w++) {
                const uint32_t c = s_hist[w][tid];
                s_hist[w][tid] = run;
                run += c;
            }
        }
    }
    __syncthreads();
    // (c) stable scatter of this wave's share; s_hist[wave][digit] is now this wave's running cursor
    auto scatter = [&](uint32_t key, uint32_t val, bool active, uint32_t rk, uint32_t cnt) {
        const uint32_t digit = (key >> shift) & 0xFFu;
        uint32_t off = 0;
        if (active) off = s_hist[wave][digit] + rk;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        if (active && rk == cnt - 1) s_hist[wave][digit] = off + 1;  // last lane of the group advances the cursor
        if (active) dst.set((int)off, key, val);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    };
    if (MAXB > 0) {
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const int i0 = begin + 64 * j;
            if (i0 >= end) break;
            scatter(c_key[j], c_val[j], i0 + lane < end, c_rk[j], c_cnt[j]);
        }
    } else {
        for (int i0 = begin; i0 < end; i0 += 64) {
            const int i = i0 + lane;
            const bool active = i < end;
            const uint32_t key = active ? src.key(i) : 0u, val = active ? src.val(i) : 0u;
            uint32_t rk, cnt;
            match((key >> shift) & 0xFFu, active, rk, cnt);
            scatter(key, val, active, rk, cnt);
        }
    }
    __syncthreads();
}

// The tile's BLEND LIST: the values of the sorted entries, Gaussian id | quadrant mask << 28, four bytes per overlap at
// blend_list[range.x ...].  This is all the blend kernels get of a tile: they scan the entries 64 at a time (256
// contiguous bytes), queue the ones whose bit for their quadrant is set and gather the 32-byte geometry record index_rec[id] next to
// the feature row of the same id -- two independent gathers behind one scan.  The position of an entry
// in its list is its index -- n_contrib's unit.  Full lists (bin_ranks_kernel): every overlap of the reference's rects is an entry,
// culled ones with mask 0, so blend_list & ID_MASK IS the reference's point_list and the index its position there; lean lists
// (bin_spans_kernel): the entries that can blend only.
// The radix passes order by depth bits and keep the ARRIVAL order of equal keys, which is arbitrary; the contract orders equal depths
// by Gaussian index (the reference's stable sort of (tile | depth) keys emitted in index order, rasterizer_impl.cu:96-113, 300-308).
// Entries whose neighbour in the sorted list has the same key -- two Gaussians of one tile at bit-identical depth: rare, but not
// excluded -- find their run and take the position of their id inside it.
template <int NW, typename Src>
__device__ __forceinline__ void emit_blend_list(Src sorted, int n, uint2 range, int tid, uint32_t* __restrict__ blend_list)
{
    uint32_t* out = blend_list + range.x;
    for (int i = tid; i < n; i += NW * 64) {
        const uint32_t k = sorted.key(i), v = sorted.val(i);
        int pos = i;
        if ((i > 0 && sorted.key(i - 1) == k) || (i + 1 < n && sorted.key(i + 1) == k)) {
            int lo = i, hi = i + 1;
            while (lo > 0 && sorted.key(lo - 1) == k) lo--;
            while (hi < n && sorted.key(hi) == k) hi++;
            int before = 0;
            for (int q = lo; q < hi; q++) before += (sorted.val(q) & ID_MASK) < (v & ID_MASK) ? 1 : 0;
            pos = lo + before;
        }
        out[pos] = v;
    }
}

// MI_RAST_VERIFY_LISTS (include/mi_rast.h): the lean lists rest on the count pass and the emit pass taking bit-identical float
// decisions in two template instances of bin_spans_kernel -- a tile is counted iff the emit pass stores an entry for it.  With
// the flag the entries are zero-filled before the emit pass and this kernel counts the slots of every tile's segment that
// are still zero afterwards (a lean entry always carries a non-zero quadrant mask): any such slot is a decision that differed.
__global__ void __launch_bounds__(256) verify_entries_kernel(uint32_t ntiles, const uint2* __restrict__ ranges,
                                                              const uint2* __restrict__ entries, uint32_t* __restrict__ unwritten)
{
    const uint32_t tile = blockIdx.x;
    if (tile >= ntiles) return;
    const uint2 r = ranges[tile];
    uint32_t n = 0;
    for (uint32_t i = r.x + threadIdx.x; i < r.y; i += 256) n += entries[i].y == 0u;
    if (n) atomicAdd(unwritten, n);
}

// ---- per-tile sort of short lists: one WAVE per tile, bitonic network in registers ------------------------------------
// Lists of up to 2048 entries (every list of a 1 M-Gaussian 1080p view; most of a 5 M-Gaussian one) are ordered by ONE wave
// each, with no LDS and no barrier: lane l holds the EPL consecutive elements l EPL .. l EPL + EPL - 1 of the list padded to
// N = 64 EPL (EPL = 4 / 8 / 16 / 32 by list length), each as one 64-bit word  depth bits << 32 | id << 4 | quadrant mask  -- ids
// are distinct inside a tile, so ordering the words orders by (depth bits, id): the contract's order, ties included, with no
// second pass.
//   * The words are compared as binary64 numbers: depth bits are those of a positive finite float (sign clear, exponent field
//     below 0xFF), so the word's top twelve bits are a binary64 exponent below 0x7FF -- never NaN or infinity --, and positive
//     binary64 numbers order like their bit patterns.  v_min_f64 / v_max_f64 are a 64-bit compare-exchange in TWO instructions;
//     v_cmp_lt_u64 + four v_cndmask_b32, the integer form, measured 0.087 ms per cfg3 view.
//   * The network is the all-ascending form of the bitonic sorter: stage K first compares element i with i ^ (K - 1) (the mirror
//     image inside its block of K), then i with i ^ j for j = K / 4 .. 1; the smaller word always goes to the smaller index, so no
//     step carries a direction.  Distances below EPL stay inside a lane (register pairs); the others pair lane l with
//     l ^ M: DPP moves for M = 1, 2, 3, 4, 7, 8, 15 (quad_perm, row_half_mirror, row_mirror, row_shl / row_shr under bank masks),
//     ds_swizzle for 16 and 31, ds_bpermute for 32 and 63 -- 21 of the 45 steps of a 512-entry list cross lanes.
__device__ __forceinline__ void minmax64(double& lo, double& hi)   // (inline asm: no canonicalisation of the operands in front of it)
{
    double mn;
    asm("v_min_f64 %0, %1, %2" : "=v"(mn) : "v"(lo), "v"(hi));
    asm("v_max_f64 %0, %1, %2" : "=v"(hi) : "v"(lo), "v"(hi));   // (may overwrite an operand in place: no copies around the pair)
    lo = mn;
}

// one step of stage K: FLIP -- partner i ^ (K - 1) -- or distance J
template <int EPL, int K, int J, bool FLIP>
__device__ __forceinline__ void bitonic_step(double (&a)[EPL], int lane)
{
    if constexpr (FLIP && K > EPL) {
        // i ^ (K - 1) = (lane ^ (K / EPL - 1)) * EPL + (EPL - 1 - r): the mirrored register of the mirrored lane
        constexpr int M = K / EPL - 1;
        const bool lower = (lane & ((M + 1) >> 1)) == 0;
#pragma unroll
        for (int r = 0; r < EPL / 2; r++) {   // registers r and EPL - 1 - r trade places with the partner lane's: two temporaries at a time
            double x0 = a[r], y0 = lane_xor64<M>(a[EPL - 1 - r]);
            double x1 = a[EPL - 1 - r], y1 = lane_xor64<M>(a[r]);
            minmax64(x0, y0);
            minmax64(x1, y1);
            a[r] = lower ? x0 : y0;
            a[EPL - 1 - r] = lower ? x1 : y1;
        }
    } else if constexpr (!FLIP && J >= EPL) {
        constexpr int M = J / EPL;
        const bool lower = (lane & M) == 0;
#pragma unroll
        for (int r = 0; r < EPL; r++) {
            double x = a[r], y = lane_xor64<M>(a[r]);
            minmax64(x, y);
            a[r] = lower ? x : y;
        }
    } else {
        constexpr int X = FLIP ? K - 1 : J;   // in-lane partner r ^ X
#pragma unroll
        for (int r = 0; r < EPL; r++)
            if ((r ^ X) > r) minmax64(a[r], a[r ^ X]);
    }
}
template <int EPL, int K, int J>
__device__ __forceinline__ void bitonic_tail(double (&a)[EPL], int lane)   // distances J, J / 2, .. 1 of stage K, then the next stage
{
    if constexpr (J >= 1) {
        bitonic_step<EPL, K, J, false>(a, lane);
        bitonic_tail<EPL, K, J / 2>(a, lane);
    } else if constexpr (K < 64 * EPL) {
        bitonic_step<EPL, 2 * K, 0, true>(a, lane);
        bitonic_tail<EPL, 2 * K, K / 2>(a, lane);
    }
}

template <int EPL>
__device__ __forceinline__ void tile_sort_in_wave(const uint2* __restrict__ seg, int n, uint32_t* __restrict__ out, int lane)
{
    double a[EPL];
#pragma unroll
    for (int r = 0; r < EPL; r++) {
        const int e = r * 64 + lane;   // (any order will do going IN: coalesced loads; the sorted sequence is indexed lane * EPL + r)
        uint64_t w = 0x7FEFFFFFFFFFFFFFull;   // padding: the largest finite binary64, behind every entry
        if (e < n) {
            const uint2 p = seg[e];
            w = ((uint64_t)p.x << 32) | __builtin_rotateleft32(p.y, 4);   // id | mask << 28  ->  id << 4 | mask
        }
        a[r] = __builtin_bit_cast(double, w);
    }
    bitonic_step<EPL, 2, 0, true>(a, lane);
    bitonic_tail<EPL, 2, 0>(a, lane);
#pragma unroll
    for (int r = 0; r < EPL; r++) {
        const int e = lane * EPL + r;
        if (e < n) out[e] = __builtin_rotateright32((uint32_t)__builtin_bit_cast(uint64_t, a[r]), 4);
    }
}

constexpr int TILE_SORT_WAVE_MAX = 4096;   // longest list the wave kernels order (EPL = 64); longer ones: tile_sort_kernel
// CLASS 0: lists of 1 .. 1024 entries (EPL = 4 / 8 / 16: 52 VGPRs); 1: 1025 .. 2048 (EPL = 32); 2: 2049 .. 4096 (EPL = 64) -- the
// longer classes are launched only when a tile needs them: one kernel for all would run the short lists at the long ones' register count.
template <int CLASS>
__global__ void __launch_bounds__(256) tile_sort_wave_kernel(uint32_t ntiles, const uint2* __restrict__ ranges,
                                                              const uint2* __restrict__ entries, uint32_t* __restrict__ blend_list)
{
    const int lane = threadIdx.x & 63;
    const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    const uint2 range = ranges[tile];
    const int n = (int)(range.y - range.x);
    const uint2* seg = entries + range.x;
    uint32_t* out = blend_list + range.x;
    if constexpr (CLASS == 2) {
        if (n > 2048 && n <= 4096) tile_sort_in_wave<64>(seg, n, out, lane);
    } else if constexpr (CLASS == 1) {
        if (n > 1024 && n <= 2048) tile_sort_in_wave<32>(seg, n, out, lane);
    } else {
        if (n == 0 || n > 1024) return;
        if (n <= 256) tile_sort_in_wave<4>(seg, n, out, lane);
        else if (n <= 512) tile_sort_in_wave<8>(seg, n, out, lane);
        else tile_sort_in_wave<16>(seg, n, out, lane);
    }
}

template <int LO, int CAP, bool GLOBAL_FALLBACK, int NT>
__global__ void __launch_bounds__(NT) tile_sort_kernel(uint32_t ntiles, const uint2* __restrict__ ranges,
                                                        uint2* __restrict__ entries, uint2* __restrict__ scratch,
                                                        const int* __restrict__ key_bits, uint32_t* __restrict__ blend_list)
{
    __shared__ uint32_t s_k[2][CAP];
    __shared__ uint32_t s_v[2][CAP];
    constexpr int NW = NT / 64;
    __shared__ uint32_t s_hist[NW][256];
    const int tid = threadIdx.x;
    // (tile = workgroup id: neighbouring tiles on different XCDs.  The cost of a tile is its list length, and a static split into
    // contiguous runs per XCD -- xcd_runs.h -- would let a scene's dense half wait for two of the eight XCDs.)
    const uint32_t tile = blockIdx.x;
    if (tile >= ntiles) return;
    const uint2 range = ranges[tile];
    const int passes = (*key_bits + 7) >> 3;
    const int n = (int)(range.y - range.x);
    if (n <= LO) return;
    if (n > CAP && !GLOBAL_FALLBACK) return;
    uint2* seg = entries + range.x;
    if (n <= CAP) {
        // (lean lists too: their counts are exact -- bin_spans_kernel --, every slot of the segment holds an entry)
        for (int i = tid; i < n; i += NT) {
            const uint2 e = seg[i];
            s_k[0][i] = e.x;
            s_v[0][i] = e.y;
        }
        __syncthreads();
        int cur = 0;
        for (int p = 0; p < passes; p++, cur ^= 1)
            radix_pass<NW, (CAP + NW * 64 - 1) / (NW * 64)>(LdsPairs{s_k[cur], s_v[cur]}, LdsPairs{s_k[cur ^ 1], s_v[cur ^ 1]}, n, 8 * p, s_hist, tid);
        emit_blend_list<NW>(LdsPairs{s_k[cur], s_v[cur]}, n, range, tid, blend_list);
    } else {
        uint2* a = seg;
        uint2* b = scratch + range.x;
        for (int p = 0; p < passes; p++) {
            radix_pass<NW, 0>(GlobalPairs{a}, GlobalPairs{b}, n, 8 * p, s_hist, tid);
            uint2* t = a;
            a = b;
            b = t;
        }
        emit_blend_list<NW>(GlobalPairs{a}, n, range, tid, blend_list);
    }
}

}  // namespace mirast
