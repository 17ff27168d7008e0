// wave.h -- wave64 primitives of the gfx950 kernels: ballot, butterfly sums, inclusive scans (ds_bpermute and DPP forms), the owner
// search of a wave-balanced walk, lane exchanges.  Depends on the HIP runtime alone.  tools/wave_prims_probe.hip checks the scans,
// wave_owner and lane_xor against serial code on the GPU (tests/test_wave_prims.py).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mirast {

__device__ __forceinline__ uint64_t ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v)
{
    return __builtin_bit_cast(
        float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}

// Sum over the 64 lanes of a wave; the result is valid in EVERY lane.
// quad_perm xor1 / xor2, row_half_mirror, row_mirror stay inside a 16-lane DPP row (VALU, no LDS);
// the two cross-row steps use ds_swizzle-free __shfl_xor (ds_bpermute).
__device__ __forceinline__ float wave_sum(float v)
{
    v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dpp_mov<0x141>(v);  // row_half_mirror
    v += dpp_mov<0x140>(v);  // row_mirror
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// Every other type __shfl_xor takes (double, uint32_t): the plain butterfly, six ds_bpermute steps, lanes 32 / 16 / .. / 1 apart; valid
// in EVERY lane.
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Inclusive prefix sum over the lanes: six trips through the LDS crossbar (__shfl_up is ds_bpermute).
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// The same scan on the VALU alone (seven DPP moves: row_shr 1 / 2 / 3, row_shr 4 and 8 under bank masks, row_bcast 15 and 31
// under row masks -- the sequence of AMD's GCN3 cross-lane note) instead of six trips through the LDS crossbar (__shfl_up is
// ds_bpermute): for the count / emit passes, whose waves run two scans per window.  MAX: running maximum instead of sum.
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ uint32_t dpp_or_zero(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, BANK_MASK, false);   // lanes without a source / masked off: 0
}
template <bool MAX = false>
__device__ __forceinline__ uint32_t wave_inclusive_scan_dpp(uint32_t v0)
{
    auto op = [](uint32_t a, uint32_t b) { return MAX ? max(a, b) : a + b; };
    uint32_t v = op(v0, dpp_or_zero<0x111, 0xF, 0xF>(v0));   // row_shr:1
    v = op(v, dpp_or_zero<0x112, 0xF, 0xF>(v0));             // row_shr:2
    v = op(v, dpp_or_zero<0x113, 0xF, 0xF>(v0));             // row_shr:3  -> windows of four
    v = op(v, dpp_or_zero<0x114, 0xF, 0xE>(v));              // row_shr:4, lanes 4 .. 15 of a row -> windows of eight
    v = op(v, dpp_or_zero<0x118, 0xF, 0xC>(v));              // row_shr:8, lanes 8 .. 15 -> the row's prefix
    v = op(v, dpp_or_zero<0x142, 0xA, 0xF>(v));              // row_bcast:15 into rows 1 and 3
    v = op(v, dpp_or_zero<0x143, 0xC, 0xF>(v));              // row_bcast:31 into rows 2 and 3
    return v;
}

// Hand-off point between the lanes of ONE wave through LDS: LDS operations of a wave execute in program order, so no wait is needed --
// but the compiler must neither move LDS accesses across this point nor forward a lane's own store to its later load (another
// lane may have stored there in between): a full fence at wavefront scope (no instruction) plus a scheduling barrier.
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Owner of item k = base + lane of a balanced walk: the lane o with excl[o] <= k < incl[o] (excl / incl: the lanes' exclusive /
// inclusive prefix of item counts; k < total).  The lane that owns position `base` is found by a ballot; every lane whose items
// START inside the window (base, base + 64) leaves its number at the start position in a wave-private LDS word, and a running
// maximum over the positions (lane numbers ascend with the prefix) spreads it to the positions behind: one LDS round trip and a
// DPP scan instead of a six-step binary search through LDS.
__device__ __forceinline__ uint32_t wave_owner(uint32_t* scratch /* [64] wave-private */, uint32_t excl, uint32_t incl, uint32_t base, int lane)
{
    const uint64_t first = ballot64(excl <= base && base < incl);
    const uint32_t owner0 = (uint32_t)__builtin_ctzll(first | (1ull << 63));
    // Lanes exchange words through LDS here: FULL fences (acquire + release, wavefront scope).  With release fences alone the
    // compiler forwards a lane's own `scratch[lane] = 0` to its own load of scratch[lane] -- another lane's store to that word is a
    // data race it may assume away -- and the owners come out wrong (round 6: a memory fault in the emit pass; tools/
    // wave_prims_probe.hip checks this function against a serial search on the GPU).
    scratch[lane] = 0u;
    wave_lds_fence();
    if (incl > excl && excl > base && excl - base < 64u) scratch[excl - base] = (uint32_t)lane;
    wave_lds_fence();
    const uint32_t here = scratch[lane];
    wave_lds_fence();
    return max(wave_inclusive_scan_dpp<true>(here), owner0);
}

// Value of lane l ^ M: DPP moves for M = 1, 2, 3, 4, 7, 8, 15, ds_swizzle for 16 and 31, ds_bpermute for the rest (the lane-crossing
// steps of the bitonic sorter, tile_sort.h).
template <int M>
__device__ __forceinline__ uint32_t lane_xor(uint32_t v)
{
    // (full row / bank masks, every lane has a source: v_mov_b32_dpp without an `old` operand -- update_dpp(0, ...) costs a
    // v_mov_b32 0 in front of every move)
    if constexpr (M == 1) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);         // quad_perm [1,0,3,2]
    else if constexpr (M == 2) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
    else if constexpr (M == 3) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x1B, 0xF, 0xF, true);    // quad_perm [3,2,1,0]
    else if constexpr (M == 7) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xF, 0xF, true);   // row_half_mirror
    else if constexpr (M == 15) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x140, 0xF, 0xF, true);  // row_mirror
    else if constexpr (M == 4) {   // lanes 0-3 / 8-11 of a row take lane + 4 (row_shl), the others lane - 4 (row_shr)
        const uint32_t t = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x104, 0xF, 0x5, false);
        return (uint32_t)__builtin_amdgcn_update_dpp((int)t, (int)v, 0x114, 0xF, 0xA, false);
    } else if constexpr (M == 8) {
        const uint32_t t = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x108, 0xF, 0x3, false);
        return (uint32_t)__builtin_amdgcn_update_dpp((int)t, (int)v, 0x118, 0xF, 0xC, false);
    } else if constexpr (M == 16 || M == 31) return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (M << 10) | 0x1F);   // bit mode: lane ^ M inside 32 lanes
    else return (uint32_t)__shfl_xor((int)v, M, 64);   // 32, 63
}
template <int M>
__device__ __forceinline__ double lane_xor64(double v)
{
    const uint64_t w = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = lane_xor<M>((uint32_t)w), hi = lane_xor<M>((uint32_t)(w >> 32));
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

}  // namespace mirast
