// lift.h -- 2D-to-3D score lifting: votes[g, k] += sum over the pixels p of w_g(p) scores[k, p], w = alpha T the forward's blending
// weight of Gaussian g at pixel p.  One FRONT-TO-BACK walk per tile, no image, no per-pixel state, no backward.
//
// What the reference does per view (clip_utils/__init__.py:291-330 through gaussian_renderer.render_mask): render a zero mask,
// loss = -(target * rendered).sum(), backward(), accumulate minus the gradient.  The render is linear in the mask, so that gradient
// is dL_dcolors of the blend backward (CF/cuda_rasterizer/backward.cu:487-501) with dL_dpixel = target, and needs alpha and T of
// every (Gaussian, pixel) pair and nothing else.  The backward kernels rebuild T back to front by division from the final_T and
// n_contrib a forward left; here T is the forward's own recurrence (CF/cuda_rasterizer/forward.cu:330-356), taken with the forward's
// tests in the forward's order:
//     power = gauss_power(...);                   power > 0      -> the pair is skipped
//     alpha = min(0.99, opacity exp(power));      alpha < 1/255  -> skipped
//     test_T = T (1 - alpha);                     test_T < 1e-4  -> the pixel is done, this pair is NOT blended
//     w = alpha T;  T = test_T
// exp is the device library's expf for every pair (gauss_exp<true>, as in the backward kernels; MI_RAST_FAST_EXP: gauss_exp<false>),
// so the pair set is the one a forward under MI_RAST_EXACT_EXP blends.  Neither final_T nor n_contrib is read.
//
// One wave owns NQ = 2 of a tile's four 8 x 8 quadrants (the upper or lower half tile, as blend_bwd_feat.h; NQ = 4, the whole
// tile, is slower: DESIGN.md section 20), lane l the pixel (l & 7, l >> 3) of each.  The wave scans the tile's blend list itself,
// 64 entries at a time, appends the entries whose quadrant mask names one of its quadrants to a ring in LDS and works through it
// in chunks of CHK records; the next chunk's records are requested before the current one is evaluated (the walk of
// blend_bwd_wave.h, turned round).  The reduction
// over pixels is blend_bwd_feat.h's dF = W^T dL contraction on v_mfma_f32_16x16x4_f32 with the SCORE image as the B operand, staged
// once per item; NB 16-channel blocks, of which the last may be partial: channels >= K are zero columns, and their atomics are not
// issued.  One row of atomics leaves per (item, record): a K <= 16 row is one 64-byte request (profiles/r06_bwd_atomics.md: the
// request rate is what bounds such a kernel).  The walk ends with the chunk in which the last of the wave's pixels is done.
//
// The kernel READS the tile ranges, the blend list, index_rec and the XCD run bounds and writes `votes` only: no work-queue
// counters, no walk counters, nothing in the geometry, binning or image buffer -- a lift is legal between a forward and its
// backward.  Tiles are dealt statically: workgroup 8 j + x takes item j of the run of tiles the range scan cut for XCD x.
//
// ORDER OF THE SUMS: the rows are added with float atomics, so the order in which the items' contributions to one Gaussian arrive --
// and with it the last bits of `votes` -- varies from run to run.  Inside one item the sum over its pixels has a fixed order.
#pragma once

#include <type_traits>

#include "blend_bwd_shared.h"
#include "blend_rec.h"
#include "common.h"
#include "wave.h"

namespace mirast {

constexpr int LIFT_NQ = 2;   // quadrants per wave: a tile is two items

// NB: 16-channel blocks (K <= 16 NB real channels, rows of `votes` K floats apart)
template <int NB, bool XEXP = true>
__global__ void __launch_bounds__(64, NB >= 4 ? 2 : 3) lift_kernel(
    const uint2* __restrict__ ranges, const uint32_t* __restrict__ blend_list, const BlendRec* __restrict__ index_rec, int W, int H,
    uint32_t horizontal_blocks, uint32_t ntiles, const float* __restrict__ scores /* [K, H, W] */, float* __restrict__ votes /* [P, K] */,
    int K, const uint32_t* __restrict__ run_bounds /* [9]: the XCDs' runs of tiles, left in the image buffer by the range scan */)
{
    constexpr int NQ = LIFT_NQ;
    static_assert(NQ == 2 || NQ == 4, "a wave owns a half tile or a whole tile");
    static_assert(NB == 1 || NB == 2 || NB == 4, "16, 32 or 64 channel columns");
    constexpr int QCAP = 128;
    constexpr int SROW = 17;      // score staging row (floats; 16 channels at a time)
    constexpr int IPT = 4 / NQ;   // items per tile
    static_assert(NQ * CHK * WROW >= 64 * SROW, "score staging must fit in the w rows");

    __shared__ BwdPar s_par[CHK];                  // the chunk's 16 records
    __shared__ float4 s_w4[NQ * CHK * WROW / 4];   // w rows, one block of CHK rows per quadrant   (prologue: score staging)
    __shared__ uint2 s_queue[QCAP];                // {list position, entry = Gaussian id | quadrant mask << 28}

    // workgroup -> (tile, part): id = 8 (IPT j + part) + x is part `part` of the j-th tile of XCD x's run
    const uint32_t xcd = blockIdx.x & 7u, jj = blockIdx.x >> 3;
    const uint32_t run_start = run_bounds[xcd], run_len = run_bounds[xcd + 1u] - run_start;
    if (jj / IPT >= run_len) return;
    const uint32_t tile = run_start + jj / IPT, part = jj % IPT;
    if (tile >= ntiles) return;

    const uint32_t tile_x = tile % horizontal_blocks, tile_y = tile / horizontal_blocks;
    const int lane = threadIdx.x & 63;
    const size_t HW = (size_t)H * W;
    float pixfx[NQ], pixfy[NQ];
    bool inside[NQ];
    size_t pix[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        const uint32_t quad = part * NQ + q;
        const uint32_t px = tile_x * TILE_X + (quad & 1u) * 8u + (lane & 7), py = tile_y * TILE_Y + (quad >> 1) * 8u + (lane >> 3);
        pixfx[q] = (float)px;
        pixfy[q] = (float)py;
        inside[q] = px < (uint32_t)W && py < (uint32_t)H;
        pix[q] = inside[q] ? (size_t)W * py + px : 0;
    }
    const uint2 range = ranges[tile];
    const int NS = (int)(range.y - range.x);
    const uint32_t* lst = NS > 0 ? blend_list + range.x : blend_list;
    // (scan loads are unconditional, index clamped: blend_bwd_wave.h)
    uint32_t scan_reg = lst[min(lane, max(NS - 1, 0))];

    // ---- score image: B of the contraction, scT[q][nb][s] = scores[channel 16 nb + n16][pixel 16 kq + s of quadrant q]
    const int n16 = lane & 15, kq = lane >> 4;
    float scT[NQ][NB][16];
    {
        float* stage = reinterpret_cast<float*>(s_w4);
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            float sc[16 * NB];
#pragma unroll
            for (int ch = 0; ch < 16 * NB; ch++) sc[ch] = ch < K ? scores[(size_t)ch * HW + pix[q]] : 0.f;   // (wave-uniform test)
#pragma unroll
            for (int h = 0; h < NB; h++) {
#pragma unroll
                for (int c = 0; c < 16; c++) stage[lane * SROW + c] = inside[q] ? sc[16 * h + c] : 0.f;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
                for (int s = 0; s < 16; s++) scT[q][h][s] = stage[(16 * kq + s) * SROW + n16];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            }
        }
    }
    if (NS == 0) return;

    float* const my_w = reinterpret_cast<float*>(s_w4);
    const char* const par_bytes = reinterpret_cast<const char*>(s_par);

    // ---- the queue of this item's records, front to back: entries whose mask names one of its quadrants
    int scanned = 0, qh = 0, qt = 0;
    auto consume_scan = [&]() {
        const int j = scanned + lane;
        const bool cand = j < NS && ((scan_reg >> (ID_BITS + NQ * part)) & ((1u << NQ) - 1u)) != 0;
        const uint64_t bal = ballot64(cand);
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if (cand) s_queue[(qt + (int)below) & (QCAP - 1)] = make_uint2((uint32_t)j, scan_reg);
        qt += __builtin_popcountll(bal);
        scanned += 64;
        scan_reg = lst[min(scanned + lane, NS - 1)];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    };
    // record quarter (lane & 3) of row (lane >> 2) of the next chunk (rows >= n repeat row n - 1 and become padding when staged)
    uint2 curq;
    auto request_rows = [&](int n) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        int l = threadIdx.x & 63;
        asm volatile("" : "+v"(l));
        const int rq = min(l >> 2, n - 1), qq = l & 3;
        const uint32_t gq = s_queue[(qh + rq) & (QCAP - 1)].y & ID_MASK;
        curq = reinterpret_cast<const uint2*>(index_rec + gq)[qq];
    };

    while (qt - qh < CHK && scanned < NS) consume_scan();
    int nrows = min(CHK, qt - qh);
    if (nrows == 0) return;
    request_rows(nrows);

    float T[NQ];
    bool done[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        T[q] = 1.0f;
        done[q] = !inside[q];   // forward.cu:294
    }

    int nnext = 0;
    bool live = true;   // some pixel of the wave is not done (wave-uniform)
    auto do_chunk = [&](auto full_tag) __attribute__((always_inline)) {
        constexpr bool FULL = decltype(full_tag)::value;   // all 16 rows are real
        // ---- 1. the chunk's rows: registers -> LDS as {x, y, -a/2, -b} {-c/2, opacity, -, id} (padding rows: opacity 0, never blended)
        {
            const int rq = lane >> 2, qq = lane & 3;
            float2 v = make_float2(__uint_as_float(curq.x), __uint_as_float(curq.y));
            const uint2 qe = s_queue[(qh + (FULL ? rq : min(rq, nrows - 1))) & (QCAP - 1)];
            if (qq == 1) v = make_float2(0.f, __uint_as_float(qe.y & ID_MASK));
            if (qq == 2) v = make_float2(-0.5f * v.x, -v.y);
            if (qq == 3) v = make_float2(-0.5f * v.x, v.y);
            if (!FULL) {
                if (rq >= nrows) {
                    v = make_float2(0.f, 0.f);
                    if (qq == 2) v = make_float2(-0.5f, 0.f);
                    if (qq == 3) v = make_float2(-0.5f, 0.f);
                }
            }
            const int dst = qq == 0 ? 0 : (qq == 1 ? 24 : (qq == 2 ? 8 : 16));
            *reinterpret_cast<float2*>(reinterpret_cast<char*>(&s_par[rq]) + dst) = v;
        }
        qh += nrows;
        // ---- 2. keep the queue ahead of the chunks, request the next chunk's rows
        if (scanned < NS && qt - qh <= QCAP - 64) consume_scan();
        while (qt - qh < CHK && scanned < NS) consume_scan();
        nnext = min(CHK, qt - qh);
        if (nnext > 0) request_rows(nnext);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");

        // ---- 3. alpha, T and w = alpha T of every pixel, front to back (forward.cu:330-356).  A row that does not blend into a pixel: w = 0.
        bool any_open = false;
#pragma unroll
        for (int r = 0; r < CHK; r++) {
            const float4 p0 = *reinterpret_cast<const float4*>(par_bytes + r * (int)sizeof(BwdPar));
            const float4 p1 = *reinterpret_cast<const float4*>(par_bytes + r * (int)sizeof(BwdPar) + 16);
#pragma unroll
            for (int q = 0; q < NQ; q++) {
                const float dx = p0.x - pixfx[q], dy = p0.y - pixfy[q];
                const float power = gauss_power(p0.z, p0.w, p1.x, dx, dy);
                const float t = p1.y * gauss_exp<XEXP>(power);
                const float alpha = fminf(0.99f, t);
                const bool ok = !done[q] && power <= 0.0f && t >= ALPHA_CUT;
                const float test_T = T[q] * (1 - alpha);
                const bool stop = ok && test_T < 0.0001f;
                done[q] = done[q] || stop;
                const bool blend = ok && !stop;
                my_w[(q * CHK + r) * WROW + lane] = blend ? alpha * T[q] : 0.f;
                T[q] = blend ? test_T : T[q];
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; q++) any_open = any_open || !done[q];
        live = ballot64(any_open) != 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");

        // ---- 4. rows = sum over the quadrants of W_q^T . scores_q   (A rows from LDS, lane (m = n16, kq) reads pixels 16 kq .. 16 kq + 15)
        v4f facc[NB];
#pragma unroll
        for (int nb = 0; nb < NB; nb++) facc[nb] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const float4* wr = reinterpret_cast<const float4*>(my_w + (q * CHK + n16) * WROW + 16 * kq);
#pragma unroll
            for (int s4 = 0; s4 < 4; s4++) {
                const float4 wv = wr[s4];
                const float w[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
                for (int t = 0; t < 4; t++)
#pragma unroll
                    for (int nb = 0; nb < NB; nb++)
                        facc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t], scT[q][nb][4 * s4 + t], facc[nb], 0, 0, 0);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the operand reads of the w rows are done: the next chunk may write them
        // ---- 5. one row of atomics per (item, record): lane l holds channel n16 of rows 4 kq + r
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = 4 * kq + r;
            const uint32_t gid = __float_as_uint(*reinterpret_cast<const float*>(par_bytes + row * (int)sizeof(BwdPar) + 28));
#pragma unroll
            for (int nb = 0; nb < NB; nb++) {
                if (16 * nb + n16 >= K || (!FULL && row >= nrows)) continue;
                atomicAdd(&votes[(size_t)gid * K + 16 * nb + n16], facc[nb][r]);
            }
        }
    };
    if (nrows == CHK) {
        do_chunk(std::true_type{});
        while (nnext == CHK && live) {
            nrows = nnext;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            do_chunk(std::true_type{});
        }
        nrows = nnext;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
    if (nrows != 0 && live) do_chunk(std::false_type{});
}

}  // namespace mirast
