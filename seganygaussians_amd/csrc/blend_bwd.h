// blend_bwd.h -- the mask-only tile backward: dL_dmask of the mask-only render pair (mi_rast_mask_backward).
//
// Restates the backward of DEPTH/cuda_rasterizer/backward.cu:568-660: one workgroup per tile, one wave per quadrant, walking the
// tile's blend list back to front in batches of ROWS records.  Every other gradient -- colours, the six geometric fields, the DEPTH
// variant's mask gradient beside them -- is the wave-per-quadrant kernel's (blend_bwd_wave.h); this file computes none of them.
//
// What is different from the reference, by design (float path, tolerance-checked):
//  * The reference issues one float atomicAdd per contributing pixel-Gaussian pair.  Here the gradient is reduced three times before
//    it reaches HBM:
//      1. over the 64 pixels of a wave: w * dL_dout_mask is quad-reduced with DPP and its 16 partials parked in LDS for up to SLOTS
//         contributing Gaussians; lanes 0..3 finish the sums;
//      2. over the 4 waves of the tile: LDS float atomics into the batch's per-record accumulator rows;
//      3. one flush per batch: touched rows go to HBM as one atomic per (tile, Gaussian) into field 6 of the packed per-Gaussian
//         record {mean2D.xy, conic.xyw, opacity, mask, pad} (unpack_mask_kernel reads it).
//  * The tile only walks entries below max_pixel(n_contrib) (the reference walks from the end of the range and skips), each wave only
//    those below ITS quadrant's maximum, and entries are culled per quadrant exactly as in the forward (cull.h).
#pragma once

#include "blend_rec.h"
#include "common.h"
#include "wave.h"

namespace mirast {

constexpr int SLOTS = 4;     // contributing Gaussians parked per wave before a flush
constexpr int NFIELD = 8;    // packed record: mean2D.x, mean2D.y, conic.x, conic.y, conic.w, opacity, mask, pad
constexpr int ROWS = 128;    // blend-list records (+ their gradient accumulators) resident in LDS at a time

template <bool XEXP>
__global__ void __launch_bounds__(256) mask_bwd_kernel(
    const uint2* __restrict__ ranges, const uint32_t* __restrict__ blend_list, const BlendRec* __restrict__ index_rec,
    const uint32_t* __restrict__ tile_nsurv, int W, int H, const float* __restrict__ final_Ts, const uint32_t* __restrict__ n_contrib,
    const float* __restrict__ dL_dout_mask, float* __restrict__ gpack /*[P,8] packed field gradients*/)
{
    constexpr int MASK_FIELD = 6;
    __shared__ uint32_t s_id[ROWS];
    __shared__ float2 s_xy[ROWS];
    __shared__ float4 s_co[ROWS];
    __shared__ uint32_t s_pm[ROWS];
    __shared__ float4 s_gfld4[ROWS * NFIELD / 4];  // per-entry packed field gradients
    __shared__ uint32_t s_touched[ROWS];
    __shared__ float4 s_f4[4 * SLOTS * NFIELD * 16 / 4];  // quad-partials of the fields
    __shared__ int s_slot_row[4 * SLOTS];
    __shared__ int s_maxc;
    float* s_gfld = reinterpret_cast<float*>(s_gfld4);
    float* s_f = reinterpret_cast<float*>(s_f4);

    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const uint32_t horizontal_blocks = (W + TILE_X - 1) / TILE_X;
    const uint32_t tile = blockIdx.y * horizontal_blocks + blockIdx.x;
    const uint32_t qx0 = blockIdx.x * TILE_X + (wave & 1) * 8, qy0 = blockIdx.y * TILE_Y + (wave >> 1) * 8;
    const uint32_t px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
    const uint32_t pix_id = W * py + px;
    const float pixfx = (float)px, pixfy = (float)py;
    const bool inside = px < (uint32_t)W && py < (uint32_t)H;

    const uint2 range = ranges[tile];
    const int last_contributor = inside ? (int)n_contrib[pix_id] : 0;

    // entries this wave / this tile has to visit: max over pixels of n_contrib
    if (tid == 0) s_maxc = 0;
    __syncthreads();
    int wave_Lt = last_contributor;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) wave_Lt = max(wave_Lt, __shfl_xor(wave_Lt, o, 64));
    if (lane == 0) atomicMax(&s_maxc, wave_Lt);
    __syncthreads();
    const int Lt = s_maxc;
    if (Lt == 0) return;
    // blend-list records the forward walked for this tile: a superset of every contributing entry
    const int NS = (int)tile_nsurv[tile];
    const uint32_t* lst = blend_list + range.x;   // four-byte entries; list_record (blend_rec.h) gathers the geometry record of one

    float T = inside ? final_Ts[pix_id] : 0;
    // (clamped address + select: no branch)
    const float dLm = dL_dout_mask[inside ? pix_id : 0];
    const float dL_dout_mask_i = inside ? dLm : 0.f;

    int nslots = 0;  // wave-uniform
    float* my_f = s_f + wave * SLOTS * NFIELD * 16;
    int* my_slot_row = s_slot_row + wave * SLOTS;

    // Finish the per-wave reductions of the parked Gaussians and add them to the tile's LDS accumulators.
    auto flush = [&]() {
        // LDS rows written by this wave's own lanes: wave-local, no workgroup barrier needed
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        const int n = __builtin_amdgcn_readfirstlane(nslots);
        if (lane < 4) {   // one quad at work: lane l sums partials [4 l, 4 l + 4)
#pragma unroll
            for (int s = 0; s < SLOTS; s++) {
                if (s < n) {
                    const float4 v = reinterpret_cast<const float4*>(my_f + (s * NFIELD + MASK_FIELD) * 16)[lane & 3];
                    float sum = (v.x + v.y) + (v.z + v.w);
                    sum += dpp_mov<0xB1>(sum);  // quad_perm [1,0,3,2]
                    sum += dpp_mov<0x4E>(sum);  // quad_perm [2,3,0,1]
                    if ((lane & 3) == 0) atomicAdd(&s_gfld[my_slot_row[s] * NFIELD + MASK_FIELD], sum);
                }
            }
        }
        if (lane < n) s_touched[my_slot_row[lane]] = 1u;
        nslots = 0;
    };
    // quad-reduce a per-pixel value and park the 16 partials of field `fi` of the current slot
    auto park = [&](int fi, float v) {
        v += dpp_mov<0xB1>(v);
        v += dpp_mov<0x4E>(v);
        const int n = __builtin_amdgcn_readfirstlane(nslots);
        if ((lane & 3) == 0) my_f[(n * NFIELD + fi) * 16 + (lane >> 2)] = v;
    };

    BlendRec cur;
    if (tid < ROWS && tid < NS) cur = list_record(lst, index_rec, NS - 1 - tid);

    for (int b0 = 0; b0 < NS; b0 += ROWS) {
        const int nr = min(ROWS, NS - b0);  // records in this batch, walked back to front
        __syncthreads();                    // previous batch's flush to HBM done: LDS may be reused
        // ---- A: this batch's records -> LDS; the next batch's record -> registers (in flight during B and C)
        if (tid < nr) {
            s_xy[tid] = cur.xy;
            s_co[tid] = cur.co;
            s_id[tid] = cur.id;
            s_pm[tid] = cur.pm;
            s_touched[tid] = 0u;
        }
        if (tid < ROWS && b0 + ROWS + tid < NS) cur = list_record(lst, index_rec, NS - 1 - (b0 + ROWS + tid));
        // ---- B: clear the tile accumulators
        for (int q = tid; q < nr * NFIELD; q += BATCH) s_gfld[q] = 0.f;
        __syncthreads();

        // ---- C: gradients of this batch
        {
            float2 nxy = s_xy[0];
            float4 nco = s_co[0];
            uint32_t npm = s_pm[0];
            for (int r = 0; r < nr; r++) {
                const float2 cxy = nxy;
                const float4 cco = nco;
                const uint32_t pm = __builtin_amdgcn_readfirstlane(npm);
                const int rn = r + 1 < nr ? r + 1 : r;
                nxy = s_xy[rn];
                nco = s_co[rn];
                npm = s_pm[rn];
                const int pos = (int)(pm >> 4);  // 0-based forward position in the tile list
                if (!((pm >> wave) & 1u) || pos >= wave_Lt) continue;
                const float dx = cxy.x - pixfx, dy = cxy.y - pixfy;
                const float power = gauss_power(-0.5f * cco.x, -cco.y, -0.5f * cco.z, dx, dy);
                const float G = gauss_exp<XEXP>(power);
                const float t = cco.w * G;
                const float alpha = fminf(0.99f, t);
                // the forward's test, on t (min(0.99, t) >= 1/255 <=> t >= 1/255; false for a NaN t like there)
                const bool valid = (pos < last_contributor) && power <= 0.0f && t >= (1.0f / 255.0f);
                if (ballot64(valid) == 0) continue;

                const float one_m_alpha_inv = __builtin_amdgcn_rcpf(1.f - alpha);
                T = valid ? T * one_m_alpha_inv : T;
                const float w = valid ? alpha * T : 0.f;  // dmask_out / dmask of this Gaussian
                park(MASK_FIELD, w * dL_dout_mask_i);
                if (lane == 0) my_slot_row[__builtin_amdgcn_readfirstlane(nslots)] = r;
                nslots++;
                if (nslots == SLOTS) flush();
            }
            flush();
        }
        __syncthreads();

        // ---- D: one HBM atomic per touched (tile, Gaussian) into the packed record
        {
            const int rr = tid / NFIELD, f = tid % NFIELD;
            for (int r = rr; r < nr; r += BATCH / NFIELD)
                if (s_touched[r] && f == MASK_FIELD) atomicAdd(&gpack[(size_t)s_id[r] * NFIELD + f], s_gfld[r * NFIELD + f]);
        }
    }
}

}  // namespace mirast
