// common.h -- shared device helpers for the gfx950 rasterizer kernels.
//
// Numeric contract: the per-Gaussian geometry path that feeds the INTEGER results
// (radii, tile rects, tiles_touched, depth key bits) is IEEE binary32 in the reference's source
// order with NO fused contraction: this translation unit is compiled with -ffp-contract=off and
// uses fmaf() only inside the blend kernels' accumulators, which are float-path (tolerance)
// quantities.  Division and sqrt are correctly rounded (hipcc default
// -fhip-fp32-correctly-rounded-divide-sqrt).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mirast {

constexpr int R_SLOTS = 64;        // partial sums of R, one per 128-byte line
constexpr int R_SLOT_STRIDE = 32;  // ints: [0] R, [1] max of ~depth key, [2] max depth key, [R_SLOT_BANDS + b] Gaussians touching band b
constexpr int R_SLOT_BANDS = 4;
constexpr int MAX_BANDS = 24;      // bands of tile rows of the lean count / emit passes (bin_lean.h); one bit per band in band_mask
// Row stride of the count passes' difference grids in LDS (bin_full.h, bin_lean.h): odd, so that column walks spread over the banks
__host__ __device__ inline int count_grid_stride(uint32_t gx) { return (int)((gx + 1) | 1u); }


constexpr int TILE_X = 16;  // CF/cuda_rasterizer/config_contrastive_f.h:16 -- part of the integer contract
constexpr int TILE_Y = 16;  // CF/cuda_rasterizer/config_contrastive_f.h:17
constexpr int TILE_PIXELS = TILE_X * TILE_Y;
constexpr int BATCH = 256;  // threads per tile workgroup (blend_fwd.h, blend_fwd_x3.h, blend_bwd.h)
constexpr int WAVE = 64;

struct Mat3 {  // glm layout m[col][row]
    float m[3][3];
};

// glm::mat3 * glm::mat3 (CF/third_party/glm/glm/detail/type_mat3x3.inl:486-520): three products
// summed left to right.
__device__ __forceinline__ Mat3 m3mul(const Mat3& A, const Mat3& B)
{
    Mat3 R;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int r = 0; r < 3; r++)
            R.m[c][r] = A.m[0][r] * B.m[c][0] + A.m[1][r] * B.m[c][1] + A.m[2][r] * B.m[c][2];
    return R;
}
__device__ __forceinline__ Mat3 m3transpose(const Mat3& A)
{
    Mat3 R;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int r = 0; r < 3; r++) R.m[c][r] = A.m[r][c];
    return R;
}

// float -> int32: v_cvt_i32_f32 saturates and maps NaN to 0, the same as nvcc's cvt.rzi.s32.f32.
__device__ __forceinline__ int f2i(float f) { return (int)f; }

// CF/cuda_rasterizer/auxiliary.h:41-44 -- double literals: evaluated in binary64, rounded once.
__device__ __forceinline__ float ndc2Pix(float v, int S) { return (float)(((v + 1.0) * S - 1.0) * 0.5); }

// CF/cuda_rasterizer/auxiliary.h:46-56
__device__ __forceinline__ void getRect(float px, float py, int max_radius, uint2& rect_min, uint2& rect_max,
                                        uint32_t gx, uint32_t gy)
{
    rect_min.x = min(gx, (uint32_t)max(0, f2i((px - (float)max_radius) / (float)TILE_X)));
    rect_min.y = min(gy, (uint32_t)max(0, f2i((py - (float)max_radius) / (float)TILE_Y)));
    rect_max.x = min(gx, (uint32_t)max(0, f2i((px + (float)max_radius + (float)TILE_X - (float)1) / (float)TILE_X)));
    rect_max.y = min(gy, (uint32_t)max(0, f2i((py + (float)max_radius + (float)TILE_Y - (float)1) / (float)TILE_Y)));
}

// CF/cuda_rasterizer/auxiliary.h:58-77
__device__ __forceinline__ float3 transformPoint4x3(const float3& p, const float* m)
{
    return make_float3(m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12],
                       m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
                       m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14]);
}
__device__ __forceinline__ float4 transformPoint4x4(const float3& p, const float* m)
{
    return make_float4(m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12],
                       m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
                       m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14],
                       m[3] * p.x + m[7] * p.y + m[11] * p.z + m[15]);
}
// CF/cuda_rasterizer/auxiliary.h:89-97
__device__ __forceinline__ float3 transformVec4x3Transpose(const float3& p, const float* m)
{
    return make_float3(m[0] * p.x + m[1] * p.y + m[2] * p.z,
                       m[4] * p.x + m[5] * p.y + m[6] * p.z,
                       m[8] * p.x + m[9] * p.y + m[10] * p.z);
}
// CF/cuda_rasterizer/auxiliary.h:107-117
__device__ __forceinline__ float3 dnormvdv(float3 v, float3 dv)
{
    float sum2 = v.x * v.x + v.y * v.y + v.z * v.z;
    float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
    float3 r;
    r.x = ((+sum2 - v.x * v.x) * dv.x - v.y * v.x * dv.y - v.z * v.x * dv.z) * invsum32;
    r.y = (-v.x * v.y * dv.x + (sum2 - v.y * v.y) * dv.y - v.z * v.y * dv.z) * invsum32;
    r.z = (-v.x * v.z * dv.x - v.y * v.z * dv.y + (sum2 - v.z * v.z) * dv.z) * invsum32;
    return r;
}

// Per-view constants every kernel needs, passed by value (kernarg -> SGPRs).  The 4x4 matrices and the
// camera position stay in device memory exactly as the reference passes them; every thread reads them
// at wave-uniform addresses, which gfx950 serves with scalar loads (s_load_dwordx16) from the scalar
// cache -- no host round trip.
struct ViewParams {
    const float* view;    // [16] world->view, column-major for the kernels (scene/cameras.py:62)
    const float* proj;    // [16] full projection
    const float* campos;  // [3] or nullptr
    float tan_fovx, tan_fovy, focal_x, focal_y, scale_modifier;
    int W, H;
    uint32_t grid_x, grid_y;
};

// Exponent of a Gaussian at offset (dx, dy) from its mean, conic pre-scaled to (ha, nb, hc) = (-a/2, -b, -c/2):
// ((-a/2 dx) dx + (-c/2 dy) dy) + (-b dx) dy -- bit-identical to the reference expression -0.5f (a dx dx + c dy dy) - b dx dy
// (forward.cu:338, backward.cu:497; scaling by -1/2 and -1 commutes with every rounding), two VALU fewer.  ONE definition for
// every blend kernel: the forward's alpha >= 1/255 decisions are re-taken by the backward, so both must round this value
// identically.  Deliberately NOT fused: the fmaf form (two instructions fewer) was measured and bought nothing, while its
// 1-ulp differences against an unfused reference flip pairs at the 1/255 threshold -- at full cfg3 size the norm-wise error of
// dL_dmeans2D against the oracle went from 5.6e-7 to 5.8e-6 and the rows outside tolerance from 2.2e-4 to 1.2e-3.
__device__ __forceinline__ float gauss_power(float ha, float nb, float hc, float dx, float dy)
{
    return (ha * dx * dx + hc * dy * dy) + nb * dx * dy;
}

// exp() of the Gaussian exponent: ONE definition for every blend kernel (see gauss_power).  XEXP = true (product default): the
// device library's expf (<= 1 ulp, 13 VALU instructions; 10 as restated below) -- the function the reference's kernels call.  XEXP = false
// (MI_RAST_FAST_EXP): v_exp_f32(power * log2e), 2 instructions, ~5 ulp (the rounding of the product dominates).  The difference
// only matters at the alpha >= 1/255 cut: measured at full cfg3 size, with the 5-ulp exp the rows of dL_dmeans2D outside
// tolerance against the fp64 oracle are 2.2e-4 against the reference's own 1.9e-5, and ALL of that excess comes from pairs put
// on the other side of the cut; with expf the product's statistics are the reference's and n_contrib equals the reference's on
// every pixel.  Cost: +0.03 ms in the forward blend (ALU-bound), nothing measurable in the backward (atomic-bound): 2 % of a
// cfg3 step.
//
// The expf form is the device library's algorithm (ocml expf, f32 with denormals, as hipcc compiles it for gfx950) restated
// with ONE clamp in place of its two range selects (0 below -103.28, inf above 88.72; two v_cmp + two v_cndmask):
// exp(x) = ldexp(exp2((ph - e) + pl), e) with ph + pl = x log2(e) in two-term precision and e = rint(ph), on max(x, -104).
// For every f32 x in [-103.28, 0] the result is bit-identical to expf(x); below that, where expf gives exactly 0, it is 0 or
// the smallest denormal (tools/expf_check.hip runs all 2^32 inputs; tests/test_gpu_parity.py::test_lean_expf_is_the_device_
// expf).  The clamp is needed: without it a hugely negative exponent (a degenerate conic) with a positive rounding residual
// pl ends in ldexp(inf, INT_MIN) = inf.  Where the two differ the blend kernels do not use the value: power > 0 and NaN are
// rejected by their own `power <= 0` test (forward.cu:339), and opacity times a denormal fails the >= 1/255 test like
// opacity times 0.
//
// HYBRID evaluation (the forward blend's product default, blend_fwd_wave.h; include/mi_rast.h: MI_RAST_EXACT_EXP switches it off):
// opacity * exp(power) only has to be the device expf's value BIT FOR BIT where it decides something -- at the alpha >= 1/255
// cut, which the backward re-takes with expf.  Away from the cut a few ulp are float-path noise (alpha to ~6e-7 relative).  So:
// G = v_exp_f32(power * log2e) (2 VALU; relative error <= 8 * 2^-24 * ln 2 + 1 ulp < 1e-6 wherever opacity * G can reach 1/255,
// i.e. power >= -5.55), two compares against the cut widened by +-4e-6 relative, and a GROUP of 16 entries (32/64-channel kernel;
// one entry in the RGB kernel) in which ANY lane falls between the two bounds is re-evaluated with the exact form (a wave-uniform
// branch, taken for ~1e-3 of the groups).  A value outside the band lies on the same side of the cut in both forms, so every
// alpha >= 1/255 decision is the one expf takes: the forward and the backward agree on who blends, always.  ONLY that decision is
// protected: the T < 1e-4 stop test runs on the v_exp_f32 alphas, so where a pixel stops (n_contrib, final_T) can differ from an
// all-expf run -- on ~1e-6 of the pixels of the benchmark scenes, on up to 7.9e-5 of the pixels of an opaque scene of faint
// Gaussians (many pixels ending right at the threshold; the worst case of tools/fuzz_parity.py's sweeps).  A band around the stop
// test, like the one around the cut, would not help: what differs is T, the product of all earlier (1 - alpha), and re-evaluating
// the current group with expf does not restore it.  The default mode is not bit-identical to the reference on the image-state
// fields (MI_RAST_EXACT_EXP is, and that is the mode their parity is checked in).
constexpr float ALPHA_CUT = 1.0f / 255.0f;
constexpr float ALPHA_CUT_LO = (float)((1.0 / 255.0) * (1.0 - 4e-6));
constexpr float ALPHA_CUT_HI = (float)((1.0 / 255.0) * (1.0 + 4e-6));
enum ExpMode : int { EXP_FAST = 0, EXP_EXACT = 1, EXP_HYBRID = 2 };
__device__ __forceinline__ float gauss_exp_fast(float power) { return __builtin_amdgcn_exp2f(power * 0x1.715476p+0f); }

template <bool XEXP>
__device__ __forceinline__ float gauss_exp(float power)
{
    if constexpr (XEXP) {
        const float x = __builtin_fmaxf(power, -104.0f);
        const float ph = x * 0x1.715476p+0f;
        float pl = __builtin_fmaf(x, 0x1.715476p+0f, -ph);
        pl = __builtin_fmaf(x, 0x1.4ae0bep-26f, pl);
        const float e = __builtin_rintf(ph);
        return __builtin_amdgcn_ldexpf(__builtin_amdgcn_exp2f((ph - e) + pl), (int)e);
    } else {
        return __expf(power);
    }
}

}  // namespace mirast
