// mi_knn_smooth.hip -- C-ABI implementation of include/mi_knn_smooth.h (fused KNN feature smoothing).
#include "host.h"
#include "../../include/mi_knn_smooth.h"

#include "knn_smooth.h"

using namespace mirast;

extern "C" {

// ---- fused KNN feature smoothing (mi_knn_smooth.h, knn_smooth.h) ------------------------------------------
int mi_knn_smooth_forward(int P, int C, int K, const int* knn_idx, uint32_t sel_mask, const float* features, float* out,
                          int normalize_out, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || K < 1 || K > 32 || (C != 32 && C != 64)) return fail(MI_RAST_ERR_INVALID, "knn_smooth: need C in {32, 64} and 1 <= K <= 32");
    const uint32_t mask = K == 32 ? sel_mask : (sel_mask & ((1u << K) - 1u));
    const int k = __builtin_popcount(mask);
    if (k < 1) return fail(MI_RAST_ERR_INVALID, "knn_smooth: no neighbour column selected");
    if (P == 0) return MI_RAST_OK;
    const long long threads = (long long)P * (C / 4);
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (C == 32)
        hipLaunchKernelGGL(knn_smooth_fwd_kernel<32>, grid, dim3(256), 0, stream, P, K, knn_idx, mask, 1.0f / (float)k, features, out, normalize_out);
    else
        hipLaunchKernelGGL(knn_smooth_fwd_kernel<64>, grid, dim3(256), 0, stream, P, K, knn_idx, mask, 1.0f / (float)k, features, out, normalize_out);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_knn_smooth_backward(int P, int C, int K, const int* knn_idx, const int* inv_offsets, const uint32_t* inv_entries,
                           uint32_t sel_mask, const float* features, const float* dL_dout, float* dmean,
                           float* dL_dfeatures, int normalize_out, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || K < 1 || K > 32 || (C != 32 && C != 64)) return fail(MI_RAST_ERR_INVALID, "knn_smooth: need C in {32, 64} and 1 <= K <= 32");
    if (P >= (1 << 27)) return fail(MI_RAST_ERR_INVALID, "knn_smooth: more than 2^27 Gaussians");
    const uint32_t mask = K == 32 ? sel_mask : (sel_mask & ((1u << K) - 1u));
    const int k = __builtin_popcount(mask);
    if (k < 1) return fail(MI_RAST_ERR_INVALID, "knn_smooth: no neighbour column selected");
    if (P == 0) return MI_RAST_OK;
    const long long threads = (long long)P * (C / 4);
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (C == 32) {
        hipLaunchKernelGGL(knn_smooth_bwd_mean_kernel<32>, grid, dim3(256), 0, stream, P, K, knn_idx, mask, 1.0f / (float)k, features, dL_dout, dmean, normalize_out);
        hipLaunchKernelGGL(knn_smooth_bwd_feat_kernel<32>, grid, dim3(256), 0, stream, P, inv_offsets, inv_entries, mask, features, dmean, dL_dfeatures);
    } else {
        hipLaunchKernelGGL(knn_smooth_bwd_mean_kernel<64>, grid, dim3(256), 0, stream, P, K, knn_idx, mask, 1.0f / (float)k, features, dL_dout, dmean, normalize_out);
        hipLaunchKernelGGL(knn_smooth_bwd_feat_kernel<64>, grid, dim3(256), 0, stream, P, inv_offsets, inv_entries, mask, features, dmean, dL_dfeatures);
    }
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

// ---- multi-resolution smoothing (mi_knn_smooth.h, knn_smooth.h) ---------------------------------------------------------

// 0 and the levels by value, or the refusal's code; no HIP call
static int smooth_levels(int P, int C, int L, const int* level_k, SmoothLevels* lv)
{
    if (P < 0 || (C != 32 && C != 64) || L < 1 || L > KNN_SMOOTH_MAX_LEVELS || !level_k)
        return fail(MI_RAST_ERR_INVALID, "knn_smooth: need C in {32, 64} and 1 <= L <= 4 levels");
    if (P >= (1 << 27)) return fail(MI_RAST_ERR_INVALID, "knn_smooth: more than 2^27 Gaussians");
    int ktot = 0;
    for (int l = 0; l < L; l++) {
        if (level_k[l] < 1 || level_k[l] > 32) return fail(MI_RAST_ERR_INVALID, "knn_smooth: need 1 <= k <= 32 in every level");
        ktot += level_k[l];
        lv->end[l] = ktot;
        lv->inv_k[l] = 1.0f / (float)level_k[l];
    }
    if (ktot > 32) return fail(MI_RAST_ERR_INVALID, "knn_smooth: need sum of level k <= 32");
    for (int l = L; l < KNN_SMOOTH_MAX_LEVELS; l++) {
        lv->end[l] = ktot;
        lv->inv_k[l] = 0.f;
    }
    lv->L = L;
    return MI_RAST_OK;
}

int mi_knn_smooth_multi_forward(int P, int C, int L, const int* level_k, const int* knn_idx, const float* weights,
                                int weights_broadcast, const float* features, float* out, int normalize_out, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    SmoothLevels lv;
    if (const int rc = smooth_levels(P, C, L, level_k, &lv)) return rc;
    if (P == 0) return MI_RAST_OK;
    if (!knn_idx || !features || !out) return fail(MI_RAST_ERR_INVALID, "knn_smooth: need a neighbour map, features and an output");
    const int ktot = lv.end[L - 1], w_stride = weights_broadcast ? 0 : L;
    const long long threads = (long long)P * (C / 4);
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (C == 32)
        hipLaunchKernelGGL(knn_smooth_multi_fwd_kernel<32>, grid, dim3(256), 0, stream, P, ktot, knn_idx, lv, weights, w_stride, features, out, normalize_out);
    else
        hipLaunchKernelGGL(knn_smooth_multi_fwd_kernel<64>, grid, dim3(256), 0, stream, P, ktot, knn_idx, lv, weights, w_stride, features, out, normalize_out);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_knn_smooth_multi_backward(int P, int C, int L, const int* level_k, const int* knn_idx, const int* inv_offsets,
                                 const uint32_t* inv_entries, const float* weights, int weights_broadcast, const float* features,
                                 const float* dL_dout, float* dret, float* dL_dfeatures, float* dL_dweights, int normalize_out,
                                 void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    SmoothLevels lv;
    if (const int rc = smooth_levels(P, C, L, level_k, &lv)) return rc;
    if (P == 0) return MI_RAST_OK;
    if (!knn_idx || !inv_offsets || !inv_entries || !features || !dL_dout || !dret || !dL_dfeatures)
        return fail(MI_RAST_ERR_INVALID, "knn_smooth: need a neighbour map, its inverse lists, features, a gradient, scratch and an output");
    const int ktot = lv.end[L - 1], w_stride = weights_broadcast ? 0 : L;
    const long long threads = (long long)P * (C / 4);
    const dim3 grid((unsigned)((threads + 255) / 256));
    // without the output normalisation dL/dret IS dL/dout: pass A then runs only for dL/dw, and pass B reads dL/dout itself
    const bool pass_a = normalize_out || dL_dweights;
    const float* dret_in = pass_a ? dret : dL_dout;
    if (C == 32) {
        if (pass_a)
            hipLaunchKernelGGL(knn_smooth_multi_bwd_ret_kernel<32>, grid, dim3(256), 0, stream, P, ktot, knn_idx, lv, weights, w_stride, features, dL_dout, dret, dL_dweights, normalize_out);
        hipLaunchKernelGGL(knn_smooth_multi_bwd_feat_kernel<32>, grid, dim3(256), 0, stream, P, inv_offsets, inv_entries, lv, weights, w_stride, features, dret_in, dL_dfeatures);
    } else {
        if (pass_a)
            hipLaunchKernelGGL(knn_smooth_multi_bwd_ret_kernel<64>, grid, dim3(256), 0, stream, P, ktot, knn_idx, lv, weights, w_stride, features, dL_dout, dret, dL_dweights, normalize_out);
        hipLaunchKernelGGL(knn_smooth_multi_bwd_feat_kernel<64>, grid, dim3(256), 0, stream, P, inv_offsets, inv_entries, lv, weights, w_stride, features, dret_in, dL_dfeatures);
    }
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

}  // extern "C"
