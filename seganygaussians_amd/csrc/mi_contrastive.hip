// mi_contrastive.hip -- C-ABI implementation of include/mi_contrastive.h: the contrastive-loss front end and the loss itself.
#include "host.h"
#include "../../include/mi_contrastive.h"

#include <algorithm>

#include "contrastive.h"
#include "contrastive_loss.h"   // the loss itself: SAM-mask targets and the pair loss

using namespace mirast;

extern "C" {

// ---- contrastive-loss front end (mi_contrastive.h, contrastive.h) --------------------------------------------------------
int mi_contrastive_forward(int C, int h, int w, const float* rendered, int H, int W, int S, const int* ray_yx, int N,
                           const float* gates, float* out, float* ray_feat, float* inv_len, float* inv_norm,
                           double* norm_sum, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (C < 1 || h < 1 || w < 1 || H < 1 || W < 1 || S < 0 || N < 1) return fail(MI_RAST_ERR_INVALID, "contrastive: need C, h, w, H, W, N >= 1 and S >= 0");
    if (S > 0 && C > 64 * CT_MAX_CPL) return fail(MI_RAST_ERR_INVALID, "contrastive: at most 256 channels");
    // what the loss that consumes `out` accepts (cl_check_loss): refused here, before anything is computed, not in the backward
    if (S > 0 && N > MI_CONTRASTIVE_LOSS_MAX_SCALES) return fail(MI_RAST_ERR_INVALID, "contrastive: at most 32 scales");
    if (!rendered || !inv_norm || !norm_sum || !gates) return fail(MI_RAST_ERR_INVALID, "contrastive: null pointer");
    if (S > 0 && (!ray_yx || !out || !ray_feat || !inv_len)) return fail(MI_RAST_ERR_INVALID, "contrastive: null ray buffers");
    const size_t HW = (size_t)h * w;
    const bool vec = HW % 4 == 0 && ((uintptr_t)rendered % 16) == 0 && ((uintptr_t)inv_norm % 16) == 0;
    const size_t per_block = (size_t)CT_THREADS * (vec ? 4 : 1);
    const uint32_t dense_blocks = (uint32_t)((HW + per_block - 1) / per_block);
    const uint32_t ray_blocks = (uint32_t)((S + CT_THREADS / 64 - 1) / (CT_THREADS / 64));
    if (vec)
        hipLaunchKernelGGL(contrastive_fwd_kernel<4>, dim3(dense_blocks + ray_blocks), dim3(CT_THREADS), 0, stream, C, h, w, rendered, H, W, S,
                           ray_yx, N, gates, out, ray_feat, inv_len, inv_norm, norm_sum, dense_blocks);
    else
        hipLaunchKernelGGL(contrastive_fwd_kernel<1>, dim3(dense_blocks + ray_blocks), dim3(CT_THREADS), 0, stream, C, h, w, rendered, H, W, S,
                           ray_yx, N, gates, out, ray_feat, inv_len, inv_norm, norm_sum, dense_blocks);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_contrastive_backward(int C, int h, int w, const float* rendered, int H, int W, int S, const int* ray_yx, int N,
                            const float* gates, const float* out, const float* ray_feat, const float* inv_len,
                            const float* inv_norm, const float* dL_dout, const float* g_norm, float* dL_drendered,
                            float* dL_dgates, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (C < 1 || h < 1 || w < 1 || H < 1 || W < 1 || S < 0 || N < 1) return fail(MI_RAST_ERR_INVALID, "contrastive: need C, h, w, H, W, N >= 1 and S >= 0");
    if (!rendered || !inv_norm || !dL_drendered) return fail(MI_RAST_ERR_INVALID, "contrastive: null pointer");
    if (S > 0 && (!ray_yx || !out || !ray_feat || !inv_len || !dL_dout || !gates || !dL_dgates)) return fail(MI_RAST_ERR_INVALID, "contrastive: null ray buffers");
    if (S > 0 && C > 64 * CT_MAX_CPL) return fail(MI_RAST_ERR_INVALID, "contrastive: at most 256 channels");
    if (S > 0 && N > MI_CONTRASTIVE_LOSS_MAX_SCALES) return fail(MI_RAST_ERR_INVALID, "contrastive: at most 32 scales");
    // the gate gradients of a workgroup's four rays meet in LDS, at most CT_LDS_FLOATS per wave (64 KiB in all) at a time
    const int gates_per_pass = S > 0 ? std::min(N, CT_LDS_FLOATS / C) : 0;
    const size_t lds = (size_t)(CT_THREADS / 64) * gates_per_pass * C * sizeof(float);
    const size_t HW = (size_t)h * w;
    const bool vec = HW % 4 == 0 && ((uintptr_t)rendered % 16) == 0 && ((uintptr_t)inv_norm % 16) == 0 && ((uintptr_t)dL_drendered % 16) == 0;
    const size_t per_block = (size_t)CT_THREADS * (vec ? 4 : 1);
    const uint32_t dense_blocks = (uint32_t)((HW + per_block - 1) / per_block);
    if (vec)
        hipLaunchKernelGGL(contrastive_bwd_dense_kernel<4>, dim3(dense_blocks), dim3(CT_THREADS), 0, stream, C, h, w, rendered, inv_norm, g_norm, dL_drendered);
    else
        hipLaunchKernelGGL(contrastive_bwd_dense_kernel<1>, dim3(dense_blocks), dim3(CT_THREADS), 0, stream, C, h, w, rendered, inv_norm, g_norm, dL_drendered);
    if (S > 0) {
        const uint32_t ray_blocks = (uint32_t)((S + CT_THREADS / 64 - 1) / (CT_THREADS / 64));
        hipLaunchKernelGGL(contrastive_bwd_rays_kernel, dim3(ray_blocks), dim3(CT_THREADS), lds, stream, C, h, w, H, W, S, ray_yx, N, gates_per_pass, gates,
                           out, ray_feat, inv_len, dL_dout, dL_drendered, dL_dgates);
    }
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}


// ---- contrastive loss: SAM-mask targets and the pair loss (mi_contrastive.h, contrastive_loss.h) ------------------------------
namespace {
int cl_check_loss(int S, int N, int C, int M)
{
    if (S < 0 || N < 1 || N > MI_CONTRASTIVE_LOSS_MAX_SCALES || C < 1 || C > 256 || M < 1 || M > MI_CONTRASTIVE_LOSS_MAX_MASKS)
        return fail(MI_RAST_ERR_INVALID, "contrastive loss: need S >= 0, 1 <= N <= 32, 1 <= C <= 256, 1 <= M <= 1024");
    if ((size_t)S * S >= ((size_t)1 << 40)) return fail(MI_RAST_ERR_INVALID, "contrastive loss: too many sampled rays");
    return MI_RAST_OK;
}
}  // namespace

int mi_contrastive_pack_masks(int M, int H, int W, const unsigned char* masks, unsigned long long* packed, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = pm_check_dims("contrastive loss", M, H, W)) return rc;
    if (!masks || !packed) return fail(MI_RAST_ERR_INVALID, "contrastive loss: null pointer");
    const size_t words = pm_words(M, H, W);
    hipLaunchKernelGGL(cl_pack_kernel, dim3((unsigned)((words + CL_THREADS - 1) / CL_THREADS)), dim3(CL_THREADS), 0, stream, M, H, W, pm_row_words(W),
                       (const uint8_t*)masks, (uint64_t*)packed);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_contrastive_cover(int M, int H, int W, const unsigned long long* packed, const float* ray_rand, float rate,
                         unsigned char* sampled_ray, unsigned long long* acc, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = pm_check_dims("contrastive loss", M, H, W)) return rc;
    if (!packed || !ray_rand || !sampled_ray || !acc) return fail(MI_RAST_ERR_INVALID, "contrastive loss: null pointer");
    const int Wq = pm_row_words(W);
    const size_t words = (size_t)H * Wq;
    hipLaunchKernelGGL(cl_cover_kernel, dim3((unsigned)((words + CL_THREADS - 1) / CL_THREADS)), dim3(CL_THREADS), 0, stream, M, H, W, Wq,
                       (const uint64_t*)packed, ray_rand, rate, (uint8_t*)sampled_ray, acc + CL_ACC_AREA);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_contrastive_targets(int M, int H, int W, const unsigned long long* packed, const long long* sort_idx, int S, const int* ray_yx,
                           int N, const int* scale_si, const int* scale_ub, unsigned long long* gt, float* a, unsigned long long* acc,
                           void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = pm_check_dims("contrastive loss", M, H, W)) return rc;
    if (int rc = cl_check_loss(S, N, 1, M)) return rc;
    if (!packed || !sort_idx || !scale_si || !scale_ub || !acc) return fail(MI_RAST_ERR_INVALID, "contrastive loss: null pointer");
    if (S == 0) return MI_RAST_OK;
    if (!ray_yx || !gt || !a) return fail(MI_RAST_ERR_INVALID, "contrastive loss: null ray buffers");
    const int Wq = pm_row_words(W), Wd = (M + 63) / 64;
    hipLaunchKernelGGL(cl_targets_kernel, dim3((unsigned)(((size_t)S * 64 + CL_THREADS - 1) / CL_THREADS)), dim3(CL_THREADS), 0, stream,
                       M, H, Wq, (const uint64_t*)packed, (const int64_t*)sort_idx, S, ray_yx, N, scale_si, scale_ub, Wd, (uint64_t*)gt, a, acc);
    hipLaunchKernelGGL(cl_classes_kernel, dim3((unsigned)S), dim3(CL_THREADS), 0, stream, S, N, Wd, (const uint64_t*)gt, acc);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_contrastive_loss_forward(int S, int N, int C, int M, const float* feats, const unsigned long long* gt, const float* a,
                                const unsigned long long* acc, const float* rand, double* partials, float* out_f32, long long* out_i64,
                                void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = cl_check_loss(S, N, C, M)) return rc;
    if (!acc || !out_f32 || !out_i64) return fail(MI_RAST_ERR_INVALID, "contrastive loss: null pointer");
    if (S > 0 && (!feats || !gt || !a || !rand || !partials)) return fail(MI_RAST_ERR_INVALID, "contrastive loss: null ray buffers");
    const int Wd = (M + 63) / 64;
    const size_t lds = (size_t)CL_ROW_STATS * CL_THREADS * sizeof(double) + (size_t)N * CL_THREADS * sizeof(float) + (size_t)N * Wd * sizeof(uint64_t);
    if (S > 0)
        hipLaunchKernelGGL(cl_loss_fwd_kernel, dim3((unsigned)S), dim3(CL_THREADS), lds, stream, S, N, C, Wd, feats, (const uint64_t*)gt, a,
                           acc, rand, partials);
    hipLaunchKernelGGL(cl_loss_final_kernel, dim3(1), dim3(CL_THREADS), 0, stream, S, N, (const double*)partials, out_f32, out_i64);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_contrastive_loss_backward(int S, int N, int C, int M, const float* feats, const unsigned long long* gt, const float* a,
                                 const unsigned long long* acc, const float* rand, const long long* out_i64, const float* g_loss,
                                 float* dL_dfeats, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = cl_check_loss(S, N, C, M)) return rc;
    if (S == 0) return MI_RAST_OK;
    if (!feats || !gt || !a || !acc || !rand || !out_i64 || !g_loss || !dL_dfeats) return fail(MI_RAST_ERR_INVALID, "contrastive loss: null pointer");
    const int Wd = (M + 63) / 64;
    const size_t lds = (size_t)N * CL_THREADS * sizeof(float) + (size_t)N * Wd * sizeof(uint64_t);
    hipLaunchKernelGGL(cl_loss_bwd_kernel, dim3((unsigned)S), dim3(CL_THREADS), lds, stream, S, N, C, Wd, feats, (const uint64_t*)gt, a, acc,
                       rand, out_i64, g_loss, dL_dfeats);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

}  // extern "C"
