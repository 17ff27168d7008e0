// mi_photometric.hip -- C-ABI implementation of include/mi_photometric.h.
#include "host.h"
#include "../../include/mi_photometric.h"

#include "photometric.h"   // RGB-training loss: fused L1 + D-SSIM forward and backward

using namespace mirast;

namespace {
int ph_check(int images, int planes_per_image, int H, int W)
{
    if (images < 1 || planes_per_image < 1 || H < 1 || W < 1) return fail(MI_RAST_ERR_INVALID, "photometric: need images, planes, H, W >= 1");
    if ((size_t)images * planes_per_image * H * W >= ((size_t)1 << 31)) return fail(MI_RAST_ERR_INVALID, "photometric: 2^31 elements or more");
    return MI_RAST_OK;
}
int ph_tiles_x(int W) { return (W + PH_TW - 1) / PH_TW; }
int ph_tiles_y(int H) { return (H + PH_TH - 1) / PH_TH; }
}  // namespace

extern "C" {

size_t mi_photo_loss_workspace_bytes(int P, int H, int W)
{
    if (P < 1 || H < 1 || W < 1 || (size_t)P * H * W >= ((size_t)1 << 31)) return 0;
    return (size_t)P * ph_tiles_x(W) * ph_tiles_y(H) * 2 * sizeof(double);
}

void mi_photo_loss_window(float* taps, double* excess)
{
    if (excess) *excess = ph_window_excess();
    static_assert(MI_PHOTO_WINDOW == PH_TAPS && MI_PHOTO_TILE_H == PH_TH && MI_PHOTO_TILE_W == PH_TW, "mi_photometric.h and photometric.h disagree");
    for (int k = 0; k < PH_TAPS; k++) taps[k] = PH_WINDOW.w[k];
}

int mi_photo_loss_forward(int images, int planes_per_image, int H, int W, const float* image, const float* target, double lambda_dssim,
                          int parts, float* maps, void* workspace, size_t workspace_bytes, float* out, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = ph_check(images, planes_per_image, H, W)) return rc;
    if (!image || !target || !workspace || !out) return fail(MI_RAST_ERR_INVALID, "photometric: null pointer");
    if (parts < 1 || parts > (MI_PHOTO_L1 | MI_PHOTO_SSIM)) return fail(MI_RAST_ERR_INVALID, "photometric: parts must be MI_PHOTO_L1, MI_PHOTO_SSIM or both");
    if (maps && !(parts & MI_PHOTO_SSIM)) return fail(MI_RAST_ERR_INVALID, "photometric: derivative maps need MI_PHOTO_SSIM");
    if (!(lambda_dssim == lambda_dssim)) return fail(MI_RAST_ERR_INVALID, "photometric: lambda_dssim is NaN");
    const int P = images * planes_per_image;
    if (workspace_bytes < mi_photo_loss_workspace_bytes(P, H, W))
        return fail(MI_RAST_ERR_INVALID, "photometric: workspace smaller than mi_photo_loss_workspace_bytes(P, H, W)");
    const int tx = ph_tiles_x(W), ty = ph_tiles_y(H);
    const size_t blocks = (size_t)P * tx * ty;
    if (blocks >= ((size_t)1 << 31)) return fail(MI_RAST_ERR_INVALID, "photometric: too many tiles");
    const size_t n = (size_t)P * H * W;
    if (parts & MI_PHOTO_SSIM)
        hipLaunchKernelGGL(ph_fwd_kernel<true>, dim3((unsigned)blocks), dim3(PH_THREADS), 0, stream, H, W, tx, ty, image, target, maps, n,
                           (double*)workspace);
    else
        hipLaunchKernelGGL(ph_fwd_kernel<false>, dim3((unsigned)blocks), dim3(PH_THREADS), 0, stream, H, W, tx, ty, image, target,
                           (float*)nullptr, n, (double*)workspace);
    hipLaunchKernelGGL(ph_finalize_kernel, dim3(1), dim3(PH_THREADS), 0, stream, images, planes_per_image * tx * ty,
                       (double)planes_per_image * H * W, lambda_dssim, (const double*)workspace, out);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_photo_loss_backward(int images, int planes_per_image, int H, int W, const float* image, const float* target, const float* maps,
                           const float* grad_out, int grad_per_image, float w_l1, float w_ssim, float* grad, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = ph_check(images, planes_per_image, H, W)) return rc;
    if (!image || !target || !grad_out || !grad) return fail(MI_RAST_ERR_INVALID, "photometric: null pointer");
    if (!(w_l1 == w_l1) || !(w_ssim == w_ssim)) return fail(MI_RAST_ERR_INVALID, "photometric: a weight is NaN");
    if (w_ssim != 0.f && !maps) return fail(MI_RAST_ERR_INVALID, "photometric: w_ssim != 0 needs the forward's derivative maps");
    const int P = images * planes_per_image;
    const int tx = ph_tiles_x(W), ty = ph_tiles_y(H);
    const size_t blocks = (size_t)P * tx * ty;
    if (blocks >= ((size_t)1 << 31)) return fail(MI_RAST_ERR_INVALID, "photometric: too many tiles");
    const size_t n = (size_t)P * H * W;
    if (w_ssim != 0.f)
        hipLaunchKernelGGL(ph_bwd_kernel<true>, dim3((unsigned)blocks), dim3(PH_THREADS), 0, stream, H, W, tx, ty, planes_per_image, image,
                           target, maps, n, grad_out, grad_per_image ? 1 : 0, w_l1, w_ssim, grad);
    else
        hipLaunchKernelGGL(ph_bwd_kernel<false>, dim3((unsigned)blocks), dim3(PH_THREADS), 0, stream, H, W, tx, ty, planes_per_image, image,
                           target, (const float*)nullptr, n, grad_out, grad_per_image ? 1 : 0, w_l1, w_ssim, grad);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

}  // extern "C"
