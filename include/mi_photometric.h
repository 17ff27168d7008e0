/* mi_photometric.h -- C-ABI of the 3DGS photometric loss (train_scene.py:101-104 with utils/loss_utils.py:17-63; DESIGN.md
 * section 17), in libmi_rast.so.
 *
 *     loss = (1 - lambda) mean |x - g|  +  lambda (1 - mean ssim_map(x, g))
 *
 * ssim_map: the reference's 11 x 11 Gaussian window (sigma 1.5, taps normalised in binary32, zero padding of 5, not renormalised
 * at the border) applied separably; mu_x, mu_g, s_x = conv(x x) - mu_x^2, s_g, s_xg;
 * ssim = (2 mu_x mu_g + C1)(2 s_xg + C2) / ((mu_x^2 + mu_g^2 + C1)(s_x + s_g + C2)), C1 = 0.01^2, C2 = 0.03^2.
 *
 * image, target: P = images * planes_per_image planes of H x W binary32, contiguous; H, W >= 1, P H W < 2^31.  All pointers are
 * device pointers, 4-byte aligned; outputs must not overlap inputs; `stream` is a hipStream_t.  No atomics; nothing is allocated
 * and nothing kept between calls; the functions are re-entrant and their results bit-identical from run to run.
 * Returns 0 or an MI_RAST_ERR_* code (mi_rast_last_error() holds the text).
 *
 * forward  : two launches.  `parts` = MI_PHOTO_L1, MI_PHOTO_SSIM or both; a part left out is not computed and reads 0.
 *            out[3 + 2 * images] binary32 = { loss, mean |x - g|, mean ssim, then per image: mean |x - g|, mean ssim }; the sums
 *            run in binary64 (per-tile partials in the workspace, added in a fixed order) and are rounded once.
 *            maps: NULL, or 3 P H W binary32 that receive the derivative maps the backward reads (needs MI_PHOTO_SSIM).
 *            Algorithmic bytes: 8 P H W read (+ 12 P H W written with maps).
 * backward : one launch.  grad[i] = go * (w_l1 * sign(x - g) + w_ssim * d(sum ssim_map)/dx[i]), sign(0) = 0, where
 *            go = grad_out[image of i] (grad_per_image != 0) or grad_out[0], read on the device.  The loss above is
 *            w_l1 = (1 - lambda) / N, w_ssim = -lambda / N, N = P H W.  maps: what the forward wrote for the same image and target;
 *            NULL with w_ssim == 0 (the L1 term alone).  Algorithmic bytes: 20 P H W read + 4 P H W written.
 */
#ifndef MI_PHOTOMETRIC_H
#define MI_PHOTOMETRIC_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_PHOTO_L1 1
#define MI_PHOTO_SSIM 2
#define MI_PHOTO_WINDOW 11
#define MI_PHOTO_TILE_H 32
#define MI_PHOTO_TILE_W 64

/* bytes of the workspace mi_photo_loss_forward needs: 16 per tile, P ceil(H / 32) ceil(W / 64) tiles; 0 for sizes out of range */
size_t mi_photo_loss_workspace_bytes(int P, int H, int W);

/* the 11 one-dimensional window taps the kernels use, and (excess != NULL) the relative excess of the sum of the reference's 2-D
 * window -- the taps' outer product rounded to binary32 -- over the sum of the exact outer product, which the forward corrects for */
void mi_photo_loss_window(float* taps /* [11], host */, double* excess /* host, or NULL */);

int mi_photo_loss_forward(int images, int planes_per_image, int H, int W, const float* image, const float* target, double lambda_dssim,
                          int parts, float* maps /* [3][P,H,W] or NULL */, void* workspace, size_t workspace_bytes,
                          float* out /* [3 + 2 images] */, void* stream);

int mi_photo_loss_backward(int images, int planes_per_image, int H, int W, const float* image, const float* target,
                           const float* maps /* [3][P,H,W] or NULL */, const float* grad_out /* [images] or [1] */, int grad_per_image,
                           float w_l1, float w_ssim, float* grad /* [P,H,W] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
