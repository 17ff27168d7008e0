/* mi_mask_scales.h -- C-ABI of the SAM-mask 3-D scales (get_scale.py:128-159; csrc/mi_mask_scales.hip), in
 * libmi_rast.so, and of the mask resize that shares the erosion's taps.  The set operations on the same packed masks are in
 * mi_mask_sets.h, the CLIP network's input made from them in mi_clip_tiles.h.
 *
 * Produces cam.mask_scales, the input of the contrastive loss (mi_contrastive.h), from a rendered depth and the SAM masks:
 *
 *     points[y, x] = ((y - W/2) d / fx, (x - H/2) d / fy, d)      d = depth[y, x]; the row index pairs with W/2, as :136-143 write it
 *     up = F.interpolate(masks[:, None], (H, W), mode='bilinear', align_corners=False)                        (:145)
 *     eroded = conv2d(up, ones(3, 3), padding=1) >= 5                                                        (:147-152)
 *     scale[m] = (points[eroded[m]].std(dim=0) * 2).norm() = 2 sqrt(var_x + var_y + var_z), unbiased         (:154-157)
 *
 * Masks are bit-packed as in mi_contrastive.h: (M, H, Wq) 64-bit words, Wq = ceil(W / 64), bit b of word q = pixel 64 q + b, padding
 * bits 0.  All pointers are device pointers, contiguous; `stream` is a hipStream_t.  1 <= M <= MI_CONTRASTIVE_LOSS_MAX_MASKS,
 * M * H * Wq < 2^31 words on either side.  Nothing is allocated; the functions are re-entrant.
 * Returns 0 or an MI_RAST_ERR_* code (mi_rast_last_error() holds the text).
 *
 * erode  : one launch.  packed_in (M, h, w) -> packed_out (M, H, W) eroded, padding bits 0; packed_out must not overlap packed_in.
 *          h == H and w == W: the bilinear resampling is the identity and the erosion is the bit-sliced majority of the 3x3 window
 *          (64 pixels per lane).  Otherwise each resampled value is PyTorch's CPU bilinear weight pair of 4 source bits and the
 *          3x3 window is summed in f32 in row-major order.
 *          Algorithmic bytes: 8 M (h Wq_in + H Wq) (31 MB read + 31 MB written at M = 120 and 1080p).
 *          erode_min_sum is the same with the threshold as an argument (3x3 box sum >= min_sum; the notebook's language section has
 *          2): erode is erode_min_sum at 5.  At the same size the count is an integer and the test is count >= ceil(min_sum).
 * scales : two launches.  eroded (M, H, W) packed, depth (H, W) f32, fx = (W/2) / tan(fovx/2), fy = (H/2) / tan(fovy/2) ->
 *          scales (M) f32 and counts (M) int64 (the eroded pixel count of each mask).  count < 2 gives NaN, as torch's std of 0
 *          or 1 rows.  Moments in f64; per-tile partials in the workspace, reduced in a fixed order: bit-identical across runs.
 *          Algorithmic bytes: 8 M H Wq + 4 H W (31 MB + 8 MB at M = 120 and 1080p), plus the partials, written once and read once.
 * resize     : packed_in (M, h, w) -> packed_out (M, H, W): bit (y, x) = F.interpolate(masks.float(), (H, W), mode='bilinear')[y, x]
 *              > threshold (:99-102, threshold 0.5), the value being PyTorch's CPU bilinear weight pair of 4 source bits exactly as the
 *              resampled branch of erode computes it (width pass a w0 + b w1, height pass one fused multiply-add).  Padding bits 0;
 *              packed_out must not overlap packed_in.  At the same size the value is the bit itself: a copy for 0 <= threshold < 1.
 *              One launch, one wave per output word.  Algorithmic bytes: 8 M (h Wq_in + H Wq).
 *              (:99-102 is clip_utils/sam_utils.py's; H * W < 2^24, h * w too; refused with MI_RAST_ERR_INVALID before any HIP call.)
 */
#ifndef MI_MASK_SCALES_H
#define MI_MASK_SCALES_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the workspace mi_mask_scales needs for M masks at H x W (M ceil(H / 16) ceil(W / 64) x 40) */
size_t mi_mask_scales_workspace_bytes(int M, int H, int W);

int mi_mask_erode(int M, int h, int w, const unsigned long long* packed_in /* [M,h,ceil(w/64)] */, int H, int W,
                  unsigned long long* packed_out /* [M,H,ceil(W/64)] */, void* stream);

int mi_mask_erode_min_sum(int M, int h, int w, const unsigned long long* packed_in /* [M,h,ceil(w/64)] */, int H, int W, float min_sum,
                          unsigned long long* packed_out /* [M,H,ceil(W/64)] */, void* stream);

int mi_mask_scales(int M, int H, int W, const unsigned long long* eroded /* [M,H,ceil(W/64)] */, const float* depth /* [H,W] */,
                   double fx, double fy, void* workspace, size_t workspace_bytes, float* scales /* [M] */, long long* counts /* [M] */,
                   void* stream);

int mi_mask_resize(int M, int h, int w, const unsigned long long* packed_in /* [M,h,ceil(w/64)] */, int H, int W, float threshold,
                   unsigned long long* packed_out /* [M,H,ceil(W/64)] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
