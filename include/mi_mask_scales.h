/* mi_mask_scales.h -- C-ABI of the SAM-mask 3-D scales (get_scale.py:128-159), in libmi_rast.so, and, in the
 * sections at its end, of the set operations on the same packed masks (overlaps, boxes, mask NMS, score images)
 * and of the CLIP network's input made from them (mask resize, masked crops resized and normalised, index map).
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

/* ---- Mask sets: set operations on the packed masks (clip_utils/sam_utils.py:123-187, clip_utils/__init__.py:115, :206, :282, :380;
 * DESIGN.md section 23).  csrc/mi_mask_sets.hip.
 *
 * The same conventions: device pointers, contiguous; `stream` is a hipStream_t; nothing is allocated and no workspace is needed;
 * arguments are refused with MI_RAST_ERR_INVALID before any HIP call.  1 <= M <= MI_CONTRASTIVE_LOSS_MAX_MASKS and H * W < 2^24, so
 * that every pixel count is exact as an f32.  Every result is exact or a fixed-order f32 sum: bit-identical across runs.
 *
 * overlaps     : inter[a, b] = |mask order[a] AND mask order[b]| (M, M) int32, symmetric, the areas on its diagonal; areas (M) int64,
 *                or NULL.  order: (M) int64 indices of masks, or NULL for 0 .. M-1; the masks are read through it, never copied (an
 *                index outside 0 .. M-1 reads as an empty mask).  A memset of inter, one launch over the 64 x 64 tiles of pairs on
 *                or above the diagonal x slices of the words (int32 atomic adds: exact), one launch that mirrors the upper
 *                triangle into the lower one and copies the diagonal to the areas.
 *                Algorithmic bytes: 8 M H Wq read once (31 MB at M = 120, 78 MB at M = 300 and 1080p) + 4 M^2; the work is
 *                M (M + 1) / 2 x H Wq AND + popcount word operations (1.46 G at M = 300 and 1080p).
 * boxes        : boxes (M, 4) f32 = (x_min, y_min, x_max, y_max) of the set pixels, inclusive (torchvision.ops.masks_to_boxes);
 *                four NaN for a mask without a pixel.  areas (M) int64 or NULL.  One launch.  Algorithmic bytes: 8 M H Wq.
 * nms_keep     : the decision of mask_nms (sam_utils.py:160-185) in one launch of one workgroup.  inter, areas and scores are in
 *                DESCENDING-SCORE order (overlaps through the sort's indices).  With s, a, I converted to f32 and every operation
 *                a separate correctly rounded f32 operation: per pair i < j, ri = I / a_i, rj = I / a_j, v = 1 - rj ri,
 *                iou = I / f32(a_i + a_j - I);  iou_max[j] = max(0, iou over i < j);  in_u[j] = max(0, v over i < j with ri < 0.5
 *                and rj >= 0.85);  in_l[c] = max(0, v over the pairs (c, j > c) with r_c >= 0.85 and r_j < 0.5, and v of the pair
 *                (c - 1, c) if it counts for in_u[c] -- the reference's tril keeps the first superdiagonal);  max propagates NaN.
 *                keep[j] = iou_max[j] <= iou_thr and s[j] > score_thr and in_u[j] <= inner_max and in_l[j] <= inner_max, where
 *                inner_max = 1 - inner_thr.  A test (score, in_u, in_l) that no mask passes is set true for the first min(3, M)
 *                masks -- what :173-181 mean to do (as written they raise).  keep: (M) bytes, 0 or 1.
 *                Algorithmic bytes: 4 M^2 read (twice: column j also walks row j by symmetry).
 * score_images : out[k, y, x] over the masks m that cover pixel (y, x), in ascending m with an f32 accumulator:
 *                MI_MASK_SCORE_SUM the sum of scores[m, k] (:380); MI_MASK_SCORE_MEAN that sum / the number of covering masks, 0
 *                where none covers (:282); MI_MASK_SCORE_MAX the maximum of scores[m, k] and, unless all M masks cover the pixel,
 *                0 (:206).  scores (M, K) f32, finite, 1 <= K <= MI_MASK_SCORE_MAX_COLUMNS; out (K, H, W) f32, every element
 *                written: the layout mi_rast_lift reads.  One launch, every K column from one read of the masks, no atomics.
 *                Algorithmic bytes: 8 M H Wq + 4 K H W (78 MB + 8 K MB at M = 300 and 1080p).
 */
#define MI_MASK_SCORE_SUM 0
#define MI_MASK_SCORE_MEAN 1
#define MI_MASK_SCORE_MAX 2
#define MI_MASK_SCORE_MAX_COLUMNS 64

int mi_mask_overlaps(int M, int H, int W, const unsigned long long* packed /* [M,H,ceil(W/64)] */, const long long* order /* [M] or NULL */,
                     int* inter /* [M,M] */, long long* areas /* [M] or NULL */, void* stream);

int mi_mask_boxes(int M, int H, int W, const unsigned long long* packed /* [M,H,ceil(W/64)] */, float* boxes /* [M,4] */,
                  long long* areas /* [M] or NULL */, void* stream);

int mi_mask_nms_keep(int M, const int* inter /* [M,M] */, const long long* areas /* [M] */, const float* scores /* [M] */, float iou_thr,
                     float score_thr, float inner_max, unsigned char* keep /* [M] */, void* stream);

int mi_mask_score_images(int M, int H, int W, int K, const unsigned long long* packed /* [M,H,ceil(W/64)] */,
                         const float* scores /* [M,K] */, int mode, float* out /* [K,H,W] */, void* stream);

/* ---- CLIP tiles: the CLIP network's input from the packed masks and the uint8 image (clip_utils/__init__.py:91-191,
 * clip_utils/sam_utils.py:99-114, :212-225).  resize in csrc/mi_mask_scales.hip, the rest in csrc/mi_clip_tiles.hip.
 *
 * The conventions of the section above: device pointers, contiguous; nothing is allocated, no workspace; arguments are refused with
 * MI_RAST_ERR_INVALID before any HIP call; 1 <= M <= MI_CONTRASTIVE_LOSS_MAX_MASKS and H * W < 2^24 (h * w too).  No atomics: every
 * result is bit-identical across runs.
 *
 * resize     : packed_in (M, h, w) -> packed_out (M, H, W): bit (y, x) = F.interpolate(masks.float(), (H, W), mode='bilinear')[y, x]
 *              > threshold (:99-102, threshold 0.5), the value being PyTorch's CPU bilinear weight pair of 4 source bits exactly as the
 *              resampled branch of erode computes it (width pass a w0 + b w1, height pass one fused multiply-add).  Padding bits 0;
 *              packed_out must not overlap packed_in.  At the same size the value is the bit itself: a copy for 0 <= threshold < 1.
 *              One launch, one wave per output word.  Algorithmic bytes: 8 M (h Wq_in + H Wq).
 * clip_tiles : tiles (M, 3, Sh, Sw), f32 (half = 0) or f16 (half = 1): per mask m the rectangle rects[m] = [X0, Y0, X1, Y1) of the
 *              image, int32, half-open, free to leave the image, resized to Sh x Sw and normalised.  Crop pixel (y, x), channel c:
 *              f32(image[Y0 + y, X0 + x, c]) / 255.0f (one correctly rounded division) where the pixel is inside the image and mask m
 *              has its bit, `background` elsewhere.  MI_CLIP_TILES_CROP: the source plane is the ch x cw crop; MI_CLIP_TILES_PAD_SQUARE
 *              (pad_img): an L x L plane, L = max(ch, cw), the crop at column (L - cw) / 2 when ch > cw, else at row (L - ch) / 2, the
 *              rest `background`.  Resize as PyTorch's CPU kernels order it (torchvision's Resize on a tensor): width pass, then height
 *              pass, f32.  antialias = 0: the taps of resize above, a l0 + b l1 along the width, fmaf(t0, wy0, t1 wy1) along the
 *              height.  antialias = 1: the weights of _upsample_bilinear2d_aa in f32: scale = f32(in) / f32(out), support = scale and
 *              inv = 1 / scale if scale >= 1, else both 1; center = scale (i + 0.5f), xmin = max(0, int(center - support + 0.5f)),
 *              xmax = min(int(center + support + 0.5f), in), w_j = max(0, 1 - |((j - center) + 0.5f) inv|) for xmin <= j < xmax, each
 *              divided by their sum taken in ascending j; both passes add w_j v_j in ASCENDING j (source column, then source row).
 *              Then (r - mean[c]) / std[c] in f32, subtract then divide, and one round-to-nearest conversion.  A rectangle that is
 *              empty or has a side above MI_CLIP_TILES_MAX_SIDE gives f32((background - mean[c]) / std[c]) in every element.
 *              1 <= Sh, Sw <= MI_CLIP_TILES_MAX_SIZE; std[c] != 0.  One launch: a workgroup per (mask, band of 8 output rows); both tap
 *              loops are bounded by the crop alone.
 *              Algorithmic bytes: sum over the masks of 8 ch ceil(cw / 64) + 3 ch cw + 2 x 3 Sh Sw (f16): 90 MB written at M = 300.
 * index_map  : out (H, W) int32 = offset + the highest m whose mask covers the pixel, -1 (no offset) where none does
 *              (sam_utils.py:214, :221, :62).  One launch, the mask words read once.  Algorithmic bytes: 8 M H Wq + 4 H W.
 */
#define MI_CLIP_TILES_CROP 0
#define MI_CLIP_TILES_PAD_SQUARE 1
#define MI_CLIP_TILES_MAX_SIZE 512
#define MI_CLIP_TILES_MAX_SIDE 32768

int mi_mask_resize(int M, int h, int w, const unsigned long long* packed_in /* [M,h,ceil(w/64)] */, int H, int W, float threshold,
                   unsigned long long* packed_out /* [M,H,ceil(W/64)] */, void* stream);

int mi_mask_clip_tiles(int M, int H, int W, const unsigned long long* packed /* [M,H,ceil(W/64)] */, const unsigned char* image /* [H,W,3] */,
                       const int* rects /* [M,4] */, int layout, float background, int antialias, const float* mean /* host [3] */,
                       const float* std /* host [3] */, int Sh, int Sw, int half, void* tiles /* [M,3,Sh,Sw] */, void* stream);

int mi_mask_index_map(int M, int H, int W, const unsigned long long* packed /* [M,H,ceil(W/64)] */, int offset, int* out /* [H,W] */,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif
