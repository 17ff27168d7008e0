/* mi_mask_sets.h -- C-ABI of the set operations on the packed SAM masks, in libmi_rast.so.  The packed layout and the general
 * conventions are mi_mask_scales.h's ("the same conventions" below).
 */
#ifndef MI_MASK_SETS_H
#define MI_MASK_SETS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif
