/* mi_clip_tiles.h -- C-ABI of the CLIP network's input made from the packed SAM masks, in libmi_rast.so.  The packed layout and the
 * general conventions are mi_mask_scales.h's; `resize` below is its mi_mask_resize.
 */
#ifndef MI_CLIP_TILES_H
#define MI_CLIP_TILES_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- CLIP tiles: the CLIP network's input from the packed masks and the uint8 image (clip_utils/__init__.py:91-191,
 * clip_utils/sam_utils.py:99-114, :212-225).  csrc/mi_clip_tiles.hip.
 *
 * The conventions of mi_mask_sets.h: device pointers, contiguous; nothing is allocated, no workspace; arguments are refused with
 * MI_RAST_ERR_INVALID before any HIP call; 1 <= M <= MI_CONTRASTIVE_LOSS_MAX_MASKS and H * W < 2^24 (h * w too).  No atomics: every
 * result is bit-identical across runs.
 *
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

int mi_mask_clip_tiles(int M, int H, int W, const unsigned long long* packed /* [M,H,ceil(W/64)] */, const unsigned char* image /* [H,W,3] */,
                       const int* rects /* [M,4] */, int layout, float background, int antialias, const float* mean /* host [3] */,
                       const float* std /* host [3] */, int Sh, int Sw, int half, void* tiles /* [M,3,Sh,Sw] */, void* stream);

int mi_mask_index_map(int M, int H, int W, const unsigned long long* packed /* [M,H,ceil(W/64)] */, int offset, int* out /* [H,W] */,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif
