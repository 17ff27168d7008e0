"""Set operations on SAM masks on the MI355X: pairwise overlaps, boxes, mask NMS and score images.

The 2-D side of the open-vocabulary path between the two networks.  The reference decides which SAM masks exist with a Python double
loop over all mask pairs (clip_utils/sam_utils.py:123-202, mask_nms / masks_update) and paints per-mask CLIP scores into per-view
score images by multiplying an (M, H, W) float tensor of masks (clip_utils/__init__.py:206, :282, :380).  Here the masks stay
bit-packed on the device, in the PackedSamMasks layout (pack_sam_masks), and nothing of size (M, H, W) is formed:

  * mask_overlaps()     -- AND + popcount over all pairs, tiled like a GEMM; read through an optional order.
  * masks_to_boxes()    -- torchvision.ops.masks_to_boxes in one pass over the words; NaN rows for empty masks.
  * mask_nms()          -- sam_utils.py:138-187: torch.sort, the overlaps through the order, one decision launch, idx[keep].
  * masks_update()      -- sam_utils.py:189-202 for SAM's lists of dicts.
  * mask_score_images() -- the masked sum / mean / max of per-mask scores per pixel, the input of lift_scores / vote_3d_mask.
  * resize_sam_masks()  -- F.interpolate(masks.float(), size, mode='bilinear') > threshold (clip_utils/__init__.py:99-102), packed
                           to packed; the masks at the image's size that clip_tiles.clip_tiles() wants.
  * mask_index_map()    -- the per-pixel index of the last mask that covers it, -1 where none does (sam_utils.py:214, :221).

Limits, refused with ValueError before any launch: 1 <= M <= 1024, h * w < 2^24 (every pixel count is exact as a float32),
1 <= K <= 64 score columns, float32 tensors on one GPU.  No autograd."""
from __future__ import annotations

import torch

from . import _lib
from ._args import check_out, f32, number, size_hw
from ._ffi import check, stream_ptr
from .packed_masks import MAX_MASKS, MAX_PIXELS, PackedSamMasks, as_packed, check_shape, row_words

MAX_SCORE_COLUMNS = _lib.MI_MASK_SCORE_MAX_COLUMNS


def _packed(masks, scores, who: str) -> PackedSamMasks:
    """masks as a PackedSamMasks on the GPU of `scores` (None: on their own GPU, or the current one for CPU masks)."""
    check_shape(who, masks)
    dev = None
    if scores is not None:
        if not scores.is_cuda:
            raise ValueError(f"{who}: scores must be on a GPU, got {scores.device}")
        dev = scores.device
    return as_packed(who, masks, dev, "scores")


def _overlaps(packed: PackedSamMasks, order):
    M, h, w = packed.shape
    dev = packed.device
    inter = torch.empty((M, M), device=dev, dtype=torch.int32)
    areas = torch.empty((M,), device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        check(_lib.load().mi_mask_overlaps(M, h, w, packed.words.data_ptr(), None if order is None else order.data_ptr(),
                                           inter.data_ptr(), areas.data_ptr(), stream_ptr(dev)))
    return inter, areas


def mask_overlaps(masks, order=None):
    """The pairwise intersections of M masks: (inter, areas).

    masks: bool (M, h, w) on the CPU or a GPU (packed here), or a PackedSamMasks.  order: optional (M,) int64 permutation of
    0 .. M-1 on the masks' GPU; the masks are read through it and never copied (checked here, at the cost of one synchronisation).
    inter: (M, M) int32, inter[a, b] = the number of pixels in both mask order[a] and mask order[b]; symmetric, the areas on its
    diagonal.  areas: (M,) int64 in the same order.  Exact."""
    packed = _packed(masks, None, "mask_overlaps")
    M = packed.shape[0]
    if order is not None:
        if not isinstance(order, torch.Tensor) or order.dtype != torch.int64 or tuple(order.shape) != (M,):
            raise ValueError(f"mask_overlaps: order must be an int64 ({M},) tensor, got "
                             f"{getattr(order, 'dtype', type(order))} {tuple(getattr(order, 'shape', ()))}")
        if order.device != packed.device:
            raise ValueError(f"mask_overlaps: the masks are on {packed.device}, the order on {order.device}")
        order = order.contiguous()
        if not torch.equal(torch.sort(order).values, torch.arange(M, device=order.device)):
            raise ValueError("mask_overlaps: order must be a permutation of 0 .. M-1")
    return _overlaps(packed, order)


def masks_to_boxes(masks, return_areas: bool = False):
    """torchvision.ops.masks_to_boxes (clip_utils/__init__.py:115) on packed masks: (M, 4) float32 rows (x_min, y_min, x_max, y_max)
    of the set pixels, inclusive.  A mask with no pixel gets a NaN row (torchvision raises there; sam_mask_scales answers NaN for
    degenerate masks too).  With return_areas, also the pixel counts (M,) int64."""
    packed = _packed(masks, None, "masks_to_boxes")
    M, h, w = packed.shape
    dev = packed.device
    boxes = torch.empty((M, 4), device=dev, dtype=torch.float32)
    areas = torch.empty((M,), device=dev, dtype=torch.int64) if return_areas else None
    with torch.cuda.device(dev):
        check(_lib.load().mi_mask_boxes(M, h, w, packed.words.data_ptr(), boxes.data_ptr(),
                                        None if areas is None else areas.data_ptr(), stream_ptr(dev)))
    return (boxes, areas) if return_areas else boxes


def mask_nms(masks, scores, iou_thr=0.7, score_thr=0.1, inner_thr=0.2, **kwargs):
    """clip_utils/sam_utils.py:123-187: mask non-maximum suppression.  Returns selected_idx (int64, on the scores' GPU), the kept
    masks in descending-score order, like the reference's idx[keep].

    masks: bool (M, h, w) on the CPU or the scores' GPU, or a PackedSamMasks there; scores: (M,) float32 on a GPU.  Extra keyword
    arguments are ignored, as in the reference.  torch.sort on the device, the overlap kernel through the sort's indices, one
    decision launch, idx[keep]; no (M, M) matrix reaches the host.  The decision is the reference's float32 arithmetic operation
    for operation (include/mi_mask_sets.h states it), its quirks included: the lower inner test also sees the pair (c-1, c)
    (torch.tril(..., diagonal=1) at :164), and of two empty masks the lower-scored one is dropped (0/0 union).

    Where this differs from the reference:
      * the fallbacks (:173-181).  When no score passes score_thr, or every upper inner test fails, or every lower inner test
        fails, the reference means to switch that one test on for the three best-scored masks, but its keep_conf[index, 0] raises
        IndexError on the 1-D tensor it has (RuntimeError for M < 3).  Here the intent is built: that test is set true for the
        first min(3, M) masks of the sorted order.
      * ties in `scores` are ordered by a stable sort; the reference's order is unspecified there."""
    f32("mask_nms", "scores", scores)
    iou_thr, score_thr = number("mask_nms", "iou_thr", iou_thr), number("mask_nms", "score_thr", score_thr)
    inner_max = 1.0 - number("mask_nms", "inner_thr", inner_thr)   # :169-170 subtract in Python doubles; the comparison is in float32
    packed = _packed(masks, scores, "mask_nms")
    M, dev = packed.shape[0], scores.device
    if tuple(scores.shape) != (M,):
        raise ValueError(f"mask_nms: scores must be ({M},) for {M} masks, got {tuple(scores.shape)}")
    s, idx = torch.sort(scores.detach(), dim=0, descending=True, stable=True)
    inter, areas = _overlaps(packed, idx)
    keep = torch.empty((M,), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        check(_lib.load().mi_mask_nms_keep(M, inter.data_ptr(), areas.data_ptr(), s.data_ptr(), iou_thr, score_thr, inner_max,
                                           keep.data_ptr(), stream_ptr(dev)))
    return idx[keep.bool()]


def masks_update(*levels, **kwargs):
    """clip_utils/sam_utils.py:189-202: removes redundant masks from each of SAM's mask lists (lists of dicts with 'segmentation',
    'predicted_iou', 'stability_score'), by mask_nms with scores = stability_score * predicted_iou (in float32).  Returns a tuple
    of the filtered lists, each in its original order; the keyword arguments go to mask_nms.  Runs on the current GPU.  An empty
    list stays empty."""
    import numpy as np
    dev = torch.device("cuda", torch.cuda.current_device())
    out = ()
    for lvl in levels:
        if len(lvl) == 0:
            out += ([],)
            continue
        seg = torch.from_numpy(np.stack([np.asarray(m["segmentation"], dtype=bool) for m in lvl], axis=0))
        iou_pred = np.stack([m["predicted_iou"] for m in lvl], axis=0)
        stability = np.stack([m["stability_score"] for m in lvl], axis=0)
        scores = torch.as_tensor(stability * iou_pred, dtype=torch.float32).to(dev)
        kept = set(mask_nms(seg.to(dev), scores, **kwargs).tolist())
        out += ([m for i, m in enumerate(lvl) if i in kept],)
    return out


def mask_score_images(scores, masks, mode: str = "mean", out=None):
    """Per-mask scores painted into score images: (K, h, w) float32, the input of lift_scores / vote_3d_mask as it is.

    scores: (M,) or (M, K) float32 on a GPU, finite (clip_relevancy's result); masks: bool (M, h, w) on the CPU or the scores'
    GPU, or a PackedSamMasks there.  Per pixel p and column k, over the masks m that cover p, in ascending m, with a float32
    accumulator:
      "sum"  : the sum of scores[m, k]                                          (get_multi_lvl_scores, clip_utils/__init__.py:380)
      "mean" : that sum / the number of covering masks, 0 where none covers p    (get_segmentation, :282: in float32 count + 1e-9
               is count, and 0 / 1e-9 is 0)
      "max"  : max over all M masks of scores[m, k] * bit_m(p): a mask that does not cover p contributes 0   (get_scores, :206)
    out: an optional contiguous float32 (K, h, w) tensor on that GPU to write into.  Deterministic: no atomics."""
    f32("mask_score_images", "scores", scores)
    if mode not in _lib.MI_MASK_SCORE_MODE:
        raise ValueError(f"mask_score_images: mode must be one of {sorted(_lib.MI_MASK_SCORE_MODE)}, got {mode!r}")
    if scores.dim() not in (1, 2):
        raise ValueError(f"mask_score_images: scores must be (M,) or (M, K), got {tuple(scores.shape)}")
    K = 1 if scores.dim() == 1 else int(scores.shape[1])
    if not 1 <= K <= MAX_SCORE_COLUMNS:
        raise ValueError(f"mask_score_images: need 1 <= K <= {MAX_SCORE_COLUMNS} score columns, got {K}")
    packed = _packed(masks, scores, "mask_score_images")
    M, h, w = packed.shape
    dev = scores.device
    if int(scores.shape[0]) != M:
        raise ValueError(f"mask_score_images: {int(scores.shape[0])} score rows for {M} masks")
    if out is None:
        out = torch.empty((K, h, w), device=dev, dtype=torch.float32)
    else:
        check_out("mask_score_images", out, (K, h, w), torch.float32, dev)
    s = scores.detach().contiguous()
    with torch.cuda.device(dev):
        check(_lib.load().mi_mask_score_images(M, h, w, K, packed.words.data_ptr(), s.data_ptr(), _lib.MI_MASK_SCORE_MODE[mode],
                                               out.data_ptr(), stream_ptr(dev)))
    return out


def resize_sam_masks(masks, size, threshold=0.5) -> PackedSamMasks:
    """clip_utils/__init__.py:99-102: the masks at another size.  Bit (y, x) of the result is
    F.interpolate(masks.float(), size, mode='bilinear')[m, y, x] > threshold, the value being PyTorch's CPU bilinear of four source
    bits, bit for bit (the taps and the rounding order of erode_sam_masks' resampled branch).

    masks: bool (M, h, w) on the CPU or a GPU (packed here), or a PackedSamMasks; size: (H, W) with H * W < 2^24.  Returns a
    PackedSamMasks (M, H, ceil(W / 64)) on the masks' GPU (the current one for CPU masks), padding bits 0.  At the same size the
    value is the bit itself, so the result is a copy for 0 <= threshold < 1.  One launch."""
    H, W = size_hw("resize_sam_masks", size)
    if H * W >= MAX_PIXELS:
        raise ValueError(f"resize_sam_masks: need H * W < 2^24 pixels, got {H} x {W}")
    threshold = number("resize_sam_masks", "threshold", threshold)
    packed = _packed(masks, None, "resize_sam_masks")
    M, h, w = packed.shape
    dev = packed.device
    out = torch.empty((M, H, row_words(W)), device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        check(_lib.load().mi_mask_resize(M, h, w, packed.words.data_ptr(), H, W, threshold, out.data_ptr(), stream_ptr(dev)))
    return PackedSamMasks(out, (M, H, W))


def mask_index_map(masks, offset: int = 0, out=None) -> torch.Tensor:
    """The seg_map of clip_utils/sam_utils.py:214 and :221 (mask2segmap): (h, w) int32, per pixel `offset` + the highest index of
    a mask that covers it -- the reference paints the masks in ascending order, so the last one stays -- and -1, without the offset,
    where no mask covers the pixel (:62 adds the cumulated lengths of the earlier levels to every value but -1).

    masks: bool (M, h, w) on the CPU or a GPU, or a PackedSamMasks; 0 <= offset <= 2^31 - 1025; out: an optional contiguous int32
    (h, w) tensor on the masks' GPU to write into.  One launch that reads the mask words once.  Exact."""
    if isinstance(offset, bool) or not isinstance(offset, int) or not 0 <= offset <= (1 << 31) - 1 - MAX_MASKS:
        raise ValueError(f"mask_index_map: offset must be an int in 0 .. 2^31 - 1 - {MAX_MASKS}, got {offset!r}")
    packed = _packed(masks, None, "mask_index_map")
    M, h, w = packed.shape
    dev = packed.device
    if out is None:
        out = torch.empty((h, w), device=dev, dtype=torch.int32)
    else:
        check_out("mask_index_map", out, (h, w), torch.int32, dev)
    with torch.cuda.device(dev):
        check(_lib.load().mi_mask_index_map(M, h, w, packed.words.data_ptr(), offset, out.data_ptr(), stream_ptr(dev)))
    return out
