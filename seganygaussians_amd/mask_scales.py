"""SAM-mask 3-D scales on the MI355X: mask erosion and the per-mask point spread.

Replaces get_scale.py:128-159, the offline step that writes cam.mask_scales for the contrastive loss (contrastive_loss.py).  Per
training view the reference moves the rendered depth to the CPU, back-projects every pixel, resamples the M SAM masks bilinearly to
the depth's size, erodes them (3x3 box sum >= 5) and takes (points[mask].std(dim=0) * 2).norm() per mask.  Here the masks stay
bit-packed on the device, in the PackedSamMasks layout the targets kernels read (pack_sam_masks):

  * erode_sam_masks() -- one launch.  At the same size the erosion is the bit-sliced count of the 3x3 window (>= 5: its majority);
    otherwise each window value is PyTorch's CPU bilinear interpolation of 4 source bits, summed in f32.  min_sum sets the threshold.
  * sam_mask_scales() -- the erosion, then per-tile f64 moments and a fixed-order reduction: counts exact, scales deterministic.

The reference's quirks are kept: x pairs the row index with W/2 and fx, y the column index with H/2 and fy;
pixels of depth 0 are points at the origin; a mask with fewer than 2 eroded pixels has scale NaN."""
from __future__ import annotations

import math

import torch

from ._args import f32, number, size_hw
from ._ffi import check, stream_ptr
from .packed_masks import MAX_MASKS, MAX_PIXELS, PackedSamMasks, as_packed, check_shape, pack_sam_masks, row_words  # noqa: F401


def erode(packed: PackedSamMasks, H: int, W: int, min_sum: float = 5.0) -> PackedSamMasks:
    from . import _lib
    L = _lib.load()
    M, h, w = packed.shape
    dev = packed.device
    if M * H * row_words(W) >= 1 << 31 or M * h * row_words(w) >= 1 << 31:
        raise ValueError("erode_sam_masks: more than 2^31 mask words")
    out = torch.empty((M, H, row_words(W)), device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        check(L.mi_mask_erode_min_sum(M, h, w, packed.words.data_ptr(), H, W, min_sum, out.data_ptr(), stream_ptr(dev)))
    return PackedSamMasks(out, (M, H, W))


def erode_sam_masks(masks, size, min_sum=5) -> PackedSamMasks:
    """get_scale.py:145-152: F.interpolate(masks[:, None], size, mode='bilinear', align_corners=False), conv2d with a 3x3 box of
    ones (zero padding) and >= min_sum (5 there; the notebook's language section has 2), bit-packed.

    masks: bool (M, h, w) on the CPU or a GPU (packed here), or a PackedSamMasks (padding bits 0, as pack_sam_masks writes them);
    size: the output (H, W).  Returns the eroded masks as a PackedSamMasks (M, H, ceil(W / 64)) on the masks' GPU (the current GPU
    for CPU masks), padding bits 0."""
    H, W = size_hw("erode_sam_masks", size)
    min_sum = number("erode_sam_masks", "min_sum", min_sum)
    packed = as_packed("erode_sam_masks", masks, None)
    return erode(packed, H, W, min_sum)


def sam_mask_scales(depth: torch.Tensor, masks, fovx: float, fovy: float, return_counts: bool = False):
    """get_scale.py:128-159 for one view: the 3-D scale of every SAM mask.

    depth: float32 (H, W), or (1, H, W) as the depth renderer returns it, on a GPU; any strides.  masks: bool (M, h, w) on the CPU
    or the depth's GPU, or a PackedSamMasks on the depth's GPU; they are resampled to (H, W) and eroded (erode_sam_masks).
    fovx, fovy: the field of view in radians (the reference passes cameras[0].FoVx / FoVy for every view).
    Returns scales (M,) float32 on the depth's device = 2 sqrt(var_x + var_y + var_z) of the eroded mask's points, unbiased, with
    points ((row - W/2) d / fx, (col - H/2) d / fy, d), fx = (W/2) / tan(fovx / 2), fy = (H/2) / tan(fovy / 2), as the reference
    pairs them; NaN for a mask with fewer than 2 eroded pixels.  With return_counts, also the eroded pixel counts (M,) int64.
    M = 1 follows the same formula (the reference's .squeeze() at :152 drops the mask axis there and breaks)."""
    from . import _lib
    f32("sam_mask_scales", "depth", depth)
    if depth.dim() == 3 and depth.shape[0] == 1:
        depth = depth[0]
    if depth.dim() != 2:
        raise ValueError(f"sam_mask_scales: depth must be (H, W) or (1, H, W), got {tuple(depth.shape)}")
    if not depth.is_cuda:
        raise ValueError(f"sam_mask_scales: depth must be on a GPU, got {depth.device}")
    H, W = (int(v) for v in depth.shape)
    if H < 1 or W < 1:
        raise ValueError(f"sam_mask_scales: empty depth {(H, W)}")
    fovx, fovy = float(fovx), float(fovy)
    if not (0.0 < fovx < math.pi and 0.0 < fovy < math.pi):
        raise ValueError(f"sam_mask_scales: need 0 < fovx, fovy < pi radians, got {(fovx, fovy)}")
    dev = depth.device
    packed = as_packed("sam_mask_scales", masks, dev)
    M = packed.shape[0]
    if M * H * row_words(W) >= 1 << 31:
        raise ValueError("sam_mask_scales: more than 2^31 mask words")
    # :138-139 in float64 (numpy's tan of the Python floats FoVx / FoVy)
    fx = (W / 2) / math.tan(fovx / 2)
    fy = (H / 2) / math.tan(fovy / 2)
    eroded = erode(packed, H, W)
    L = _lib.load()
    depth = depth.contiguous()
    ws = torch.empty((L.mi_mask_scales_workspace_bytes(M, H, W),), device=dev, dtype=torch.uint8)
    scales = torch.empty((M,), device=dev, dtype=torch.float32)
    counts = torch.empty((M,), device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        check(L.mi_mask_scales(M, H, W, eroded.words.data_ptr(), depth.data_ptr(), fx, fy, ws.data_ptr(), ws.numel(),
                               scales.data_ptr(), counts.data_ptr(), stream_ptr(dev)))
    return (scales, counts) if return_counts else scales
