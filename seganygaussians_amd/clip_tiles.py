"""The CLIP network's input on the MI355X: one masked crop per SAM mask, resized and normalised.

The step between mask_nms and the CLIP image encoder in the open-vocabulary path.  The reference interpolates the masks to the
image's size, builds an (M, H, W, 3) float tensor of masked images on the CPU, slices one box per mask and calls the encoder M
times with batch 1, each call resizing and normalising on its own (clip_utils/__init__.py:91-191, clip_utils/clip_utils.py:60-68,
:201-203); clip_utils/sam_utils.py:99-114 and :212-225 do the same per mask on the host with a zero background, a centred pad to a
square and cv2.resize.  Here the masks stay bit-packed on the device (PackedSamMasks) and one launch reads the mask bits and the
uint8 image once per crop and writes the (M, 3, Sh, Sw) batch:

  * clip_tiles()                        -- the tiles and which of them are valid.
  * get_features_from_image_and_masks() -- the reference's function of that name on top of it: batched encoder calls.

The masks are brought to the image's size by sam_masks.resize_sam_masks(); the per-pixel seg_map of mask2segmap is
sam_masks.mask_index_map().  No autograd."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._args import check_out, number, size_hw
from ._ffi import check, stream_ptr
from .packed_masks import as_packed, check_shape
from .sam_masks import resize_sam_masks

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)   # clip_utils/clip_utils.py:64
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)   # clip_utils/clip_utils.py:65
MAX_SIZE = _lib.MI_CLIP_TILES_MAX_SIZE
MAX_SIDE = _lib.MI_CLIP_TILES_MAX_SIDE
_DEFAULT_BACKGROUND = {"crop": 1.0, "pad_square": 0.0}   # clip_utils/__init__.py:91, :108; sam_utils.py:101


def _triple(v, name: str):
    try:
        t = tuple(float(x) for x in v)
    except (TypeError, ValueError):
        t = ()
    if len(t) != 3 or any(x != x for x in t):
        raise ValueError(f"clip_tiles: {name} must be three numbers, got {v!r}")
    return (C.c_float * 3)(*t)


def clip_tiles(image, masks, size=(224, 224), layout: str = "crop", background=None, antialias: bool = True, mean=CLIP_MEAN,
               std=CLIP_STD, dtype=torch.float16, rects=None, inclusive: bool = False, out=None):
    """One masked crop of `image` per mask, resized to `size` and normalised: (tiles, valid).

    image: uint8 (H, W, 3), a numpy array, a CPU tensor or a tensor on the masks' GPU; host data is copied to that GPU once.
    masks: bool (M, H, W) on the CPU or a GPU, or a PackedSamMasks, at the image's size (sam_masks.resize_sam_masks brings them
    there).  tiles: (M, 3, Sh, Sw) in `dtype` (float16 or float32) on the masks' GPU; valid: (M,) bool there.

    The rectangle of mask m comes from masks_to_boxes on the device, without a host read: from the inclusive box (x_min, y_min,
    x_max, y_max) the crop is [x_min, x_max) x [y_min, y_max) -- the reference's slice, which drops the box's last row and column
    (clip_utils/__init__.py:157, :168; get_seg_img's w = x_max - x_min) -- or, with inclusive=True, the whole box.  `rects`
    overrides it: an (M, 4) int32 tensor of half-open [X0, Y0, X1, Y1) on the masks' GPU (SAM's own bbox, say); a rectangle may
    leave the image, and what lies outside reads as background.  valid[m] is false for a mask without a pixel and for a rectangle
    that is empty or longer than 32768 on a side (the reference raises there); such a tile holds the normalised background.

    Crop pixel (y, x), channel c: float32(image[Y0 + y, X0 + x, c]) / 255 where mask m has its bit, else
    bg = float32(float32(255 * background) / 255); background defaults to 1.0 for layout "crop" (:91) and 0.0 for "pad_square"
    (get_seg_img).  "crop" resizes the ch x cw crop; "pad_square" (pad_img) an L x L plane, L = max(ch, cw), with the crop at column
    (L - cw) // 2 when ch > cw, else at row (L - ch) // 2, the rest bg.  The resize is torchvision's Resize on a tensor,
    F.interpolate(mode='bilinear', align_corners=False, antialias=antialias), in the order of PyTorch's CPU kernels: width pass,
    then height pass, float32 (include/mi_clip_tiles.h states the weights).  Then (r - mean[c]) / std[c] in float32 and one
    rounding to `dtype`.  1 <= Sh, Sw <= 512.

    "pad_square" stands in for cv2.resize(pad_img(seg_img), (224, 224)) with antialias=False: the same geometry (half-pixel
    centres, INTER_LINEAR), but cv2 resamples uint8 with 11-bit fixed-point weights and rounds to uint8, while this resamples in
    float32.  cv2 is not available where this was written: the difference is unmeasured.

    out: an optional contiguous (M, 3, Sh, Sw) tensor of `dtype` on the masks' GPU to write into.  Deterministic: no atomics."""
    who = "clip_tiles"
    Sh, Sw = size_hw(who, size)
    if Sh > MAX_SIZE or Sw > MAX_SIZE:
        raise ValueError(f"{who}: need 1 <= Sh, Sw <= {MAX_SIZE}, got {(Sh, Sw)}")
    if layout not in _lib.MI_CLIP_TILES_LAYOUT:
        raise ValueError(f"{who}: layout must be one of {sorted(_lib.MI_CLIP_TILES_LAYOUT)}, got {layout!r}")
    if dtype not in (torch.float16, torch.float32):
        raise ValueError(f"{who}: dtype must be torch.float16 or torch.float32, got {dtype}")
    if background is None:
        background = _DEFAULT_BACKGROUND[layout]
    background = number(who, "background", background)
    bg = float(np.float32(np.float32(255.0 * background) / np.float32(255.0)))
    mean_c, std_c = _triple(mean, "mean"), _triple(std, "std")
    if any(s == 0.0 for s in std_c):
        raise ValueError(f"{who}: std must not be 0, got {std!r}")
    if isinstance(image, np.ndarray):
        image = torch.from_numpy(np.ascontiguousarray(image))
    if not isinstance(image, torch.Tensor) or image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
        raise ValueError(f"{who}: image must be uint8 (H, W, 3), got {getattr(image, 'dtype', type(image))} "
                         f"{tuple(getattr(image, 'shape', ()))}")
    H, W = int(image.shape[0]), int(image.shape[1])
    if tuple(int(v) for v in getattr(masks, "shape", ()))[1:] != (H, W):
        raise ValueError(f"{who}: the masks {tuple(getattr(masks, 'shape', ()))} are not at the image's size {(H, W)}; "
                         f"resize_sam_masks(masks, {(H, W)}) brings them there")
    check_shape(who, masks)
    packed = as_packed(who, masks, image.device if image.is_cuda else None, "image")   # CPU masks go to the image's GPU
    M = packed.shape[0]
    dev = packed.device
    if image.device != dev:
        image = image.to(dev)   # host data: one copy
    image = image.contiguous()
    if rects is not None:
        if not isinstance(rects, torch.Tensor) or rects.dtype != torch.int32 or tuple(rects.shape) != (M, 4):
            raise ValueError(f"{who}: rects must be an int32 ({M}, 4) tensor, got {getattr(rects, 'dtype', type(rects))} "
                             f"{tuple(getattr(rects, 'shape', ()))}")
        if rects.device != dev:
            raise ValueError(f"{who}: the masks are on {dev}, the rects on {rects.device}")
        if inclusive:
            raise ValueError(f"{who}: inclusive applies to the masks' own boxes; rects are half-open as given")
    if out is None:
        out = torch.empty((M, 3, Sh, Sw), device=dev, dtype=dtype)
    else:
        check_out(who, out, (M, 3, Sh, Sw), dtype, dev, dtype_name=str(dtype))
    L = _lib.load()
    boxes = torch.empty((M, 4), device=dev, dtype=torch.float32)
    areas = torch.empty((M,), device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        check(L.mi_mask_boxes(M, H, W, packed.words.data_ptr(), boxes.data_ptr(), areas.data_ptr(), stream_ptr(dev)))
    if rects is None:
        rects = torch.nan_to_num(boxes, nan=0.0).to(torch.int32)   # (x_min, y_min, x_max, y_max): the exclusive slice as it is
        if inclusive:
            rects[:, 2:] += 1
    side = rects[:, 2:].long() - rects[:, :2].long()
    valid = (areas > 0) & (side >= 1).all(dim=1) & (side <= MAX_SIDE).all(dim=1)
    rects = torch.where(valid[:, None], rects, torch.zeros_like(rects)).contiguous()   # an invalid mask: the empty rectangle
    with torch.cuda.device(dev):
        check(L.mi_mask_clip_tiles(M, H, W, packed.words.data_ptr(), image.data_ptr(), rects.data_ptr(),
                                   _lib.MI_CLIP_TILES_LAYOUT[layout], bg, 1 if antialias else 0, mean_c, std_c, Sh, Sw,
                                   1 if dtype == torch.float16 else 0, out.data_ptr(), stream_ptr(dev)))
    return out, valid


@torch.no_grad()
def get_features_from_image_and_masks(clip_model, image, masks, background=1., batch: int = 64, antialias: bool = True):
    """clip_utils/__init__.py:91-191 with the reference's name and first four arguments: the CLIP image features of every mask's
    crop, (M, D) on the CPU.

    clip_model: the reference's OpenCLIPNetwork (clip_model.model.encode_image is called; the resize and normalisation of
    clip_model.process, clip_utils/clip_utils.py:60-68, happen in clip_tiles); image: uint8 (H, W, 3), numpy or tensor; masks:
    (M, h, w) bool -- any other dtype counts as `!= 0`, which for the reference's 0 / 1 masks is its masks.float() -- or a
    PackedSamMasks; they are resized to the image (resize_sam_masks) if their size differs.  The encoder sees `batch` tiles per
    call where the reference makes M calls of one.  Rows of masks whose crop is empty are NaN (the reference raises there)."""
    if isinstance(masks, torch.Tensor) and masks.dtype != torch.bool:
        masks = masks != 0
    H, W = int(image.shape[0]), int(image.shape[1])
    if tuple(int(v) for v in masks.shape)[1:] != (H, W):
        masks = resize_sam_masks(masks, (H, W))
    batch = int(batch)
    if batch < 1:
        raise ValueError(f"get_features_from_image_and_masks: batch must be positive, got {batch}")
    tiles, valid = clip_tiles(image, masks, layout="crop", background=background, antialias=antialias)
    feats = torch.cat([clip_model.model.encode_image(tiles[i:i + batch]).cpu() for i in range(0, tiles.shape[0], batch)], dim=0)
    feats[~valid.cpu()] = float("nan")
    return feats
