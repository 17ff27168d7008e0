"""The bit-packed SAM masks that the contrastive loss, the mask scales, the mask sets, the CLIP tiles and the vote graph share
(csrc/packed_masks.h): (M, H, ceil(W / 64)) 64-bit words on the device, bit x & 63 of word x >> 6 = pixel x of the row, padding
bits 0.  The container, the launch that packs bool masks, and the checks of a `masks` argument."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _lib
from ._ffi import check, stream_ptr

MAX_MASKS = _lib.MI_CONTRASTIVE_LOSS_MAX_MASKS
MAX_PIXELS = 1 << 24


def row_words(w: int) -> int:
    return (w + 63) // 64   # the 64-bit words of a row of w pixels


@dataclass
class PackedSamMasks:
    """Bit-packed SAM masks on the device: words (M, H, ceil(W / 64)) int64, bit b of word q = pixel 64 q + b."""
    words: torch.Tensor
    shape: tuple   # (M, H, W)

    @property
    def device(self):
        return self.words.device


def pack_sam_masks(masks: torch.Tensor, device=None) -> PackedSamMasks:
    """bool (M, H, W) masks (cam.original_masks), on the CPU or the device -> PackedSamMasks on `device` (default: the masks'
    device, or the current CUDA device for CPU masks).  One launch; a caller may keep the result per camera, which removes the
    per-iteration host-to-device copy of the masks."""
    if not isinstance(masks, torch.Tensor) or masks.dtype != torch.bool or masks.dim() != 3:
        raise ValueError(f"pack_sam_masks: need a bool (M, H, W) tensor, got "
                         f"{getattr(masks, 'dtype', type(masks))} {tuple(getattr(masks, 'shape', ()))}")
    M, H, W = (int(v) for v in masks.shape)
    if not 1 <= M <= MAX_MASKS or H < 1 or W < 1:
        raise ValueError(f"pack_sam_masks: need 1 <= M <= {MAX_MASKS} masks and a non-empty image, got {(M, H, W)}")
    dev = torch.device(device) if device is not None else (masks.device if masks.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    if dev.type != "cuda":
        raise ValueError(f"pack_sam_masks: the packed masks live on a GPU, not on {dev}")
    L = _lib.load()
    src = masks.to(dev).contiguous()
    words = torch.empty((M, H, row_words(W)), device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        check(L.mi_contrastive_pack_masks(M, H, W, src.data_ptr(), words.data_ptr(), stream_ptr(dev)))
    return PackedSamMasks(words, (M, H, W))


def mask_dims(who: str, masks) -> tuple:
    """(M, h, w) of a `masks` argument of either accepted type with 1 <= M <= MAX_MASKS: check_shape without the pixel limit."""
    if not isinstance(masks, PackedSamMasks) and not (isinstance(masks, torch.Tensor) and masks.dtype == torch.bool and masks.dim() == 3):
        raise ValueError(f"{who}: masks must be a bool (M, h, w) tensor or PackedSamMasks, got "
                         f"{getattr(masks, 'dtype', type(masks))} {tuple(getattr(masks, 'shape', ()))}")
    M, h, w = (int(v) for v in masks.shape)
    if not 1 <= M <= MAX_MASKS:
        raise ValueError(f"{who}: need 1 <= M <= {MAX_MASKS} masks, got {M}")
    return M, h, w


def check_shape(who: str, masks) -> None:
    """The limits of sam_masks.py and clip_tiles.py that need no device, before anything is packed or launched (the rest is
    as_packed's)."""
    M, h, w = mask_dims(who, masks)
    if h * w >= MAX_PIXELS:
        raise ValueError(f"{who}: need h * w < 2^24 pixels, got {h} x {w}")


def as_packed(who: str, masks, dev, versus: str = "depth") -> PackedSamMasks:
    """masks as a PackedSamMasks on the GPU dev (None: on their own GPU, or the current one for CPU masks).  versus names the
    tensor whose GPU dev is, for the message about masks that are elsewhere."""
    if isinstance(masks, PackedSamMasks):
        M, h, w = masks.shape
        words = masks.words
        if not 1 <= M <= MAX_MASKS or h < 1 or w < 1:
            raise ValueError(f"{who}: need 1 <= M <= {MAX_MASKS} masks and a non-empty image, got {(M, h, w)}")
        if words.dtype != torch.int64 or tuple(words.shape) != (M, h, row_words(w)) or not words.is_cuda:
            raise ValueError(f"{who}: PackedSamMasks words must be int64 ({M}, {h}, {row_words(w)}) on a GPU, got "
                             f"{words.dtype} {tuple(words.shape)} on {words.device}")
        if dev is not None and words.device != dev:
            raise ValueError(f"{who}: the masks are on {words.device}, the {versus} on {dev}")
        return PackedSamMasks(words.contiguous(), (M, h, w))
    if isinstance(masks, torch.Tensor):
        if masks.dtype != torch.bool or masks.dim() != 3:
            raise ValueError(f"{who}: masks must be a bool (M, h, w) tensor or PackedSamMasks, got {masks.dtype} {tuple(masks.shape)}")
        if masks.is_cuda and dev is not None and masks.device != dev:
            raise ValueError(f"{who}: the masks are on {masks.device}, the {versus} on {dev}")
        if not masks.is_cuda and masks.device.type != "cpu":
            raise ValueError(f"{who}: masks on {masks.device}; need the CPU or a GPU")
        return pack_sam_masks(masks, device=dev)   # checks M and the image size
    raise ValueError(f"{who}: masks must be a bool (M, h, w) tensor or PackedSamMasks, got {type(masks)}")
