"""The call helpers every host module uses on its way into the C-ABI library (include/*.h): return-code check, tensor ->
pointer, stream -> pointer.  PyTorch supplies the memory and the stream; nothing here loads the library before a call fails."""
from __future__ import annotations

import torch

from . import _lib


def check(rc):
    if rc != 0:
        raise RuntimeError(_lib.last_error())


def ptr(t):
    """None or an empty tensor -> NULL (the reference's convention for an absent argument); no other check."""
    return None if t is None or t.numel() == 0 else t.data_ptr()


def dev_ptr(t, name, device=None, dtype=torch.float32):
    """ptr() for a caller's tensor: refuses one that is not on the GPU, of another dtype or on another device than expected
    (CF/.../__init__.py:196-206 passes empty tensors for absent arguments; the library tests `!= nullptr`)."""
    if t is None or t.numel() == 0:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a GPU tensor (got {t.device}); the MI355X rasterizer has no CPU path")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype} (got {t.dtype})")
    if device is not None and t.device != device:
        raise RuntimeError(f"{name} is on {t.device}, expected {device}")
    return t.data_ptr()


def contig(t):
    return t if (t is None or t.numel() == 0) else t.contiguous()


def stream_ptr(device):
    return torch.cuda.current_stream(device).cuda_stream
