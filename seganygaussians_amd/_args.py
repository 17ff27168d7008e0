"""The argument checks that two or more feature modules share, each written once.  Plain functions that raise ValueError with
the caller's name (`who`) in front; nothing here loads the library or needs a device."""
from __future__ import annotations

import torch


def to_float(who: str, name: str, value) -> float:
    try:
        return float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {name} must be a number, got {value!r}") from None


def number(who: str, name: str, value) -> float:
    """value as a float; refuses what float() refuses, and NaN."""
    v = to_float(who, name, value)
    if v != v:
        raise ValueError(f"{who}: {name} is NaN")
    return v


def f32(who: str, name: str, t, optional: bool = False):
    """Refuses what is not a float32 tensor (None passes where optional); returns t."""
    if t is None and optional:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise ValueError(f"{who}: {name} must be a float32 tensor{' or None' if optional else ''}, got {getattr(t, 'dtype', type(t))}")
    return t


def size_hw(who: str, size):
    """(H, W) as positive ints."""
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: size must be (H, W), got {size!r}") from None
    if H < 1 or W < 1:
        raise ValueError(f"{who}: size must be positive, got {(H, W)}")
    return H, W


def no_grad_one_gpu(who: str, tensors, versus: str = None):
    """The checks that come last, over (name, tensor) pairs: none requires grad while grad mode is on, all are on a GPU, all are on
    the GPU of the first, which is returned.  A tensor elsewhere "is on X, expected Y", or with versus, "is on X, the <versus> on Y"
    (the first tensor is then the one `versus` names)."""
    if torch.is_grad_enabled():
        for name, t in tensors:
            if t.requires_grad:
                raise ValueError(f"{who}: {name} requires grad and there is no backward; call under torch.no_grad() or detach it")
    dev = None
    for name, t in tensors:
        if not t.is_cuda:
            raise ValueError(f"{who}: {name} must be on a GPU, got {t.device} (there is no CPU fallback)")
        dev = t.device if dev is None else dev
        if t.device != dev:
            raise ValueError(f"{who}: {name} is on {t.device}, " + (f"expected {dev}" if versus is None else f"the {versus} on {dev}"))
    return dev


def check_out(who: str, out, shape, dtype, device, dtype_name: str = None) -> None:
    """A caller's `out` must be a contiguous tensor of this shape and dtype on this device.  dtype_name: how the message spells
    the dtype (default: without "torch.")."""
    if not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device \
            or not out.is_contiguous():
        dtype_name = dtype_name or str(dtype).replace("torch.", "")
        raise ValueError(f"{who}: out must be a contiguous {dtype_name} {tuple(shape)} tensor on {device}")
