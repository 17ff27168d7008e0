"""The 3DGS photometric loss on the MI355X: fused L1 + D-SSIM, forward and backward.

Replaces train_scene.py:101-102 with utils/loss_utils.py:17-63, the loss every iteration of the RGB-Gaussian training evaluates
behind the rasterizer:

    loss = (1 - lambda_dssim) * l1_loss(image, gt) + lambda_dssim * (1 - ssim(image, gt))

  * photometric_loss() -- the whole expression: one forward launch sequence (tile kernel + fixed-order reduction), one backward
    launch; the gradient it returns is the dL_dout_color the rasterizer's backward consumes.
  * ssim(), l1_loss()  -- the reference's names, argument order and return shapes, so that
    `from seganygaussians_amd.photometric import l1_loss, ssim` replaces train_scene.py:16.

float32 (C, H, W) or (B, C, H, W) tensors on one GPU, differentiable in the first argument only (the reference never differentiates
the target), once (no double backward).  The means are summed in float64 in a fixed order: results are bit-identical from run to
run.  No host synchronisation.  There is no CPU fallback."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._args import f32, number
from ._ffi import check, stream_ptr

WINDOW_SIZE = _lib.MI_PHOTO_WINDOW
TILE_H, TILE_W = _lib.MI_PHOTO_TILE_H, _lib.MI_PHOTO_TILE_W
_L1, _SSIM = _lib.MI_PHOTO_L1, _lib.MI_PHOTO_SSIM


def _prepare(who: str, image, gt, names=("image", "gt")):
    """Checks everything that can be checked without a device; returns (B, C, H, W).  Raises ValueError before any launch."""
    for name, t in zip(names, (image, gt)):
        f32(who, name, t)
    if image.dim() not in (3, 4):
        raise ValueError(f"{who}: {names[0]} must be (C, H, W) or (B, C, H, W), got {tuple(image.shape)}")
    if image.shape != gt.shape:
        raise ValueError(f"{who}: shape mismatch: {names[0]} {tuple(image.shape)}, {names[1]} {tuple(gt.shape)}")
    shape = tuple(int(v) for v in image.shape)
    B, (C, H, W) = (1, shape) if len(shape) == 3 else (shape[0], shape[1:])
    if min(B, C, H, W) < 1:
        raise ValueError(f"{who}: empty tensor {shape}")
    if B * C * H * W >= 1 << 31:
        raise ValueError(f"{who}: need fewer than 2^31 elements, got {B * C * H * W}")
    if torch.is_grad_enabled() and gt.requires_grad:
        raise ValueError(f"{who}: {names[1]} requires grad, and the loss is differentiated with respect to {names[0]} only; detach it")
    for name, t in zip(names, (image, gt)):
        if not t.is_cuda:
            raise ValueError(f"{who}: {name} must be on a GPU, got {t.device} (there is no CPU fallback)")
    if gt.device != image.device:
        raise ValueError(f"{who}: {names[1]} is on {gt.device}, {names[0]} on {image.device}")
    return B, C, H, W


def _forward(image, gt, dims, lambda_dssim: float, parts: int, want_maps: bool):
    """Launches the forward.  Returns (out, maps): out float32 (3 + 2 B,) = loss, l1, ssim, then per image l1, ssim."""
    L = _lib.load()
    B, C, H, W = dims
    dev = image.device
    out = torch.empty((3 + 2 * B,), device=dev, dtype=torch.float32)
    maps = torch.empty((3, B * C, H, W), device=dev, dtype=torch.float32) if want_maps else None
    ws = torch.empty((L.mi_photo_loss_workspace_bytes(B * C, H, W),), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        check(L.mi_photo_loss_forward(B, C, H, W, image.data_ptr(), gt.data_ptr(), float(lambda_dssim), parts,
                                      None if maps is None else maps.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), stream_ptr(dev)))
    return out, maps


def _backward(image, gt, maps, dims, grad_out, per_image: bool, w_l1: float, w_ssim: float):
    L = _lib.load()
    B, C, H, W = dims
    dev = image.device
    grad = torch.empty(image.shape, device=dev, dtype=torch.float32)
    grad_out = grad_out.to(torch.float32).contiguous()
    with torch.cuda.device(dev):
        check(L.mi_photo_loss_backward(B, C, H, W, image.data_ptr(), gt.data_ptr(), None if maps is None else maps.data_ptr(),
                                       grad_out.data_ptr(), 1 if per_image else 0, w_l1, w_ssim, grad.data_ptr(), stream_ptr(dev)))
    return grad


class _PhotometricLoss(torch.autograd.Function):
    """mode 0: (loss, l1, ssim); mode 1: ssim mean; mode 2: per-image ssim means; mode 3: l1 mean."""

    @staticmethod
    def forward(ctx, image, gt, dims, lambda_dssim, mode):
        image_c, gt_c = image.contiguous(), gt.contiguous()     # a non-contiguous input is copied once here
        need = ctx.needs_input_grad[0]
        parts = (_L1 | _SSIM, _SSIM, _SSIM, _L1)[mode]
        out, maps = _forward(image_c, gt_c, dims, lambda_dssim, parts, bool(need and parts & _SSIM))
        ctx.dims, ctx.lambda_dssim, ctx.mode = dims, lambda_dssim, mode
        if need:
            ctx.save_for_backward(image_c, gt_c, maps)
        if mode == 0:
            l1, ss = out[1], out[2]
            ctx.mark_non_differentiable(l1, ss)
            return out[0], l1, ss
        if mode == 1:
            return out[2]
        if mode == 2:
            return out[4::2]
        return out[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        image, gt, maps = ctx.saved_tensors
        B, C, H, W = ctx.dims
        g = grads[0]
        if ctx.mode == 0:
            n = float(B * C * H * W)
            grad = _backward(image, gt, maps, ctx.dims, g.reshape(1), False, (1.0 - ctx.lambda_dssim) / n, -ctx.lambda_dssim / n)
        elif ctx.mode == 1:
            grad = _backward(image, gt, maps, ctx.dims, g.reshape(1), False, 0.0, 1.0 / float(B * C * H * W))
        elif ctx.mode == 2:
            grad = _backward(image, gt, maps, ctx.dims, g.reshape(B), True, 0.0, 1.0 / float(C * H * W))
        else:
            grad = _backward(image, gt, None, ctx.dims, g.reshape(1), False, 1.0 / float(B * C * H * W), 0.0)
        return grad, None, None, None, None


def photometric_loss(image: torch.Tensor, gt: torch.Tensor, lambda_dssim: float = 0.2, return_parts: bool = False):
    """train_scene.py:101-102: (1 - lambda_dssim) * mean|image - gt| + lambda_dssim * (1 - mean ssim_map(image, gt)).

    image, gt: float32 (C, H, W) or (B, C, H, W) on one GPU; a non-contiguous tensor is copied once.  Returns the loss as a 0-dim
    float32 tensor, differentiable with respect to image; with return_parts also the detached Ll1 and ssim scalars
    (training_report logs Ll1).  The gradient is written in image's own layout by autograd."""
    lambda_dssim = number("photometric_loss", "lambda_dssim", lambda_dssim)
    dims = _prepare("photometric_loss", image, gt)
    loss, l1, ss = _PhotometricLoss.apply(image, gt.detach(), dims, lambda_dssim, 0)
    return (loss, l1, ss) if return_parts else loss


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True) -> torch.Tensor:
    """utils/loss_utils.py:33-63.  The mean of the SSIM map (0-dim), or with size_average=False the per-image means (B,) of a
    (B, C, H, W) input.  Differentiable in img1.  Only the reference's window of 11 is built."""
    if window_size != WINDOW_SIZE:
        raise ValueError(f"ssim: only window_size = {WINDOW_SIZE} is supported, got {window_size!r}")
    if not size_average and isinstance(img1, torch.Tensor) and img1.dim() != 4:
        raise ValueError(f"ssim: size_average=False needs a (B, C, H, W) input, got {tuple(img1.shape)}")   # the reference's mean(1) x 3
    dims = _prepare("ssim", img1, img2, names=("img1", "img2"))
    return _PhotometricLoss.apply(img1, img2.detach(), dims, 0.0, 1 if size_average else 2)


def l1_loss(network_output: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """utils/loss_utils.py:17-18: mean |network_output - gt| (0-dim), differentiable in network_output (sign(0) = 0)."""
    dims = _prepare("l1_loss", network_output, gt, names=("network_output", "gt"))
    return _PhotometricLoss.apply(network_output, gt.detach(), dims, 0.0, 3)
