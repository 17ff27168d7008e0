"""The 3DGS photometric loss restated for the tests (train_scene.py:101-104 with utils/loss_utils.py:17-63), dtype-generic and
differentiable by autograd.  tests/test_photometric_host.py pins it to recorded results of the reference's own functions
(tests/golden/photometric/photometric.npz); the GPU tests take its float64 evaluation as the truth and its float32 evaluation as
the yardstick of what float32 can deliver on a given input.

    loss = (1 - lambda) mean|x - g| + lambda (1 - mean ssim_map(x, g))

ssim_map: with W the 11 x 11 window below and conv = zero-padded (5) depthwise correlation,
    mu_x = conv(x), mu_g = conv(g), s_x = conv(x x) - mu_x^2, s_g = conv(g g) - mu_g^2, s_xg = conv(x g) - mu_x mu_g
    ssim_map = (2 mu_x mu_g + C1) (2 s_xg + C2) / ((mu_x^2 + mu_g^2 + C1) (s_x + s_g + C2)),  C1 = 0.01^2, C2 = 0.03^2

The window is part of the function: the 11 Gaussian taps (sigma 1.5) are rounded to float32, normalised in float32, their outer
product is rounded to float32 again, and only then converted to the images' dtype.  It is not renormalised at the border."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

WINDOW = 11
SIGMA = 1.5
C1 = 0.01 ** 2
C2 = 0.03 ** 2
FLOOR = 2.0 ** -22      # tolerance floor of the GPU tests, as a fraction of the quantity's scale
FACTOR = 4.0            # |product - f64| <= max(FACTOR * |f32 restatement - f64|, floor)


def taps() -> torch.Tensor:
    """The 11 one-dimensional weights, float32."""
    half = WINDOW // 2
    t = torch.tensor([math.exp(-((i - half) ** 2) / (2.0 * SIGMA ** 2)) for i in range(WINDOW)], dtype=torch.float32)
    return t / t.sum()


def window(dtype, device="cpu") -> torch.Tensor:
    t = taps()
    return torch.outer(t, t).to(device=device, dtype=dtype)


def _as4(a):
    if a.dim() == 3:
        return a[None]
    if a.dim() != 4:
        raise ValueError(f"(C, H, W) or (B, C, H, W), got {tuple(a.shape)}")
    return a


def ssim_map(x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """(B, C, H, W) map of the structural similarity of x and g (3-D inputs count as B = 1)."""
    x, g = _as4(x), _as4(g)
    ch = x.shape[1]
    w = window(x.dtype, x.device)[None, None].expand(ch, 1, WINDOW, WINDOW).contiguous()
    blur = lambda a: F.conv2d(a, w, padding=WINDOW // 2, groups=ch)
    mx, mg = blur(x), blur(g)
    sx = blur(x * x) - mx * mx
    sg = blur(g * g) - mg * mg
    sxg = blur(x * g) - mx * mg
    return ((2 * mx * mg + C1) * (2 * sxg + C2)) / ((mx * mx + mg * mg + C1) * (sx + sg + C2))


def ssim(x, g, size_average=True):
    m = ssim_map(x, g)
    return m.mean() if size_average else m.mean(dim=(1, 2, 3))


def l1(x, g):
    return (x - g).abs().mean()


def loss(x, g, lambda_dssim=0.2):
    return (1.0 - lambda_dssim) * l1(x, g) + lambda_dssim * (1.0 - ssim(x, g))


def evaluate(x: torch.Tensor, g: torch.Tensor, lambda_dssim: float, dtype, grad_scale: float = 1.0):
    """loss, l1, ssim, per-image ssim and d(grad_scale * loss)/dx, evaluated in `dtype` on x's device; returned as float64."""
    xd = x.detach().to(dtype).requires_grad_(True)
    gd = g.detach().to(dtype)
    val = loss(xd, gd, lambda_dssim)
    (grad_scale * val).backward()
    with torch.no_grad():
        return {"loss": val.detach().double(), "l1": l1(xd, gd).double(), "ssim": ssim(xd, gd).double(),
                "ssim_per_image": ssim(xd, gd, size_average=False).double(), "grad": xd.grad.double()}


def bounds(e32: dict, e64: dict) -> dict:
    """The tolerance rule of the GPU tests: per quantity max(FACTOR * |f32 restatement - f64|, floor), floor = 2^-22 of the
    quantity's scale (max(1, |value|) for a scalar, max |gradient| for the gradient)."""
    out = {}
    for k in ("loss", "l1", "ssim", "ssim_per_image"):
        err = (e32[k] - e64[k]).abs().max().item()
        out[k] = max(FACTOR * err, FLOOR * max(1.0, e64[k].abs().max().item()))
    out["grad"] = max(FACTOR * (e32["grad"] - e64["grad"]).abs().max().item(), FLOOR * e64["grad"].abs().max().item())
    return out


# ---- the input classes of the tests -----------------------------------------------------------------------------------------------
CLASSES = ("noise", "smooth", "constant", "zero")


def make_target(kind: str, shape, gen: torch.Generator) -> torch.Tensor:
    """float32 target of one of the four classes: uniform noise; 9 x 9 box-filtered noise; 0.7 + 1e-3 rand; all zero."""
    shape = tuple(shape)
    if kind == "noise":
        return torch.rand(shape, generator=gen)
    if kind == "smooth":
        n = torch.rand(shape, generator=gen)
        n4 = n.reshape((-1, 1) + shape[-2:])
        return F.avg_pool2d(F.pad(n4, (4, 4, 4, 4), mode="replicate"), 9, stride=1).reshape(shape).contiguous()
    if kind == "constant":
        return 0.7 + 1e-3 * torch.rand(shape, generator=gen)
    if kind == "zero":
        return torch.zeros(shape)
    raise ValueError(kind)


def make_pair(kind: str, shape, seed: int):
    """(image, target), float32 on the CPU: image = clamp(target + 0.05 N(0, 1), 0, 1)."""
    gen = torch.Generator().manual_seed(seed)
    g = make_target(kind, shape, gen)
    x = (g + 0.05 * torch.randn(tuple(shape), generator=gen)).clamp(0.0, 1.0)
    return x.contiguous(), g.contiguous()
