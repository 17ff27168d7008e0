"""GPU tests of the photometric loss (seganygaussians_amd/photometric.py) against the float64 restatement
(tests/photometric_ref.py, pinned to the reference by tests/test_photometric_host.py).

The tolerance is measured per input, not fixed: E32 = |float32 restatement - float64 restatement| on that very input, and the
product must satisfy |product - f64| <= max(4 E32, floor), floor = 2^-22 max(1, |value|) for a scalar and 2^-22 max |gradient64| for a
gradient (ref.FACTOR, ref.FLOOR).  Every test prints `error / bound` per quantity."""
import os

import numpy as np
import pytest
import torch

import seganygaussians_amd
from seganygaussians_amd import photometric as ph
from tests import helpers as hp
from tests import photometric_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH, TW = ph.TILE_H, ph.TILE_W


def _eval_ref(fn, x, g, dtype):
    """(value, d sum(value) / dx) of fn(x, g) evaluated in dtype on the CPU, as float64."""
    xd = x.detach().cpu().to(dtype).requires_grad_(True)
    v = fn(xd, g.detach().cpu().to(dtype))
    v.sum().backward()
    return v.detach().double(), xd.grad.double()


def _eval_gpu(fn, x, g):
    xd = x.detach().to(DEV).requires_grad_(True)
    v = fn(xd, g.to(DEV))
    v.sum().backward()
    assert v.dtype == torch.float32 and xd.grad.dtype == torch.float32 and xd.grad.shape == xd.shape
    return v.detach().double().cpu(), xd.grad.double().cpu()


def _bound(v32, v64, scalar):
    e32 = (v32 - v64).abs().max().item()
    scale = max(1.0, v64.abs().max().item()) if scalar else v64.abs().max().item()
    return max(ref.FACTOR * e32, ref.FLOOR * scale)


def _check_one(label, fn_gpu, fn_ref, x, g):
    """Value and gradient of one entry point under the rule; returns the two error / bound ratios."""
    v64, g64 = _eval_ref(fn_ref, x, g, torch.float64)
    v32, g32 = _eval_ref(fn_ref, x, g, torch.float32)
    v, gr = _eval_gpu(fn_gpu, x, g)
    assert v.shape == v64.shape, (label, v.shape, v64.shape)
    bv, bg = _bound(v32, v64, True), _bound(g32, g64, False)
    ev, eg = (v - v64).abs().max().item(), (gr - g64).abs().max().item()
    print(f"{label}: value {ev:.3e} / {bv:.3e} = {ev / bv:.3f}   gradient {eg:.3e} / {bg:.3e} = {eg / max(bg, 1e-300):.3f}")
    assert ev <= bv, (label, "value", ev, bv)
    assert eg <= bg, (label, "gradient", eg, bg)
    return ev / bv, eg / max(bg, 1e-300)


def _check_all(label, x, g, lam=0.2):
    _check_one(f"{label} loss(lambda={lam})", lambda a, b: ph.photometric_loss(a, b, lam), lambda a, b: ref.loss(a, b, lam), x, g)
    _check_one(f"{label} ssim", ph.ssim, ref.ssim, x, g)
    _check_one(f"{label} l1_loss", ph.l1_loss, ref.l1, x, g)
    if x.dim() == 4:
        _check_one(f"{label} ssim(size_average=False)", lambda a, b: ph.ssim(a, b, 11, False), lambda a, b: ref.ssim(a, b, False), x, g)
    # the detached parts
    with torch.no_grad():
        loss, l1, ss = ph.photometric_loss(x.to(DEV), g.to(DEV), lam, return_parts=True)
        assert loss.dim() == 0 and not l1.requires_grad and not ss.requires_grad
        assert torch.equal(l1, ph.l1_loss(x.to(DEV), g.to(DEV))) and torch.equal(ss, ph.ssim(x.to(DEV), g.to(DEV)))


Z = np.load(os.path.join(ROOT, "tests", "golden", "photometric", "photometric.npz"))


@pytest.mark.parametrize("name", [str(n) for n in Z["names"]])
def test_fixture_inputs(name):
    x, g = torch.from_numpy(Z[f"{name}.image"]), torch.from_numpy(Z[f"{name}.target"])
    _check_all(name, x, g, float(Z["lambda_dssim"]))
    if np.array_equal(Z[f"{name}.image"], Z[f"{name}.target"]):
        xd = x.to(DEV).requires_grad_(True)
        loss, l1, ss = ph.photometric_loss(xd, g.to(DEV), return_parts=True)
        loss.backward()
        assert ss.item() == 1.0 and l1.item() == 0.0 and loss.item() == 0.0 and not xd.grad.any()


SIZES = [(1, 1, 1), (1, 1, 150), (1, 90, 1), (1, 10, 10), (1, 11, 11), (1, TH - 1, TW - 1), (1, TH, TW), (1, TH + 1, TW + 1),
         (2, TH - 1, TW + 1), (3, TH + 1, TW - 1), (1, 2 * TH, 2 * TW), (2, 1, 37, 53), (2, 3, 2 * TH + 3, TW + 9)]


@pytest.mark.parametrize("shape", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_sizes_that_exercise_the_tiling(shape):
    x, g = ref.make_pair("noise", shape, seed=100 + sum(shape))
    _check_all("x".join(map(str, shape)), x, g)


@pytest.mark.parametrize("lam", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("kind", ref.CLASSES)
def test_input_classes_and_lambdas(kind, lam):
    x, g = ref.make_pair(kind, (3, 2 * TH + 6, 2 * TW + 22), seed=7)
    _check_one(f"{kind} loss(lambda={lam})", lambda a, b: ph.photometric_loss(a, b, lam), lambda a, b: ref.loss(a, b, lam), x, g)


@pytest.mark.parametrize("kind", ref.CLASSES)
def test_full_hd(kind):
    x, g = ref.make_pair(kind, (3, 1080, 1920), seed=11)
    _check_one(f"1080p {kind} loss", ph.photometric_loss, ref.loss, x, g)
    if kind == "noise":
        _check_one(f"1080p {kind} ssim", ph.ssim, ref.ssim, x, g)
        _check_one(f"1080p {kind} l1_loss", ph.l1_loss, ref.l1, x, g)


def test_incoming_gradient_scales_the_gradient():
    x, g = ref.make_pair("noise", (3, 45, 83), seed=21)
    other = torch.linspace(-1.0, 1.0, x.numel()).reshape(x.shape)
    _check_one("2.5 * loss", lambda a, b: 2.5 * ph.photometric_loss(a, b), lambda a, b: 2.5 * ref.loss(a, b), x, g)
    _check_one("loss + other term", lambda a, b: ph.photometric_loss(a, b) + 0.5 * (a * other.to(a.device)).sum() + 3.0 * ph.l1_loss(a, b),
               lambda a, b: ref.loss(a, b) + 0.5 * (a * other.to(a.dtype)).sum() + 3.0 * ref.l1(a, b), x, g)
    x4, g4 = ref.make_pair("smooth", (2, 3, 37, 70), seed=22)
    wts = torch.tensor([0.25, -1.5])
    _check_one("weighted per-image ssim", lambda a, b: (ph.ssim(a, b, 11, False) * wts.to(a.device)).sum(),
               lambda a, b: (ref.ssim(a, b, False) * wts.to(a.dtype)).sum(), x4, g4)


def _run(x, g):
    xd = x.detach().clone().requires_grad_(True)
    loss = ph.photometric_loss(xd, g)
    loss.backward()
    return loss.detach(), xd.grad


def test_deterministic():
    x, g = (t.to(DEV) for t in ref.make_pair("noise", (3, 300, 500), seed=31))
    l0, g0 = _run(x, g)
    for _ in range(2):
        l1, g1 = _run(x, g)
        assert torch.equal(l0, l1) and torch.equal(g0, g1)


def test_loss_is_the_combination_of_its_parts():
    lam = 0.2
    x, g = ref.make_pair("smooth", (3, 70, 150), seed=41)
    v64, g64 = _eval_ref(lambda a, b: ref.loss(a, b, lam), x, g, torch.float64)
    v32, g32 = _eval_ref(lambda a, b: ref.loss(a, b, lam), x, g, torch.float32)
    va, ga = _eval_gpu(lambda a, b: ph.photometric_loss(a, b, lam), x, g)
    vb, gb = _eval_gpu(lambda a, b: (1.0 - lam) * ph.l1_loss(a, b) + lam * (1.0 - ph.ssim(a, b)), x, g)
    bv, bg = _bound(v32, v64, True), _bound(g32, g64, False)
    print(f"fused vs composed: value {(va - vb).abs().item():.3e} / {bv:.3e}   gradient {(ga - gb).abs().max().item():.3e} / {bg:.3e}")
    assert (va - vb).abs().item() <= bv and (ga - gb).abs().max().item() <= bg


def test_side_stream_and_non_contiguous_image():
    x, g = (t.to(DEV) for t in ref.make_pair("noise", (3, 200, 333), seed=51))
    l0, g0 = _run(x, g)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        l1, g1 = _run(x, g)
    side.synchronize()
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    # an (H, W, C) leaf seen as (C, H, W): accepted, and the gradient arrives in the leaf's own layout
    hwc = x.permute(1, 2, 0).contiguous().requires_grad_(True)
    view = hwc.permute(2, 0, 1)
    assert not view.is_contiguous()
    ph.photometric_loss(view, g).backward()
    assert hwc.grad.shape == hwc.shape and torch.equal(hwc.grad.permute(2, 0, 1), g0)
    gt_view = g.permute(1, 2, 0).contiguous().permute(2, 0, 1)
    assert torch.equal(ph.photometric_loss(x, gt_view), l0)


def test_one_rgb_training_step_through_the_rasterizer():
    """train_scene.py's step: render with SH colours, loss against a target, backward into the Gaussians; the fused loss against the
    float32 restatement on the device."""
    seganygaussians_amd.install_dropin()
    import diff_gaussian_rasterization as mod
    inp = hp.make_inputs(6000, 208, 144, 3, seed=61, with_shs=True, sh_degree=3, bg="random")
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(DEV)
    settings = mod.GaussianRasterizationSettings(
        image_height=inp.image_height, image_width=inp.image_width, tanfovx=inp.tanfovx, tanfovy=inp.tanfovy, bg=t(inp.bg),
        scale_modifier=inp.scale_modifier, viewmatrix=t(inp.viewmatrix), projmatrix=t(inp.projmatrix), sh_degree=inp.sh_degree,
        campos=t(inp.campos), prefiltered=False, debug=False)

    def step(loss_fn, target=None):
        leaves = {k: t(v).requires_grad_(True) for k, v in (("means3D", inp.means3D), ("shs", inp.shs), ("opacities", inp.opacities))}
        means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
        color, _ = mod.GaussianRasterizer(raster_settings=settings)(
            means3D=leaves["means3D"], means2D=means2D, shs=leaves["shs"], colors_precomp=None, opacities=leaves["opacities"],
            scales=t(inp.scales), rotations=t(inp.rotations), cov3D_precomp=None)
        if target is None:
            gen = torch.Generator().manual_seed(62)
            target = (color.detach().cpu() + 0.05 * torch.randn(color.shape, generator=gen)).clamp(0.0, 1.0).to(DEV)
        loss = loss_fn(color, target)
        loss.backward()
        return loss.detach(), {k: v.grad.cpu().numpy() for k, v in leaves.items()}, target

    loss_new, grads_new, target = step(lambda a, b: ph.photometric_loss(a, b, 0.2))
    loss_ref, grads_ref, _ = step(lambda a, b: ref.loss(a, b, 0.2), target)
    assert abs(loss_new.item() - loss_ref.item()) <= hp.RTOL * abs(loss_ref.item())
    for k in grads_ref:
        assert np.abs(grads_ref[k]).max() > 0
        frac = hp.assert_close(f"dL_d{k}", grads_new[k], grads_ref[k], rtol=hp.RTOL, flip_frac=hp.GRAD_FLIP_FRAC)
        print(f"dL_d{k}: fraction outside {frac:.2e}")


def _as_allocated(nbytes: int) -> int:
    """What PyTorch's caching allocator hands out for a request (c10 CachingAllocator: multiples of 512 bytes; requests of 10 MiB
    and more come from blocks rounded up to a multiple of 2 MiB, and a remainder of less than 1 MiB stays with the block)."""
    if nbytes >= 10 << 20:
        block = -(-nbytes // (2 << 20)) * (2 << 20)
        return block if block - nbytes < (1 << 20) else -(-nbytes // 512) * 512
    return -(-nbytes // 512) * 512


def test_extra_memory_is_what_the_design_states():
    """DESIGN.md section 17, design (a): between forward and backward the three derivative maps (one allocation); in the backward
    the gradient; the workspace (16 bytes per tile), the 5 output scalars and autograd's incoming scalar; nothing else of image
    size.  Each allocation counts as the framework's allocator hands it out."""
    C, H, W = 3, 1080, 1920
    x, g = (t.to(DEV) for t in ref.make_pair("noise", (C, H, W), seed=71))
    _run(x, g)                       # load the code objects and the allocator's small pools
    xd = x.detach().clone().requires_grad_(True)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    ph.photometric_loss(xd, g).backward()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(DEV) - base
    n = C * H * W * 4
    tiles = C * -(-H // TH) * -(-W // TW)
    stated = _as_allocated(3 * n) + _as_allocated(n) + _as_allocated(16 * tiles) + _as_allocated(4 * 5) + _as_allocated(4)
    print(f"extra {extra / 2 ** 20:.2f} MiB, stated {stated / 2 ** 20:.2f} MiB ({4 * n / 2 ** 20:.2f} MiB of maps and gradient as requested)")
    assert extra <= stated + (1 << 20)
