"""CPU checks of the photometric loss: the restatement (tests/photometric_ref.py) against recorded results of the reference's own
utils/loss_utils.py in float64 and float32 (tests/golden/photometric/photometric.npz, made by
tests/golden/make_photometric_golden.py), autograd's gradcheck of the restatement, the argument checks of
seganygaussians_amd/photometric.py before any launch, and the exports.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from seganygaussians_amd import _lib, build
from seganygaussians_amd import photometric as ph
from tests import photometric_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "photometric", "photometric.npz")
Z = np.load(GOLDEN)
NAMES = [str(n) for n in Z["names"]]
LAMBDA = float(Z["lambda_dssim"])


def _case(name):
    return torch.from_numpy(Z[f"{name}.image"]), torch.from_numpy(Z[f"{name}.target"])


def test_fixture_covers_the_required_inputs():
    assert os.path.getsize(GOLDEN) < 512 * 1024
    shapes = {n: Z[f"{n}.image"].shape for n in NAMES}
    assert any(len(s) == 4 and s[0] == 2 for s in shapes.values())                       # B = 2
    assert {s[-3] for s in shapes.values()} >= {1, 3}                                    # C = 1 and C = 3
    assert any(s[-2] < 11 for s in shapes.values()) and any(s[-1] < 11 for s in shapes.values())
    assert any(not Z[f"{n}.target"].any() for n in NAMES)                                # an all-zero target
    assert any(np.array_equal(Z[f"{n}.image"], Z[f"{n}.target"]) for n in NAMES)         # image == target
    assert any(np.ptp(Z[f"{n}.target"]) <= 1e-3 and Z[f"{n}.target"].min() >= 0.7 for n in NAMES)   # nearly constant


@pytest.mark.parametrize("name", NAMES)
def test_float64_restatement_is_the_reference(name):
    x, g = _case(name)
    e = ref.evaluate(x, g, LAMBDA, torch.float64)
    for k in ("loss", "l1", "ssim"):
        want = float(Z[f"{name}.f64.{k}"])
        assert abs(e[k].item() - want) <= 1e-12 * abs(want), (k, e[k].item(), want)
    want = torch.from_numpy(Z[f"{name}.f64.grad"])
    # relative to the larger of the recorded gradient and the L1 term's magnitude 1 / N: with image == target the recorded gradient
    # is rounding residue of a sum that cancels, of no fixed value
    assert (e["grad"] - want).abs().max().item() <= 1e-12 * max(want.abs().max().item(), 1.0 / want.numel())
    if x.dim() == 4:
        want = torch.from_numpy(Z[f"{name}.f64.ssim_per_image"])
        assert ((e["ssim_per_image"] - want).abs() <= 1e-12 * want.abs()).all()
    if np.array_equal(Z[f"{name}.image"], Z[f"{name}.target"]):
        assert e["ssim"].item() == 1.0 and e["l1"].item() == 0.0


@pytest.mark.parametrize("name", NAMES)
def test_float32_restatement_within_the_rule_of_the_reference(name):
    """The float32 restatement against the float64 truth, bounded by the recorded float32 reference's own error under the rule the
    GPU tests apply to the product."""
    x, g = _case(name)
    e64 = ref.evaluate(x, g, LAMBDA, torch.float64)
    e32 = ref.evaluate(x, g, LAMBDA, torch.float32)
    rec = {k: torch.from_numpy(np.asarray(Z[f"{name}.f32.{k}"])).double() for k in ("loss", "l1", "ssim", "grad")}
    rec["ssim_per_image"] = torch.from_numpy(Z[f"{name}.f32.ssim_per_image"]).double() if x.dim() == 4 else e64["ssim_per_image"]
    bound = ref.bounds(rec, e64)
    for k in ("loss", "l1", "ssim", "grad"):
        err = (e32[k] - e64[k]).abs().max().item()
        print(f"{name} {k}: {err:.3e} / {bound[k]:.3e}")
        assert err <= bound[k], (k, err, bound[k])


def test_gradcheck_of_the_restatement():
    x, g = ref.make_pair("noise", (1, 6, 7), 11)
    x = x.double().requires_grad_(True)
    # |x - g| has a kink at 0; keep the image away from the target
    assert ((x - g.double()).abs() > 1e-4).all()
    assert torch.autograd.gradcheck(lambda a: ref.loss(a, g.double(), 0.2), (x,), eps=1e-6, atol=1e-8)
    assert torch.autograd.gradcheck(lambda a: ref.ssim(a[None], g.double()[None], size_average=False), (x,), eps=1e-6, atol=1e-8)


def test_window_taps_are_the_formula():
    build.build_library()
    L = _lib.load()
    taps = (ctypes.c_float * ph.WINDOW_SIZE)()
    excess = ctypes.c_double()
    L.mi_photo_loss_window(taps, ctypes.byref(excess))
    assert torch.equal(torch.tensor(list(taps), dtype=torch.float32), ref.taps())
    # the 2-D window of the function is the ROUNDED outer product; the kernels sum separably and correct for the difference of the sums
    t = ref.taps().double()
    want = (ref.window(torch.float64).sum() / torch.outer(t, t).sum() - 1.0).item()
    assert abs(want) > 1e-9 and abs(excess.value - want) <= 1e-6 * abs(want)


def test_bad_inputs_refused_before_any_launch():
    x, g = torch.zeros(3, 8, 9), torch.zeros(3, 8, 9)
    for fn in (ph.photometric_loss, ph.ssim, ph.l1_loss):
        with pytest.raises(ValueError, match="GPU"):
            fn(x, g)
        with pytest.raises(ValueError, match="float32"):
            fn(x.double(), g)
        with pytest.raises(ValueError, match="float32"):
            fn(x, g.half())
        with pytest.raises(ValueError, match="float32"):
            fn(x.numpy(), g)
        with pytest.raises(ValueError, match="shape mismatch"):
            fn(x, torch.zeros(3, 8, 8))
        with pytest.raises(ValueError, match=r"\(C, H, W\) or \(B, C, H, W\)"):
            fn(torch.zeros(8, 9), torch.zeros(8, 9))
        with pytest.raises(ValueError, match=r"\(C, H, W\) or \(B, C, H, W\)"):
            fn(torch.zeros(1, 1, 3, 8, 9), torch.zeros(1, 1, 3, 8, 9))
        with pytest.raises(ValueError, match="empty"):
            fn(torch.zeros(3, 0, 9), torch.zeros(3, 0, 9))
        with pytest.raises(ValueError, match="requires grad"):
            fn(x, g.clone().requires_grad_())
        with torch.no_grad(), pytest.raises(ValueError, match="GPU"):    # allowed with grad mode off; then the device check
            fn(x, g.clone().requires_grad_())
        big = torch.zeros(1).expand(2, 1 << 15, 1 << 15)                 # 2^31 elements, no storage behind them
        with pytest.raises(ValueError, match="2\\^31"):
            fn(big, big)
    with pytest.raises(ValueError, match="window_size"):
        ph.ssim(x, g, window_size=7)
    with pytest.raises(ValueError, match="size_average"):
        ph.ssim(x, g, size_average=False)
    with pytest.raises(ValueError, match="lambda_dssim"):
        ph.photometric_loss(x, g, lambda_dssim="much")
    with pytest.raises(ValueError, match="NaN"):
        ph.photometric_loss(x, g, lambda_dssim=float("nan"))
    meta = torch.zeros(3, 8, 9, device="meta")
    with pytest.raises(ValueError, match="GPU"):
        ph.photometric_loss(meta, meta)


def test_abi_exported_and_checks_arguments():
    build.build_library()
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "mi_photometric.h")).read()
    declared = set(re.findall(r"\b(mi_photo_[a-z_0-9]+)\s*\(", hdr.split("#ifndef")[1]))
    assert declared == {"mi_photo_loss_workspace_bytes", "mi_photo_loss_window", "mi_photo_loss_forward", "mi_photo_loss_backward"} <= set(_lib.ALL_EXPORTS)
    for name in declared:
        assert ctypes.cast(getattr(L, name), ctypes.c_void_p).value
    assert os.path.join(ROOT, "include", "mi_photometric.h") in build.HEADERS and "photometric.h" in build.SOURCES
    # 16 bytes per tile of TILE_H x TILE_W
    ws = L.mi_photo_loss_workspace_bytes
    assert ws(1, 1, 1) == 16 and ws(1, ph.TILE_H, ph.TILE_W) == 16
    assert ws(1, ph.TILE_H + 1, ph.TILE_W) == 32 and ws(1, ph.TILE_H, ph.TILE_W + 1) == 32
    assert ws(3, 1080, 1920) == 3 * 34 * 30 * 16
    assert ws(0, 4, 4) == 0 and ws(1, 0, 4) == 0 and ws(2, 1 << 15, 1 << 15) == 0
    assert (_lib.MI_PHOTO_L1, _lib.MI_PHOTO_SSIM, _lib.MI_PHOTO_WINDOW) == (ph._L1, ph._SSIM, ph.WINDOW_SIZE) == (1, 2, 11)
    # argument checks run before any launch: no device needed
    fwd, bwd = L.mi_photo_loss_forward, L.mi_photo_loss_backward
    assert fwd(0, 3, 4, 4, 8, 8, 0.2, 3, None, 8, 1 << 20, 8, None) != 0 and ">= 1" in _lib.last_error()
    assert fwd(2, 1, 1 << 15, 1 << 15, 8, 8, 0.2, 3, None, 8, 1 << 20, 8, None) != 0 and "2^31" in _lib.last_error()
    assert fwd(1, 3, 4, 4, None, 8, 0.2, 3, None, 8, 1 << 20, 8, None) != 0 and "null" in _lib.last_error()
    assert fwd(1, 3, 4, 4, 8, 8, 0.2, 3, None, 8, 1 << 20, None, None) != 0 and "null" in _lib.last_error()
    assert fwd(1, 3, 4, 4, 8, 8, 0.2, 0, None, 8, 1 << 20, 8, None) != 0 and "parts" in _lib.last_error()
    assert fwd(1, 3, 4, 4, 8, 8, 0.2, 1, 8, 8, 1 << 20, 8, None) != 0 and "MI_PHOTO_SSIM" in _lib.last_error()
    assert fwd(1, 3, 4, 4, 8, 8, float("nan"), 3, None, 8, 1 << 20, 8, None) != 0 and "NaN" in _lib.last_error()
    assert fwd(1, 3, 4, 4, 8, 8, 0.2, 3, None, 8, 47, 8, None) != 0 and "workspace" in _lib.last_error()
    assert bwd(1, 3, 0, 4, 8, 8, 8, 8, 0, 1.0, 1.0, 8, None) != 0 and ">= 1" in _lib.last_error()
    assert bwd(1, 3, 4, 4, 8, 8, 8, None, 0, 1.0, 1.0, 8, None) != 0 and "null" in _lib.last_error()
    assert bwd(1, 3, 4, 4, 8, 8, None, 8, 0, 1.0, 1.0, 8, None) != 0 and "maps" in _lib.last_error()
    assert bwd(1, 3, 4, 4, 8, 8, 8, 8, 0, float("nan"), 1.0, 8, None) != 0 and "NaN" in _lib.last_error()


def test_module_exports():
    assert callable(ph.photometric_loss) and callable(ph.ssim) and callable(ph.l1_loss)
    assert (ph.WINDOW_SIZE, ph.TILE_H, ph.TILE_W) == (11, 32, 64)
    hdr = open(os.path.join(ROOT, "include", "mi_photometric.h")).read()
    assert f"#define MI_PHOTO_TILE_H {ph.TILE_H}" in hdr and f"#define MI_PHOTO_TILE_W {ph.TILE_W}" in hdr
    assert f"#define MI_PHOTO_WINDOW {ph.WINDOW_SIZE}" in hdr
