"""The antialiased render mode without a GPU: the flag bit and the Python switches, the float64 reference of tests/antialias_ref.py
(closed form, finite differences, the energy property), and the designed properties of the scenes tests/test_antialias.py runs."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from seganygaussians_amd import _lib
from seganygaussians_amd import rasterizer as R
from tests import antialias_ref as ar
from tests import raster_edge_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_bit_is_1024_and_disjoint():
    assert _lib.MI_RAST_ANTIALIAS == 1024
    others = ("FULL_LISTS", "F32_BLEND", "NO_CULL", "FAST_EXP", "VERIFY_LISTS", "TILE_FWD", "PREZERO_BWD", "EXACT_EXP", "EQUAL_RUNS",
              "BWD_FEATURES_ONLY")
    for name in others:
        bit = getattr(_lib, "MI_RAST_" + name)
        assert bit & (bit - 1) == 0 and bit & _lib.MI_RAST_ANTIALIAS == 0, name


def test_forward_flags_sets_and_restores_the_bit():
    before = R._opts.call_flags()
    assert before & _lib.MI_RAST_ANTIALIAS == 0
    with R.forward_flags(antialiasing=True, exact_exp=True):
        assert R._opts.call_flags() & _lib.MI_RAST_ANTIALIAS
        with R.forward_flags(full_lists=True):                 # a bit it is not given stays
            assert R._opts.call_flags() & _lib.MI_RAST_ANTIALIAS
        with R.forward_flags(antialiasing=False):
            assert R._opts.call_flags() & _lib.MI_RAST_ANTIALIAS == 0
            assert R._opts.call_flags() & _lib.MI_RAST_EXACT_EXP
        assert R._opts.call_flags() & _lib.MI_RAST_ANTIALIAS
    assert R._opts.call_flags() == before


def test_enable_antialiasing_is_process_wide_and_returns_the_previous_setting():
    assert R.antialiasing_enabled() is False
    assert R.enable_antialiasing() is False
    try:
        assert R.antialiasing_enabled() is True
        assert R._opts.call_flags() & _lib.MI_RAST_ANTIALIAS
        assert R._opts.flags & _lib.MI_RAST_ANTIALIAS == 0     # the thread's own flags are not touched
    finally:
        assert R.enable_antialiasing(False) is True
    assert R._opts.call_flags() & _lib.MI_RAST_ANTIALIAS == 0


@pytest.mark.parametrize("value,want", [("1", True), ("0", False), ("", False)])
def test_environment_variable(value, want):
    env = dict(os.environ, MI_RAST_ANTIALIASING=value)
    out = subprocess.check_output([sys.executable, "-c", "from seganygaussians_amd import rasterizer as R; "
                                   "print(R.antialiasing_enabled(), bool(R._opts.call_flags() & 1024))"], env=env, cwd=ROOT, text=True)
    assert out.split() == [str(want), str(want)]


@pytest.mark.parametrize("s2", [0.01, 0.3, 3.0, 40.0])
def test_isotropic_closed_form(s2):
    """An isotropic 2-D variance s^2 on the optical axis: h = s^2 / (s^2 + 0.3)."""
    inp = ar.known_answer_inputs(s2)
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    s = t(np.full((1, 3), math.sqrt(s2) * 4.0 / 16.0))     # the float64 value, not the float32 one of the inputs
    h = ar.h_factor(t(inp.means3D), t(inp.viewmatrix), 32, 32, inp.tanfovx, inp.tanfovy, scales=s, rotations=t(inp.rotations))
    assert abs(float(h[0]) - s2 / (s2 + 0.3)) <= 1e-13


def test_float64_gradient_against_central_differences():
    """h of the reference on 8 Gaussians of the scene (the floored needle and a clamped centre among them): autograd against
    central differences in means3D, scales and rotations."""
    _, inp = ar.aa_scene("c32")
    idx = [inp.classes.index(c) for c in ("aa_subpixel", "aa_large", "aa_needle", "aa_clamped", "unnorm_quat", "tile_corner", "pixel_centre", "fill")]
    t = lambda a, g=False: torch.tensor(np.asarray(a, np.float64)[idx], requires_grad=g)
    m, s, q = t(inp.means3D, True), t(inp.scales, True), t(inp.rotations, True)
    view = torch.tensor(np.asarray(inp.viewmatrix, np.float64))
    f = lambda m_, s_, q_: ar.h_factor(m_, view, inp.image_width, inp.image_height, inp.tanfovx, inp.tanfovy, scales=s_, rotations=q_,
                                       scale_modifier=inp.scale_modifier)
    wgt = torch.tensor(np.linspace(0.5, 1.5, len(idx)))
    grads = torch.autograd.grad((f(m, s, q) * wgt).sum(), [m, s, q])
    clamped = 3
    for k, (x, g) in enumerate(zip((m, s, q), grads)):
        for i in range(len(idx)):
            for j in range(x.shape[1]):
                if k == 0 and i == clamped:
                    continue     # the quirk: a clamped t.x is detached, the reference's value is not the derivative there
                eps = 1e-6 * max(1e-3, abs(float(x[i, j].detach())))
                args = [m.detach().clone(), s.detach().clone(), q.detach().clone()]
                args[k][i, j] += eps
                up = float((f(*args) * wgt).sum())
                args[k][i, j] -= 2 * eps
                dn = float((f(*args) * wgt).sum())
                fd = (up - dn) / (2 * eps)
                noise = 4 * 2.0 ** -52 * abs(up) / eps      # rounding of the two sums of 8 values of h
                assert abs(fd - float(g[i, j])) <= 1e-5 * max(abs(fd), abs(float(g[i, j]))) + noise, (k, i, j, fd, float(g[i, j]))
    needle = 2
    assert all(float(g[needle].abs().max()) == 0.0 for g in grads)


@pytest.mark.parametrize("s2", [0.3, 3.0])
def test_energy_of_the_dense_reference(s2):
    """The pixel sum of a channel is 2 pi opacity s^2 with the mode and 2 pi opacity (s^2 + 0.3) without, each within 3 %: 1.1 % for
    the 3 sigma rect, at most 0.9 % for the alpha < 1/255 cut, 0.5 % for the sampling."""
    inp = ar.known_answer_inputs(s2)
    on, off = ar.dense_image(inp, True)[0].sum(), ar.dense_image(inp, False)[0].sum()
    assert abs(on / (2 * math.pi * 0.9 * s2) - 1) <= 0.03
    assert abs(off / (2 * math.pi * 0.9 * (s2 + 0.3)) - 1) <= 0.03
    assert abs(off / on - (s2 + 0.3) / s2) <= 0.03 * (s2 + 0.3) / s2


@pytest.mark.parametrize("cfg", list(ar.AA_CONFIGS))
def test_scene_properties(cfg):
    ref = ar.reference(cfg)
    inp = ref.inp
    cls = inp.classes
    i = {c: cls.index(c) for c in ("aa_subpixel", "aa_large", "aa_needle", "aa_faint", "aa_clamped")}
    assert inp.scale_modifier == 0.6
    assert (inp.image_width + 15) // 16 == 3 and (inp.image_height + 15) // 16 == 2
    for h in (ref.h64, ref.h32.astype(np.float64)):
        assert abs(h[i["aa_subpixel"]] - 0.1) < 0.005
        assert h[i["aa_large"]] > 0.99
        assert h[i["aa_needle"]] == np.float32(0.005) or abs(h[i["aa_needle"]] - 0.005) < 1e-9
    for rho in (ref.rho64, ref.rho32):
        assert rho[i["aa_needle"]] < 1e-6
        others = np.delete(np.arange(len(cls)), i["aa_needle"])
        assert (np.abs(rho[others] / ar.RHO_FLOOR - 1.0) > 1e-3).all()
    op = np.asarray(inp.opacities, np.float64).reshape(-1)
    assert op[i["aa_faint"]] > 1 / 255 > op[i["aa_faint"]] * ref.h64[i["aa_faint"]]
    assert abs(ref.dense["txtz"][i["aa_clamped"]]) > 1.3 * inp.tanfovx
    assert all(ref.radii[k] > 0 for k in i.values())
    np.testing.assert_array_equal(ref.radii, ref.radii32)
    np.testing.assert_array_equal(ref.radii, ref.fwd.radii)
    for name, table in (("dense64", ref.d64), ("dense32", ref.d32), ("oracle", ref.oracle)):
        for c in ref.classes:
            if c in er.PIXEL_CLASSES:
                continue
            assert np.abs(table[c][i["aa_faint"]]).max() == 0.0, (name, c, "aa_faint")
    # the h path of the floored needle is exactly zero in restatement (ii) (float32 autograd of h32; the float64 one: the finite-
    # difference test), while a Gaussian above the floor has one; its rows are not zero all the same: it is blended, the conic's path
    hp32 = ar.h_path32(inp)
    for k, g in hp32.items():
        assert np.abs(g[i["aa_needle"]]).max() == 0.0, (k, "aa_needle")
    assert any(np.abs(g[i["aa_subpixel"]]).max() > 0 for g in hp32.values())
    assert ref.rho32[i["aa_needle"]] <= ar.RHO_FLOOR and ref.rho64[i["aa_needle"]] <= ar.RHO_FLOOR
    assert np.abs(ref.d64["dL_dmeans2D"][i["aa_needle"]]).max() > 0
    designed = np.array([c != "fill" for c in cls])
    assert not (ref.excused_gaussians & designed).any(), [cls[k] for k in np.flatnonzero(ref.excused_gaussians & designed)]
    assert ref.excused_gaussians.sum() <= er.EXCUSED_GAUSSIANS and ref.excused_pixels.sum() <= er.EXCUSED_PIXELS


@pytest.mark.parametrize("cfg", list(ar.AA_CONFIGS))
def test_restatements_pass_the_rule_against_each_other(cfg):
    """The oracle judged by dense32's error and dense32 by the oracle's, with the undoubled pair of ar.AA_TABLE (er.MUTUAL but for
    dL_dsh, recalibrated)."""
    ref = ar.reference(cfg)
    worst = {}
    for c in ref.classes:
        f, fl = er.mutual_rule(c, "aa")
        for got, other in ((ref.oracle, "d32"), (ref.d32, "oracle")):
            r, zd = ref.ratios(c, got[c], f, fl, e32_from=(other,))
            worst[c] = max(worst.get(c, 0.0), float(r.max()))
            assert not zd.any(), (c, other, [ref.group_name(c, k) for k in np.flatnonzero(zd)])
    print("mutual error / bound: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
