"""Pins the CPU oracle against the independent dense float64 autograd re-derivation
(tests/dense_ref.py).  The reference has no golden vectors: this is pin (3) of
the oracle header -- forward image, radii and EVERY gradient the reference's backward returns
(CF/diff_gaussian_rasterization_contrastive_f/__init__.py:142-152) are checked.
"""
import math
import os

import numpy as np
import pytest
import torch

from oracle import saga_oracle as so
from seganygaussians_amd import scenes
from tests.dense_ref import render_dense

RTOL = 2e-4   # oracle forward is fp32, dense reference fp64


def _small_scene(P, W, H, C, seed, with_shs=False, focal=None, rotated=False):
    focal = focal or 0.9 * W
    sc = scenes.make_scene(P, W, H, focal, C, math.log(0.12), 0.5, seed=seed, with_shs=with_shs,
                           z_range=(1.0, 6.0))
    if rotated:
        cam = scenes.orbit_camera(W, H, focal, 0.25, 0.1)
        # recentre the cloud in front of the rotated camera
        sc.means3D[:, 2] += 1.0
    else:
        cam = scenes.look_at_camera(W, H, focal)
    return sc, cam


def _assert_close(name, got, want, rtol=RTOL, floor=1e-6, max_outlier_frac=0.0):
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(np.abs(want).max(), 1e-30)
    err = np.abs(got - want)
    tol = rtol * np.abs(want) + rtol * scale + floor * scale
    bad = err > tol
    frac = bad.mean() if bad.size else 0.0
    assert frac <= max_outlier_frac, f"{name}: {bad.sum()} / {bad.size} outside tol; max err {err.max():.3e} scale {scale:.3e}"


def _run(P, W, H, C, seed, *, with_shs=False, sh_degree=0, use_cov=False, use_mask=False, rotated=False,
         bg_val=0.0, scale_modifier=1.0):
    sc, cam = _small_scene(P, W, H, C, seed, with_shs=with_shs, rotated=rotated)
    rng = np.random.default_rng(seed + 100)
    bg = np.full(C, bg_val, np.float32) if bg_val == 0.0 else rng.uniform(0, 1, C).astype(np.float32)
    mask = rng.uniform(0, 1, P).astype(np.float32) if use_mask else None
    cov_pre = None
    if use_cov:
        # Sigma from scales/rotations computed in fp64, passed as precomputed 6-vector
        q = torch.tensor(sc.rotations, dtype=torch.float64)
        from tests.dense_ref import build_rotation
        R = build_rotation(q)
        S = torch.diag_embed(torch.tensor(sc.scales, dtype=torch.float64) * scale_modifier)
        Sig = (R @ S) @ (R @ S).transpose(1, 2)
        cov_pre = torch.stack([Sig[:, 0, 0], Sig[:, 0, 1], Sig[:, 0, 2], Sig[:, 1, 1], Sig[:, 1, 2], Sig[:, 2, 2]],
                              1).numpy().astype(np.float32)
    inp = so.Inputs(means3D=sc.means3D, opacities=sc.opacities, viewmatrix=cam.viewmatrix,
                    projmatrix=cam.projmatrix, campos=cam.campos, bg=bg, image_width=W, image_height=H,
                    tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, channels=C, scale_modifier=scale_modifier,
                    sh_degree=sh_degree, shs=sc.shs if with_shs else None,
                    colors_precomp=None if with_shs else sc.features,
                    scales=None if use_cov else sc.scales, rotations=None if use_cov else sc.rotations,
                    cov3D_precomp=cov_pre, mask=mask)
    fwd = so.forward(inp)
    assert fwd.rc == 0
    dL = scenes.make_grad_image(C, H, W, seed=seed + 1) * (W * H)
    dLm = rng.normal(0, 1, (H, W)).astype(np.float32) if use_mask else None
    bwd = so.backward(inp, fwd, dL, dLm)

    # ---- dense float64 autograd reference on the SAME fp32 input values
    t64 = lambda a, g=True: None if a is None else torch.tensor(np.asarray(a, np.float64), requires_grad=g)
    means3D, opac = t64(sc.means3D), t64(sc.opacities)
    scales_t = None if use_cov else t64(sc.scales)
    rots_t = None if use_cov else t64(sc.rotations)
    cov_t = t64(cov_pre) if use_cov else None
    cols_t = None if with_shs else t64(sc.features)
    shs_t = t64(sc.shs) if with_shs else None
    m2d = torch.zeros(P, 3, dtype=torch.float64, requires_grad=True)
    mask_t = t64(mask) if use_mask else None
    ref = render_dense(means3D, opac, t64(cam.viewmatrix, False), t64(cam.projmatrix, False), t64(cam.campos, False),
                       t64(bg, False), W, H, cam.tanfovx, cam.tanfovy, scales=scales_t, rotations=rots_t,
                       cov3D_precomp=cov_t, colors_precomp=cols_t, shs=shs_t, sh_degree=sh_degree,
                       scale_modifier=scale_modifier, means2D_offset=m2d, mask=mask_t)
    loss = (ref["color"] * torch.tensor(dL, dtype=torch.float64)).sum()
    mask_grad = None
    if use_mask:
        # reference quirk (DEPTH/cuda_rasterizer/backward.cu:516): dL/dout_mask reaches ONLY dL_dmask; it is
        # not propagated into alpha / geometry.  So the mask loss is differentiated w.r.t. mask alone.
        mloss = (ref["mask"][0] * torch.tensor(dLm, dtype=torch.float64)).sum()
        mask_grad = torch.autograd.grad(mloss, mask_t, retain_graph=True)[0]
    loss.backward()

    np.testing.assert_array_equal(fwd.radii, ref["radii"].numpy())
    assert (fwd.radii > 0).sum() > P // 3
    _assert_close("color", fwd.color, ref["color"].detach().numpy())
    _assert_close("final_T", fwd.state.field(so.F_FINAL_T).reshape(H, W), ref["final_T"].detach().numpy())
    if use_mask:
        _assert_close("mask", fwd.mask, ref["mask"].detach().numpy())
        _assert_close("depth", fwd.depth, ref["depth"].detach().numpy())
        _assert_close("dL_dmask", bwd.dL_dmask, mask_grad.numpy())
    _assert_close("dL_dmeans3D", bwd.dL_dmeans3D, means3D.grad.numpy(), rtol=5e-4)
    _assert_close("dL_dmeans2D", bwd.dL_dmeans2D[:, :2], m2d.grad.numpy()[:, :2])
    _assert_close("dL_dopacity", bwd.dL_dopacity, opac.grad.numpy())
    if with_shs:
        _assert_close("dL_dsh", bwd.dL_dsh, shs_t.grad.numpy())
    else:
        _assert_close("dL_dcolors", bwd.dL_dcolors, cols_t.grad.numpy())
    if use_cov:
        _assert_close("dL_dcov3D", bwd.dL_dcov3D, cov_t.grad.numpy(), rtol=5e-4)
    else:
        # reference quirk (CF backward.cu:295-325): dL/dscale is w.r.t. s = mod*scale and is NOT multiplied
        # by scale_modifier -- exact autograd parity only up to that factor
        _assert_close("dL_dscales", bwd.dL_dscales * scale_modifier, scales_t.grad.numpy(), rtol=5e-4)
        _assert_close("dL_drotations", bwd.dL_drotations, rots_t.grad.numpy(), rtol=5e-4)
    return fwd, bwd


@pytest.mark.parametrize("seed", [0, 1])
def test_rgb_precomp(seed):
    _run(120, 48, 40, 3, seed, bg_val=1.0)


def test_features32():
    _run(150, 40, 40, 32, 3)


def test_features64_rotated_camera():
    _run(100, 36, 52, 64, 4, rotated=True)


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_sh_degrees(deg):
    _run(80, 40, 32, 3, 10 + deg, with_shs=True, sh_degree=deg, rotated=(deg == 3), bg_val=1.0)


def test_cov3d_precomp():
    _run(90, 40, 40, 3, 7, use_cov=True)


def test_mask_depth_variant():
    _run(90, 40, 40, 3, 8, use_mask=True)


def test_scale_modifier_quirk():
    _run(80, 32, 32, 3, 9, scale_modifier=1.7)


def test_dense_ref_helpers_match_reference_python_helpers():
    """tests/dense_ref.py restates eval_sh / build_rotation / the projective transform so that it can run anywhere; the
    restatements are checked against the reference's own functions (utils/sh_utils.py:57, utils/general_utils.py:78-110,
    utils/graphics_utils.py:22-29): against their outputs stored in tests/golden/helpers/reference_helpers.npz
    (tests/golden/make_helpers_golden.py) everywhere, and against the functions themselves where the reference is present."""
    from tests import dense_ref as dr
    from tests import reference_helpers as rh
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "helpers", "reference_helpers.npz"))
    live = rh.ReferenceHelpers() if rh.present() else None
    T = lambda k: torch.from_numpy(z[k])
    q, s, sh, d = T("q"), T("s"), T("sh"), T("dirs")
    L = dr.build_rotation(q) @ torch.diag_embed(s)
    assert torch.allclose(T("build_rotation"), dr.build_rotation(q), rtol=0, atol=1e-14)
    assert torch.allclose(T("build_scaling_rotation"), L, rtol=0, atol=1e-14)
    for deg in range(4):
        assert torch.equal(T(f"eval_sh{deg}"), dr.eval_sh(deg, sh, d))
    if live is not None:
        assert torch.allclose(live.build_rotation(q), dr.build_rotation(q), rtol=0, atol=1e-14)
        assert torch.allclose(live.build_scaling_rotation(s, q), L, rtol=0, atol=1e-14)
        for deg in range(4):
            assert torch.equal(live.eval_sh(deg, sh, d), dr.eval_sh(deg, sh, d))
    # matrix conventions: scenes.py cameras == getWorld2View2 / getProjectionMatrix / full_proj (scene/cameras.py:56-65)
    for i, cam in enumerate((scenes.look_at_camera(64, 48, 50.0), scenes.orbit_camera(64, 48, 50.0, 0.3, 0.1))):
        mats = [(T(f"cam{i}_view"), T(f"cam{i}_full"))]
        if live is not None:
            gu = live.graphics_utils
            fovx, fovy = 2 * math.atan(64 / 100.0), 2 * math.atan(48 / 100.0)
            proj = gu.getProjectionMatrix(znear=0.01, zfar=100.0, fovX=fovx, fovY=fovy).transpose(0, 1)
            view = torch.tensor(gu.getWorld2View2(cam.R, cam.T)).transpose(0, 1)
            mats.append((view, view.unsqueeze(0).bmm(proj.unsqueeze(0)).squeeze(0)))
        for view, full in mats:
            assert np.allclose(view.numpy(), cam.viewmatrix, rtol=0, atol=1e-6)
            assert np.allclose(full.numpy(), cam.projmatrix, rtol=0, atol=1e-5)
            assert np.allclose(view.inverse()[3, :3].numpy(), cam.campos, atol=1e-5)
