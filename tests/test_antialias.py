"""The antialiased render mode (include/mi_rast.h: MI_RAST_ANTIALIAS) on the GPU: a known answer, equivalence with an explicit
opacity, per-group parity with the float64 autograd reference of tests/antialias_ref.py under the rule of tests/raster_edge_ref.py,
and the mode through every entry that runs or reuses the preprocess stage (features-only backward, mask-only pair, lift_scores,
geometry cache, the drop-in packages)."""
import copy
import math

import numpy as np
import pytest
import torch

import seganygaussians_amd
from seganygaussians_amd import _lib, lifting
from seganygaussians_amd import rasterizer as R
from tests import antialias_ref as ar
from tests import helpers as hp
from tests.test_raster_edges import _pixels

seganygaussians_amd.install_dropin()
pytestmark = pytest.mark.gpu

RERUN = 2e-5     # two runs of the same sums differ by the order of the float atomics (tests/test_geometry_cache.py: _same)


def _forward(inp, antialiasing, **kw):
    with R.forward_flags(antialiasing=antialiasing):
        return hp.GpuRun(inp).forward(**kw)


def _stored_w(gpu):
    return gpu.geom_fields()["conic_opacity"].reshape(-1, 4)[:, 3]


def _with_opacities(inp, w, visible):
    out = copy.copy(inp)
    out.opacities = np.where(visible, w, np.asarray(inp.opacities, np.float32).reshape(-1)).astype(np.float32).reshape(-1, 1)
    return out


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))


@pytest.mark.parametrize("s2", [0.3, 3.0])
def test_known_answer(s2):
    """One Gaussian of 2-D variance s^2 on the optical axis: the pixel sum of a channel is 2 pi opacity s^2 within 3 % (1.1 % for the
    3 sigma rect, at most 0.9 % for the alpha < 1/255 cut, 0.5 % for the sampling, rounded up); without the mode 2 pi opacity
    (s^2 + 0.3), which is 2.0 and 1.1 times as much; the stored w is opacity s^2 / (s^2 + 0.3) to 4 float32 ulp."""
    inp = ar.known_answer_inputs(s2)
    on, off = _forward(inp, True, exact_exp=True), _forward(inp, False, exact_exp=True)
    e_on, e_off = float(on.color[0].double().sum()), float(off.color[0].double().sum())
    print(f"s2 {s2}: energy {e_on:.5f} with the mode (2 pi o s2 = {2 * math.pi * 0.9 * s2:.5f}), {e_off:.5f} without")
    assert abs(e_on / (2 * math.pi * 0.9 * s2) - 1) <= 0.03
    assert abs(e_off / (2 * math.pi * 0.9 * (s2 + 0.3)) - 1) <= 0.03
    assert abs(e_off / e_on - (s2 + 0.3) / s2) <= 0.03 * (s2 + 0.3) / s2
    s2_32 = (float(np.float32(inp.scales[0, 0])) * 16.0 / 4.0) ** 2          # the variance the float32 scale really gives
    want = 0.9 * s2_32 / (s2_32 + 0.3)
    assert _ulps(_stored_w(on)[0], np.float32(want)) <= 4, (_stored_w(on)[0], want)
    assert _stored_w(off)[0] == np.float32(0.9)
    assert torch.equal(on.radii, off.radii) and on.num_rendered == off.num_rendered


def _backward_raw(gpu, dL, dLm):
    """GpuRun.backward, keeping the tensors: the named gradients and the conic gradient, which lies behind dL_dmeans2D in the block."""
    i = gpu.inp
    g = torch.as_tensor(np.ascontiguousarray(dL, np.float32)).to(gpu.dev)
    gm = None if not gpu.with_mask else torch.as_tensor(np.ascontiguousarray(dLm, np.float32)).to(gpu.dev)
    res = R.rasterize_gaussians_backward_native(
        i.channels, gpu.with_mask, gpu.bg, gpu.means3D, gpu.radii, gpu.colors, gpu.scales, gpu.rots, i.scale_modifier, gpu.cov,
        gpu.view, gpu.proj, i.tanfovx, i.tanfovy, g, gm, gpu.shs, i.sh_degree, gpu.campos, gpu.geom, gpu.num_rendered, gpu.binning,
        gpu.img, False)
    m2d = res[0]
    P = gpu.P
    s1 = (3 * P + 3) // 4 * 4                      # the block: dL_dmeans3D, dL_dmeans2D, dL_dconic, ..., each 16-byte aligned
    conic = m2d._base[2 * s1:2 * s1 + 4 * P]
    out = {"dL_dmeans2D": m2d, "dL_dcolors": res[1], "dL_dopacity": res[2], "dL_dconic": conic.view(P, 4)}
    out = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in out.items()}
    # dL_dw as THIS backward's blend kernel left it: float 5 of the 8-float packed record in the geometry buffer
    pack = gpu._view(gpu.geom, _lib.geometry_layout(P)[1]["bwd_pack"], 8 * P, np.float32).reshape(P, 8)
    out["g_w"] = pack[:, 5].copy()
    return out


def _product_h(inp):
    """h32 of the product, bit for bit: the w a forward under the mode stores for opacities of exactly 1 (w = 1 * h)."""
    ones = copy.copy(inp)
    ones.opacities = np.ones_like(np.asarray(inp.opacities, np.float32).reshape(-1, 1))
    g = _forward(ones, True, exact_exp=True)
    return _stored_w(g), g.radii.cpu().numpy() > 0


@pytest.mark.parametrize("cfg", ["c32", "mask_depth"])
def test_equivalence_with_an_explicit_opacity(cfg):
    """Run A with the mode; run B without it on opacities := the w run A stored.  Everything the blend stage makes is bit-identical,
    the gradients that do not pass through h agree up to the order of the atomics, dL_dopacity_A = h32 dL_dopacity_B."""
    ref = ar.reference(cfg)
    inp = ref.inp
    a = _forward(inp, True, exact_exp=True)
    visible = a.radii.cpu().numpy() > 0
    w = _stored_w(a)
    b = _forward(_with_opacities(inp, w, visible), False, exact_exp=True)
    assert torch.equal(a.color, b.color) and torch.equal(a.radii, b.radii) and a.num_rendered == b.num_rendered
    if a.with_mask:
        assert torch.equal(a.out_mask, b.out_mask) and torch.equal(a.out_depth, b.out_depth)
    fa, fb = a.img_fields(), b.img_fields()
    for k in ("final_T", "n_contrib", "ranges"):
        np.testing.assert_array_equal(fa[k].view(np.uint32), fb[k].view(np.uint32), err_msg=k)
    np.testing.assert_array_equal(a.bin_fields()["blend_list"], b.bin_fields()["blend_list"])
    ga, gb = _backward_raw(a, ref.dL, ref.dLm), _backward_raw(b, ref.dL, ref.dLm)
    for k in ("dL_dmeans2D", "dL_dcolors", "dL_dconic"):
        assert np.abs(ga[k] - gb[k]).max() <= RERUN * max(np.abs(gb[k]).max(), 1e-30), k
    # dL_dopacity = h32 dL_dw to 2 ulp, PER ROW: h32 is the product's own (bit for bit, from a forward on opacities of 1), dL_dw the
    # one run A's own blend backward left in its packed record -- no second run, so no order of atomics, in the comparison
    op = np.asarray(inp.opacities, np.float32).reshape(-1)
    h32, vis1 = _product_h(inp)
    np.testing.assert_array_equal(vis1, visible)
    np.testing.assert_array_equal(w[visible], (op * h32)[visible], err_msg="stored w is not float32(opacity * h32)")
    got = ga["dL_dopacity"].reshape(-1).astype(np.float32)
    want = (h32 * ga["g_w"]).astype(np.float32)
    assert (np.abs(got.astype(np.float64) - want)[visible] <= 2 * np.spacing(np.abs(want))[visible]).all(), "dL_dopacity_A != h32 * dL_dw_A"
    assert (got[~visible] == 0).all()
    assert (h32[visible] < 0.9).any() and (np.abs(ga["g_w"][visible]) > 0).any()      # (the check is not vacuous)
    # run B's dL_dopacity IS its dL_dw: the same sums in another order of the atomics, so A against B holds by the rerun rule only
    rerun_b = np.abs(got - h32 * gb["dL_dopacity"].reshape(-1)).max()
    assert rerun_b <= RERUN * np.abs(gb["dL_dopacity"]).max(), "dL_dopacity_A against h32 * dL_dopacity_B beyond the order of the atomics"
    # against a run without the mode on the original opacities: the integer path
    c = _forward(inp, False, exact_exp=True)
    assert torch.equal(a.radii, c.radii) and a.num_rendered == c.num_rendered
    np.testing.assert_array_equal(a.bin_fields()["point_list"], c.bin_fields()["point_list"])
    np.testing.assert_array_equal(fa["ranges"], c.img_fields()["ranges"])
    gf_a, gf_c = a.geom_fields(), c.geom_fields()
    for k in ("tiles_touched", "depth_key"):
        np.testing.assert_array_equal(gf_a[k], gf_c[k], err_msg=k)
    np.testing.assert_array_equal(_stored_w(c)[visible], op[visible])


def _run(ref, full_lists, exact_exp):
    with R.forward_flags(antialiasing=True):
        gpu = hp.GpuRun(ref.inp).forward(full_lists=full_lists, exact_exp=exact_exp)
    np.testing.assert_array_equal(gpu.radii.cpu().numpy(), ref.radii, err_msg="radii")
    got = _pixels(ref, gpu)
    from tests import raster_edge_ref as er
    got.update(er.classes_of_grads(ref.inp, gpu.backward(ref.dL, ref.dLm)))
    return gpu, got


@pytest.mark.parametrize("full_lists", [True, False], ids=["full", "lean"])
@pytest.mark.parametrize("cfg", list(ar.AA_CONFIGS))
def test_exact_exp_forward_and_backward(cfg, full_lists):
    """Every image pixel and every row of every gradient against float64 autograd through the blend and through h, by the rule."""
    ref = ar.reference(cfg)
    gpu, got = _run(ref, full_lists, True)
    if full_lists:
        hp.compare_integer_path(gpu, ref.fwd)
    ref.check(f"antialias {cfg} full_lists={full_lists}", got)
    # the rows the scene was designed for
    cls = ref.inp.classes
    faint, needle = cls.index("aa_faint"), cls.index("aa_needle")
    assert gpu.radii[faint] > 0
    for k, v in got.items():
        if k not in ("image", "final_T", "out_mask", "out_depth"):
            assert np.abs(v[faint]).max() == 0.0, (k, "aa_faint")
    assert _stored_w(gpu)[needle] == np.float32(np.float32(1.0) * np.sqrt(np.float32(0.000025)))


@pytest.mark.parametrize("full_lists", [True, False], ids=["full", "lean"])
@pytest.mark.parametrize("size", ar.SMALL, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cfg", ["rgb", "c32"])
def test_small_sizes_one_gaussian(cfg, size, full_lists):
    ref = ar.reference(cfg, size[0], size[1], 1)
    gpu, got = _run(ref, full_lists, True)
    ref.check(f"antialias {cfg} {size} P1 full_lists={full_lists}", got)


def test_default_hybrid_exp_forward():
    from tests import raster_edge_ref as er
    ref = ar.reference("c32")
    hy, got = _run(ref, False, None)
    with R.forward_flags(antialiasing=True):
        ex = hp.GpuRun(ref.inp).forward(full_lists=False, exact_exp=True)
    keep = ~ref.excused_pixels
    np.testing.assert_array_equal(hy.img_fields()["n_contrib"][keep], ex.img_fields()["n_contrib"][keep], err_msg="n_contrib")
    classes = ["image"] + [c for c in ref.classes if c not in er.PIXEL_CLASSES]
    ref.check("antialias hybrid c32", got, extra=ref.hybrid_extra(), classes=classes)


def test_features_only_backward():
    ref = ar.reference("c32")
    with R.forward_flags(antialiasing=True):
        gpu = hp.GpuRun(ref.inp).forward(full_lists=False, exact_exp=True)
    got = gpu.backward(ref.dL, features_only=True)["dL_dcolors"]
    ref.check("antialias features-only c32", {"dL_dcolors": got}, classes=["dL_dcolors"])


def _lift_geometry(g):
    opt = lambda t: t if t.numel() else None
    return dict(scales=opt(g.scales), rotations=opt(g.rots), cov3D_precomp=opt(g.cov), viewmatrix=g.view, projmatrix=g.proj,
                tanfovx=g.inp.tanfovx, tanfovy=g.inp.tanfovy, scale_modifier=g.inp.scale_modifier)


def cls_rows(ref):
    """The appended designed Gaussians of the mode (well conditioned: the CPU's h32 and the product's agree closely there)."""
    return [i for i, c in enumerate(ref.inp.classes) if c in ("aa_subpixel", "aa_large", "aa_faint", "aa_clamped")]


def _mask_forward(g, antialiasing):
    inp = g.inp
    with R.forward_flags(full_lists=True, exact_exp=True, antialiasing=antialiasing):
        return R.rasterize_mask_gaussians_native(g.means3D, g.opac, g.mask, g.scales, g.rots, inp.scale_modifier, g.cov, g.view, g.proj,
                                                 inp.tanfovx, inp.tanfovy, inp.image_height, inp.image_width, False, False)


def test_mask_only_pair_and_lift_scores():
    """The mask-only forward under the mode is bit-identical to the one of run B (explicit opacities); its backward follows the
    forward's flags; lift_scores under the mode gives dL_dcolors of the mode's backward, judged as tests/test_lifting.py judges."""
    ref = ar.reference("mask_depth")
    a = hp.GpuRun(ref.inp)
    nr_a, mask_a, radii_a, geom_a, bin_a, img_a = _mask_forward(a, True)
    assert geom_a.mi_notes.flags & 1024
    w = a._view(geom_a, _lib.geometry_layout(a.P)[1]["conic_opacity"], 4 * a.P, np.float32).reshape(-1, 4)[:, 3]
    visible = radii_a.cpu().numpy() > 0
    # the mask-only forward honours the flag: it stores the w of the full forward under the mode, and that is not the opacity
    op = np.asarray(ref.inp.opacities, np.float32).reshape(-1)
    np.testing.assert_array_equal(w[visible], _stored_w(_forward(ref.inp, True, exact_exp=True))[visible])
    assert (w[visible] != op[visible]).any()
    np.testing.assert_allclose(w[cls_rows(ref)], (op * ref.h32)[cls_rows(ref)], rtol=1e-5)
    b = hp.GpuRun(_with_opacities(ref.inp, w, visible))
    nr_b, mask_b, radii_b, geom_b, bin_b, img_b = _mask_forward(b, False)
    assert nr_a == nr_b and torch.equal(radii_a, radii_b) and torch.equal(mask_a, mask_b)
    dLm = torch.as_tensor(ref.dLm).cuda()
    gm_a = R.rasterize_mask_gaussians_backward_native(a.means3D, dLm, geom_a, nr_a, bin_a, img_a, False)
    gm_b = R.rasterize_mask_gaussians_backward_native(b.means3D, dLm, geom_b, nr_b, bin_b, img_b, False)
    assert float((gm_a - gm_b).abs().max()) <= RERUN * float(gm_b.abs().max())

    ref = ar.reference("c32")
    g = hp.GpuRun(ref.inp)
    s = torch.as_tensor(np.asarray(ref.dL, np.float32)).to(g.dev)
    with R.forward_flags(full_lists=False, exact_exp=True, antialiasing=True):
        votes, st = lifting.lift_scores(s, g.means3D, g.opac, return_state=True, **_lift_geometry(g))
    assert st.flags & 1024
    np.testing.assert_array_equal(st.radii.cpu().numpy(), ref.radii)
    ref.check("antialias lift c32", {"dL_dcolors": votes.cpu().numpy()}, classes=["dL_dcolors"])
    votes2 = lifting.lift_scores(s, g.means3D, g.opac, state=st)          # the reuse entry reads the stored w
    assert float((votes2 - votes).abs().max()) <= RERUN * float(votes.abs().max())


def _dropin_step(mod, inp, leaves, dL):
    dev = dL.device
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(dev)
    settings = mod.GaussianRasterizationSettings(
        image_height=inp.image_height, image_width=inp.image_width, tanfovx=inp.tanfovx, tanfovy=inp.tanfovy, bg=t(inp.bg),
        scale_modifier=inp.scale_modifier, viewmatrix=t(inp.viewmatrix), projmatrix=t(inp.projmatrix), sh_degree=0, campos=t(inp.campos),
        prefiltered=False, debug=False)
    for l in leaves:
        l.grad = None
    means3D, feats, opac, scales, rots = leaves
    means2D = torch.zeros_like(means3D, requires_grad=True)
    color, radii = mod.GaussianRasterizer(settings)(means3D=means3D, means2D=means2D, shs=None, colors_precomp=feats, opacities=opac,
                                                    scales=scales, rotations=rots, cov3D_precomp=None)
    color.backward(dL)
    return [color.detach().clone(), radii.clone()] + [l.grad.clone() for l in leaves] + [means2D.grad.clone()]


def _leaves(inp, dev):
    return [torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(dev).requires_grad_(True)
            for a in (inp.means3D, inp.colors_precomp, inp.opacities, inp.scales, inp.rotations)]


def _same(a, b, what):
    assert torch.equal(a[0], b[0]), f"{what}: image differs"
    assert torch.equal(a[1], b[1]), f"{what}: radii differ"
    for x, y, name in zip(a[2:], b[2:], ("dL_dmeans3D", "dL_dfeatures", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dmeans2D")):
        assert float((x - y).abs().max()) <= RERUN * max(float(y.abs().max()), 1e-30), f"{what}: {name} differs beyond atomic order"


def test_geometry_cache_keys_on_the_mode():
    import diff_gaussian_rasterization_contrastive_f as mod
    dev = torch.device("cuda:0")
    inp = ar.reference("c32").inp
    leaves = _leaves(inp, dev)
    dL = torch.as_tensor(ar.reference("c32").dL).to(dev)
    R.disable_geometry_cache()
    with R.forward_flags(antialiasing=True):
        plain_on = _dropin_step(mod, inp, leaves, dL)
    c = R.enable_geometry_cache(1 << 30)
    c.clear()
    try:
        off1 = _dropin_step(mod, inp, leaves, dL)
        assert c.stats()["misses"] == 1 and c.stats()["hits"] == 0
        with R.forward_flags(antialiasing=True):
            on1 = _dropin_step(mod, inp, leaves, dL)
            assert c.stats()["misses"] == 2 and c.stats()["hits"] == 0, "a change of the mode must miss"
            on2 = _dropin_step(mod, inp, leaves, dL)
            assert c.stats()["hits"] == 1
        off2 = _dropin_step(mod, inp, leaves, dL)
        assert c.stats()["hits"] == 2 and c.stats()["misses"] == 2
    finally:
        R.disable_geometry_cache(drop=True)
    assert not torch.equal(on1[0], off1[0])
    _same(on1, plain_on, "first visit with the mode")
    _same(on2, plain_on, "cached visit with the mode")
    _same(off2, off1, "back without the mode")


def test_autograd_through_a_drop_in_package():
    """Under forward_flags(antialiasing=True) and under enable_antialiasing() the drop-in package returns the native calls' gradients."""
    import diff_gaussian_rasterization_contrastive_f as mod
    from tests import raster_edge_ref as er
    ref = ar.reference("c32")
    inp = ref.inp
    dev = torch.device("cuda:0")
    with R.forward_flags(antialiasing=True):
        gpu = hp.GpuRun(inp).forward(full_lists=False)
    native = gpu.backward(ref.dL)
    want = [gpu.color, gpu.radii] + [torch.as_tensor(native[k]).to(dev).reshape(s) for k, s in
                                     (("dL_dmeans3D", (-1, 3)), ("dL_dcolors", (-1, 32)), ("dL_dopacity", (-1, 1)), ("dL_dscales", (-1, 3)),
                                      ("dL_drotations", (-1, 4)), ("dL_dmeans2D", (-1, 3)))]
    dL = torch.as_tensor(ref.dL).to(dev)
    leaves = _leaves(inp, dev)
    with R.forward_flags(antialiasing=True):
        _same(_dropin_step(mod, inp, leaves, dL), want, "forward_flags")
    off = _dropin_step(mod, inp, leaves, dL)
    assert not torch.equal(off[0], want[0])
    prev = R.enable_antialiasing()
    try:
        _same(_dropin_step(mod, inp, leaves, dL), want, "enable_antialiasing")
    finally:
        R.enable_antialiasing(prev)
