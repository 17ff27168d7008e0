"""Rasterizer edge scenes on the GPU: every kernel family against the dense float64 reference, per pixel and per Gaussian row
(the scenes, the decision margins and the rule: tests/raster_edge_ref.py; their CPU half: tests/test_raster_edges_host.py).

tests/test_gpu_parity.py judges whole tensors against the oracle with a floor at the tensor's largest element: a Gaussian whose
gradient row is a thousand times smaller than the largest can be wrong there unseen.  Here every group has its own bound,

    |product - dense64| <= max(FACTOR * E32, FLOOR * magnitude of the group's terms),

and a group that dense64 leaves at exactly zero must be exactly zero.  Every case prints the worst error / bound per class.

The tests named *_tiles_* run the same kernels on the many-tile scenes of er.tile_cases() (97 x 33: 21 tiles, 177 x 17: 24 tiles;
their own calibrated table, er.MUTUAL_TILES): gradient rows summed by atomics from every tile, the eight XCD runs cut at equal
modelled work with their queued halves (and again cut at equal tile counts), empty ranges between occupied tiles, last tile
columns and rows one pixel wide, a tile whose walk ends in the first quarter of its list."""
import numpy as np
import pytest

from oracle import saga_oracle as so
from tests import helpers as hp
from tests import raster_edge_ref as er

pytestmark = pytest.mark.gpu


def _pixels(ref, gpu):
    inp = ref.inp
    n = inp.image_width * inp.image_height
    out = {"image": gpu.color.cpu().numpy().astype(np.float64).reshape(inp.channels, n).T,
           "final_T": gpu.img_fields()["final_T"].astype(np.float64).reshape(n, 1)}
    if gpu.with_mask:
        out["out_mask"] = gpu.out_mask.cpu().numpy().astype(np.float64).reshape(n, 1)
        out["out_depth"] = gpu.out_depth.cpu().numpy().astype(np.float64).reshape(n, 1)
    return out


def _run(ref, full_lists, exact_exp):
    """Forward and default backward of one case; the product's classes."""
    gpu = hp.GpuRun(ref.inp).forward(full_lists=full_lists, exact_exp=exact_exp)
    np.testing.assert_array_equal(gpu.radii.cpu().numpy(), ref.radii, err_msg="radii")
    got = _pixels(ref, gpu)
    got.update(er.classes_of_grads(ref.inp, gpu.backward(ref.dL, ref.dLm)))
    return gpu, got


def _mask_only(ref, full_lists, keep=None):
    """The mask-only pair of one case; the product's classes (keep, a dict: the forward's image buffer is left in it)."""
    import torch
    from seganygaussians_amd import rasterizer as R
    inp = ref.inp
    g = hp.GpuRun(inp)
    with R.forward_flags(full_lists=full_lists, exact_exp=True):
        nr, out_mask, radii, geom, binning, img = R.rasterize_mask_gaussians_native(
            g.means3D, g.opac, g.mask, g.scales, g.rots, inp.scale_modifier, g.cov, g.view, g.proj, inp.tanfovx, inp.tanfovy,
            inp.image_height, inp.image_width, False, False)
    assert nr == ref.fwd.num_rendered or not full_lists
    np.testing.assert_array_equal(radii.cpu().numpy(), ref.radii, err_msg="radii")
    gm = R.rasterize_mask_gaussians_backward_native(g.means3D, torch.as_tensor(ref.dLm).cuda(), geom, nr, binning, img, False)
    if keep is not None:
        keep["img"] = img
    return {"out_mask": out_mask.cpu().numpy().astype(np.float64).reshape(-1, 1), "dL_dmask": gm.cpu().numpy().astype(np.float64).reshape(-1, 1)}


def _cases(cfg, scene):
    return [er.edge_case(cfg)] if scene == "edge" else er.list_cases(cfg)


def _merge(worst, w):
    for k, v in w.items():
        worst[k] = max(worst.get(k, 0.0), v)


def _strict(case, full_lists, worst):
    ref = er.reference(case)
    name = f"{case[0]} {case[1]}x{case[2]} C{case[3]} {case[5].kind or ''}{case[5].L or ''} P{case[5].P} full_lists={full_lists}"
    if case[5].mask_only:
        _merge(worst, ref.check(name, _mask_only(ref, full_lists)))
        return
    gpu, got = _run(ref, full_lists, True)
    if full_lists:
        hp.compare_integer_path(gpu, ref.fwd)
    _merge(worst, ref.check(name, got))


def _hybrid(case, worst):
    ref = er.reference(case)
    name = f"hybrid {case[0]} C{case[3]} {case[5].kind or ''}{case[5].L or ''}"
    hy, got = _run(ref, False, None)
    ex = hp.GpuRun(ref.inp).forward(full_lists=False, exact_exp=True)
    keep = ~ref.excused_pixels
    np.testing.assert_array_equal(hy.img_fields()["n_contrib"][keep], ex.img_fields()["n_contrib"][keep], err_msg="n_contrib")
    classes = ["image"] + [c for c in ref.classes if c not in er.PIXEL_CLASSES]
    _merge(worst, ref.check(name, got, extra=ref.hybrid_extra(), classes=classes))


def _features_only(case, worst):
    ref = er.reference(case)
    name = f"features-only {case[0]} {case[1]}x{case[2]} C{case[3]} {case[5].kind or ''}{case[5].L or ''} P{case[5].P}"
    gpu = hp.GpuRun(ref.inp).forward(full_lists=False, exact_exp=True)
    default = gpu.backward(ref.dL)["dL_dcolors"]
    got = gpu.backward(ref.dL, features_only=True)["dL_dcolors"]
    _merge(worst, ref.check(name, {"dL_dcolors": got}, classes=["dL_dcolors"]))
    np.testing.assert_array_equal(np.abs(got).max(axis=1) == 0, np.abs(default).max(axis=1) == 0, err_msg=name + ": zero rows")


@pytest.mark.parametrize("full_lists", [True, False], ids=["full", "lean"])
@pytest.mark.parametrize("scene", ["edge", "list"])
@pytest.mark.parametrize("cfg", er.STRICT_CONFIGS)
def test_exact_exp_forward_and_backward(cfg, scene, full_lists):
    """Forward with expf for every pair and the backward after it, under the strict rule: on the 37 x 21 scene of designed classes
    and on the 16 x 16 scene whose list ends one below, at and one above the kernels' batch sizes; with full lists (where the
    integer path is the oracle's bit for bit) and with the product's lean lists."""
    worst = {}
    for case in _cases(cfg, scene):
        _strict(case, full_lists, worst)
    print(f"worst error / bound, {cfg} {scene} full_lists={full_lists}: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


SMALL = ["16x16", "1x1", "40x5", "5x40", "P1", "culled"]


@pytest.mark.parametrize("full_lists", [True, False], ids=["full", "lean"])
@pytest.mark.parametrize("which", SMALL)
@pytest.mark.parametrize("cfg", ["rgb", "c32"])
def test_small_sizes_one_gaussian_and_all_culled(cfg, which, full_lists):
    """16 x 16, 1 x 1, 40 x 5 and 5 x 40 images, P = 1, and a scene in which every Gaussian is culled.

    The 1 x 1 image is the case that found the float32 moment shift of the backward: one pixel, a centre
    0.3 px from it, and dL_dmeans3D / dL_dscales 1.4 / 1.8 times the bound until the moments became exact and their shift binary64."""
    worst = {}
    _strict(er.small_cases(cfg)[SMALL.index(which)], full_lists, worst)


@pytest.mark.parametrize("scene", ["edge", "list"])
@pytest.mark.parametrize("cfg", [c for c in er.STRICT_CONFIGS if c != "mask_only"])
def test_default_hybrid_exp_forward(cfg, scene):
    """The product default (csrc/common.h, hybrid evaluation: alpha within 1e-6 relative of the expf form's).  Image per pixel within
    the strict bound plus 1e-6 sum_g k_g w_g |c_g|, k_g = 1 + sum_{j<g} alpha_j / (1 - alpha_j); the gradients after it per row
    within the strict bound plus 1e-6 K_max times the row's term magnitude; n_contrib that of the expf run on every pixel that is
    not excused."""
    worst = {}
    for case in _cases(cfg, scene):
        _hybrid(case, worst)
    print(f"worst error / bound, hybrid {cfg} {scene}: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("cfg", er.FEATURE_CONFIGS)
def test_features_only_backward(cfg):
    """The features-only backward (csrc/blend_bwd_feat.h, one wave per half tile): dL_dcolors per row under the strict rule and the
    same zero rows as the default backward -- on the 37 x 21 scene, on every list length, and on the small images (the 16 x 16 and
    the 1 x 1 among them), P = 1 and the culled scene."""
    worst = {}
    for case in [er.edge_case(cfg)] + er.list_cases(cfg) + er.small_cases(cfg):
        _features_only(case, worst)
    print(f"worst error / bound, features-only {cfg}: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---- the many-tile scenes ----------------------------------------------------------------------------------------------------------

TILES = [(which, cfg) for which, cfgs in er.TILE_CONFIGS.items() for cfg in cfgs]
FULL = pytest.mark.parametrize("full_lists", [True, False], ids=["full", "lean"])


def _tile_id(t):
    return "-".join(t)


def _zero_rows(ref, got):
    return {c: np.abs(np.asarray(got[c], np.float64).reshape(ref.d64[c].shape)).max(axis=1) == 0 for c in ref.classes}


def _tiles_both_runs(ref, name, full_lists, launch):
    """`launch()` -> the product's classes, once with the XCD runs of equal modelled work (the default) and once with those of
    equal tile counts: both under the rule, with identical zero groups."""
    from seganygaussians_amd import rasterizer as R
    worst, zero = {}, []
    for equal_runs in (False, True):
        with R.forward_flags(equal_runs=equal_runs):
            got = launch()
        _merge(worst, ref.check(f"{name} full_lists={full_lists} equal_runs={equal_runs}", got))
        zero.append(_zero_rows(ref, got))
    for c in ref.classes:
        np.testing.assert_array_equal(zero[0][c], zero[1][c], err_msg=f"{name}: zero groups of {c}, default runs vs equal runs")
    print(f"worst error / bound, {name} full_lists={full_lists}: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@FULL
@pytest.mark.parametrize("tile", [t for t in TILES if t[1] != "mask_only"], ids=_tile_id)
def test_tiles_exact_exp_forward_and_backward(tile, full_lists):
    """expf forward and default backward per pixel and per Gaussian row on the many-tile scenes, with both cuts of the XCD runs;
    with full lists the integer path is the oracle's bit for bit."""
    ref = er.reference(er.tile_case(*tile))

    def launch():
        gpu, got = _run(ref, full_lists, True)
        if full_lists:
            hp.compare_integer_path(gpu, ref.fwd)
        return got
    _tiles_both_runs(ref, "tiles " + _tile_id(tile), full_lists, launch)


@FULL
def test_tiles_mask_only_pair(full_lists):
    ref = er.reference(er.tile_case("t1", "mask_only"))
    _tiles_both_runs(ref, "tiles t1-mask_only", full_lists, lambda: _mask_only(ref, full_lists))


@FULL
@pytest.mark.parametrize("tile", TILES, ids=_tile_id)
def test_tiles_published_run_boundaries(tile, full_lists):
    """The nine run boundaries the range scan leaves behind the image buffer's num_rendered field (include/mi_rast.h): monotone
    from 0 to the tile count; by default those of equal modelled work -- the CPU restatement of tests/test_xcd_mapping.py on the
    lists of this forward, which with full lists are the oracle's (tests/test_raster_edges_host.py asserts what those runs look
    like: not the equal-count ones, one run of a single tile) --; with equal_runs those of equal tile counts."""
    from seganygaussians_amd import rasterizer as R
    from tests.test_xcd_mapping import bounds_from_model, run_start
    ref = er.reference(er.tile_case(*tile))
    W, H = ref.inp.image_width, ref.inp.image_height
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    bounds = {}
    for equal_runs in (False, True):
        with R.forward_flags(equal_runs=equal_runs):
            if tile[1] == "mask_only":
                keep = {}
                _mask_only(ref, full_lists, keep)
                img = keep["img"]
            else:
                img = hp.GpuRun(ref.inp).forward(full_lists=full_lists, exact_exp=True).img
        b = hp.run_bounds(img, W, H)
        print(f"tiles {_tile_id(tile)} full_lists={full_lists} equal_runs={equal_runs}: run boundaries {b.tolist()}")
        assert b[0] == 0 and b[8] == ntiles and (np.diff(b) >= 0).all(), b
        ranges = hp.tile_ranges(img, W, H)
        if full_lists:
            np.testing.assert_array_equal(ranges.reshape(-1), ref.fwd.state.field(so.F_RANGES), err_msg="tile ranges")
        if equal_runs:
            assert b.tolist() == [run_start(x, ntiles) for x in range(9)]
        else:
            assert b.tolist() == bounds_from_model(ranges[:, 1] - ranges[:, 0], er.RUN_CAP, er.RUN_FIX), "modelled-work runs of this forward's lists"
            if full_lists:
                assert b.tolist() == er.model_runs(ref)[0]
        bounds[equal_runs] = b.tolist()
    assert bounds[False] != bounds[True]


@pytest.mark.parametrize("cfg", ["rgb", "c32"])
def test_tiles_default_hybrid_exp_forward(cfg):
    """The product default (hybrid exp) on the 97 x 33 scene, as test_default_hybrid_exp_forward."""
    worst = {}
    _hybrid(er.tile_case("t1", cfg), worst)
    print(f"worst error / bound, hybrid tiles t1-{cfg}: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("tile", [("t1", "c32"), ("t1", "c64"), ("t2", "c32")], ids=_tile_id)
def test_tiles_features_only_backward(tile):
    """dL_dcolors of the features-only backward per row, and the zero rows of the default backward."""
    worst = {}
    _features_only(er.tile_case(*tile), worst)
    print(f"worst error / bound, features-only tiles {_tile_id(tile)}: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
