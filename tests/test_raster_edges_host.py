"""CPU half of the rasterizer's edge tests (tests/raster_edge_ref.py; the GPU half is tests/test_raster_edges.py): for every scene
and variant the GPU tests use -- the caps on excused groups, radii equal to the oracle's, the mutual calibration check of FACTOR and
FLOOR, the oracle against dense float64 per group under the final rule, the exact-zero groups, and that each designed class is
what its name says.  It also closes a hole in the oracle's own pin (tests/test_oracle_dense.py never had a Gaussian beyond the
1.3 tan(fov) clamp or a saturated alpha): with dense_ref's reference_quirks the oracle agrees with autograd there per row."""
import numpy as np
import pytest

from oracle import saga_oracle as so
from tests import raster_edge_ref as er

CASES = er.all_cases()


def _id(case):
    fn, W, H, C, seed, v = case
    tags = [fn, f"{W}x{H}", f"C{C}", v.colors] + [k for k in ("mask", "mask_only", "cov") if getattr(v, k)]
    tags += [f"mod{v.modifier}"] * (v.modifier != 1.0) + [f"bg-{v.bg}"] * (v.bg != "zero")
    tags += [f"{v.kind}{v.L}"] * (v.kind is not None) + [f"P{v.P}"] * (v.P != 96)
    return "-".join(tags)


def _rows(ref, cls):
    return [i for i, c in enumerate(ref.inp.classes) if c == cls]


def _blended(ref):
    """(P,) in input order: the Gaussian is blended at some pixel;  (P, N): where."""
    w = np.zeros_like(ref.dense["weights"])
    w[ref.dense["order"]] = ref.dense["weights"]
    return (w > 0).any(axis=1), w > 0


def _evaluated(ref):
    """(P, N) in input order: the pair is in the pixel's tile list and the pixel had not stopped before it."""
    d = ref.dense
    N = d["member"].shape[1]
    c = d["member"] & np.concatenate([np.ones((1, N), bool), d["alive"][:-1]], 0)
    out = np.zeros_like(c)
    out[d["order"]] = c
    return out


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_caps_radii_calibration_and_oracle(case):
    ref = er.reference(case)
    P = len(ref.radii)
    # the caps are conditions of the scene, not measurements; no designed class is excused
    assert int(ref.excused_gaussians.sum()) <= er.EXCUSED_GAUSSIANS and int(ref.excused_pixels.sum()) <= er.EXCUSED_PIXELS
    assert all(ref.inp.classes[i] == "fill" for i in np.flatnonzero(ref.excused_gaussians))
    # the integer decisions of the three evaluations agree
    np.testing.assert_array_equal(ref.fwd.radii, ref.radii, err_msg="radii: oracle vs dense64")
    np.testing.assert_array_equal(ref.radii32, ref.radii, err_msg="radii: dense32 vs dense64")
    np.testing.assert_array_equal(ref.fwd.state.field(so.F_TILES_TOUCHED)[:P], ref.tiles_touched, err_msg="tile rects")
    for cls in ref.classes:
        f, fl = er.mutual_rule(cls)
        # the two float32 restatements judge each other with the undoubled constants
        r_o, _ = ref.ratios(cls, ref.oracle[cls], f, fl, e32_from=("d32",))
        r_d, _ = ref.ratios(cls, ref.d32[cls], f, fl, e32_from=("oracle",))
        assert (r_o <= 1.0).all() and (r_d <= 1.0).all(), (cls, float(r_o.max()), float(r_d.max()),
                                                             ref.group_name(cls, int(np.argmax(np.maximum(r_o, r_d)))))
    # the oracle under the rule the product is held to, exact zeros included; dense32 takes the same zero decisions
    ref.check("oracle", ref.oracle)
    for cls in ref.classes:
        _, zd = ref.ratios(cls, ref.d32[cls], *er.rule(cls))
        assert not zd.any(), (cls, "dense32 zero groups")


@pytest.mark.parametrize("cfg", er.STRICT_CONFIGS)
def test_designed_classes_are_what_their_names_say(cfg):
    ref = er.reference(er.edge_case(cfg))
    inp, d = ref.inp, ref.dense
    W, H = inp.image_width, inp.image_height
    blended, where = _blended(ref)
    evaluated = _evaluated(ref)
    grad_classes = [c for c in ref.classes if c not in er.PIXEL_CLASSES]
    zero_row = lambda i: all(np.abs(ref.d64[c][i]).max() == 0 and np.abs(ref.oracle[c][i]).max() == 0 for c in grad_classes)
    limx, limy = 1.3 * inp.tanfovx, 1.3 * inp.tanfovy
    one = lambda cls: _rows(ref, cls)[0]
    # clamped centres: beyond the clamp in the named axes only, and blended
    for cls, cx, cy in (("clamped_x", True, False), ("clamped_y", False, True), ("clamped_xy", True, True)):
        i = one(cls)
        assert (abs(d["txtz"][i]) > limx) == cx and (abs(d["tytz"][i]) > limy) == cy and blended[i], cls
    # centres outside the image whose radius reaches in; one rect over every tile
    means = np.asarray(inp.means3D, np.float64)
    focal = W / (2 * inp.tanfovx)
    u = focal * means[:, 0] / means[:, 2] + (W - 1) / 2
    v = focal * means[:, 1] / means[:, 2] + (H - 1) / 2
    for i in _rows(ref, "off_image") + _rows(ref, "border_half_out"):
        assert (u[i] < 0 or u[i] > W - 1 or v[i] < 0 or v[i] > H - 1) and blended[i], (i, u[i], v[i])
    assert ref.tiles_touched[one("cover_all")] == ((W + 15) // 16) * ((H + 15) // 16)
    # near plane: one float32 ulp above float32(0.2) is seen, one below is culled and leaves exactly zero rows
    assert blended[one("near_visible")] and ref.radii[one("near_visible")] > 0
    assert ref.radii[one("near_culled")] == 0 and zero_row(one("near_culled"))
    # tiny: the low-pass alone (cov2D = 0.3 I: lambda = 0.3 + sqrt(0.1), radius ceil(3 sqrt(0.616)) = 3); needles; quaternions
    s = np.asarray(inp.scales if inp.scales is not None else np.zeros((len(u), 3)), np.float64) * inp.scale_modifier
    if inp.scales is not None:
        for i in _rows(ref, "tiny"):
            assert s[i].max() <= 1.0001e-4 and ref.radii[i] == 3 and blended[i]
        for i in _rows(ref, "needle"):
            assert 999 < s[i].max() / s[i].min() < 1001 and blended[i]
        norms = np.linalg.norm(np.asarray(inp.rotations, np.float64), axis=1)[_rows(ref, "unnorm_quat")]
        assert norms.min() < 0.51 and norms.max() > 1.99
    # the opaque stack: a saturated alpha is blended on its pixel, the pixel stops there, the hidden Gaussians are in its list but
    # not blended at that pixel and blended next to it
    px = ref.inp.stack_pixel[1] * W + ref.inp.stack_pixel[0]
    raw = np.zeros_like(d["raw_alpha"])
    raw[d["order"]] = d["raw_alpha"]
    st = _rows(ref, "stack")
    assert where[st[0], px] and where[st[1], px] and raw[st[1], px] > 0.99
    assert evaluated[st[2], px] and not where[st[2], px]                 # the entry that ends the pixel is not blended
    assert (raw > 0.99)[where].sum() >= 3                                # saturated pairs next to it as well
    for i in _rows(ref, "hidden"):
        assert not evaluated[i, px] and not where[i, px] and where[i].any() and d["member"][list(d["order"]).index(i), px]
    # faint: a row below the cut has radii > 0, no pair and exactly zero gradients; just above has a pair
    assert blended[one("faint_above")]
    for cls in ("faint_below", "opacity_zero"):
        assert ref.radii[one(cls)] > 0 and not blended[one(cls)] and zero_row(one(cls)), cls
    # equal depths: the same bits, and two of them blended on one pixel
    eq = _rows(ref, "equal_depth")
    assert len({np.float32(means[i, 2]).tobytes() for i in eq}) == 1 and (where[eq].sum(axis=0) >= 2).any()
    # SH colours below zero: that channel's dL_dsh is exactly zero
    if inp.shs is not None:
        for k in (1, 2, 3):
            i = one("sh_clamped_%d" % k)
            neg = d["sh_pre_clamp"][i] < 0
            assert neg.sum() == k and blended[i]
            for name in ("d64", "oracle"):
                g = getattr(ref, name)["dL_dsh"][i].reshape(-1, 3)
                assert (np.abs(g).max(axis=0) == 0).tolist() == neg.tolist(), (k, name)
    # placement
    assert abs(u[one("pixel_centre")] - W // 3) < 1e-4 and abs(u[one("last_pixel")] - (W - 1)) < 1e-4
    assert abs(u[_rows(ref, "tile_corner")[0]] - 16) < 1e-4 and abs(v[_rows(ref, "tile_corner")[0]] - 16) < 1e-4


@pytest.mark.parametrize("cfg", list(er.CONFIGS))
@pytest.mark.parametrize("kind", ["contrib", "raw"])
def test_list_scene_has_the_lengths_it_claims(cfg, kind):
    assert {er.XG, er.CHK} == {16} and {er.FB, er.XB, er.ROWS} == {128}, "LIST_LENGTHS follow the headers; so must the scenes' notes"
    for L in er.LIST_LENGTHS:
        ref = er.reference(er.list_case(cfg, kind, L))
        ranges = ref.fwd.state.field(so.F_RANGES)
        assert len(ranges) == 2 and int(ranges[1]) - int(ranges[0]) == L == ref.fwd.num_rendered
        blended, where = _blended(ref)
        if kind == "contrib":
            assert where.all(), "every entry blends at every pixel"
        else:
            dead = np.array([c == "culled_entry" for c in ref.inp.classes])
            assert dead.any() and (ref.radii[dead] > 0).all() and not blended[dead].any() and blended[~dead].all()


def test_small_scenes():
    for cfg in er.SMALL_CONFIGS:
        one = er.reference(er.edge_case(cfg, P=1))
        assert len(one.radii) == 1 and one.radii[0] > 0 and _blended(one)[0][0]
        culled = er.reference(er.edge_case(cfg, P="culled"))
        assert (culled.radii == 0).all() and culled.fwd.num_rendered == 0 and len(culled.radii) > 1
        for W, H in er.SMALL_SIZES:
            assert _blended(er.reference(er.edge_case(cfg, W, H)))[0].any()
