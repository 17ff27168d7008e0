"""CPU half of the rasterizer's edge tests (tests/raster_edge_ref.py; the GPU half is tests/test_raster_edges.py): for every scene
and variant the GPU tests use -- the caps on excused groups, radii equal to the oracle's, the mutual calibration check of FACTOR and
FLOOR, the oracle against dense float64 per group under the final rule, the exact-zero groups, and that each designed class is
what its name says; the same for the many-tile scenes of er.tile_cases() under their own table (MUTUAL_TILES), with the
properties those scenes are designed for and the XCD runs they give.  It also closes a hole in the oracle's own pin (tests/test_oracle_dense.py never had a Gaussian beyond the
1.3 tan(fov) clamp or a saturated alpha): with dense_ref's reference_quirks the oracle agrees with autograd there per row."""
import numpy as np
import pytest

from oracle import saga_oracle as so
from tests import raster_edge_ref as er

CASES = er.all_cases()
TILE_CASES = er.tile_cases()


def _id(case):
    fn, W, H, C, seed, v = case
    tags = [fn, f"{W}x{H}", f"C{C}", v.colors] + [k for k in ("mask", "mask_only", "cov") if getattr(v, k)]
    tags += [f"mod{v.modifier}"] * (v.modifier != 1.0) + [f"bg-{v.bg}"] * (v.bg != "zero")
    tags += [f"{v.kind}{v.L or ''}"] * (v.kind is not None) + [f"P{v.P}"] * (v.P != 96)
    return "-".join(tags)


def _rows(ref, cls):
    return [i for i, c in enumerate(ref.inp.classes) if c == cls]


def _blended(ref):
    """(P,) in input order: the Gaussian is blended at some pixel;  (P, N): where."""
    w = np.zeros_like(ref.dense["weights"])
    w[ref.dense["order"]] = ref.dense["weights"]
    return (w > 0).any(axis=1), w > 0


def _member_tiles(ref, i, tile_of_pixel):
    """The tiles whose list holds Gaussian i (input order)."""
    k = ref.dense["order"].tolist().index(i)
    return set(tile_of_pixel[ref.dense["member"][k]].tolist())


def _evaluated(ref):
    """(P, N) in input order: the pair is in the pixel's tile list and the pixel had not stopped before it."""
    d = ref.dense
    N = d["member"].shape[1]
    c = d["member"] & np.concatenate([np.ones((1, N), bool), d["alive"][:-1]], 0)
    out = np.zeros_like(c)
    out[d["order"]] = c
    return out


@pytest.mark.parametrize("case", CASES + TILE_CASES, ids=_id)
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
        f, fl = er.mutual_rule(cls, case[0])
        # the two float32 restatements judge each other with the undoubled constants
        r_o, _ = ref.ratios(cls, ref.oracle[cls], f, fl, e32_from=("d32",))
        r_d, _ = ref.ratios(cls, ref.d32[cls], f, fl, e32_from=("oracle",))
        assert (r_o <= 1.0).all() and (r_d <= 1.0).all(), (cls, float(r_o.max()), float(r_d.max()),
                                                             ref.group_name(cls, int(np.argmax(np.maximum(r_o, r_d)))))
    # the oracle under the rule the product is held to, exact zeros included; dense32 takes the same zero decisions
    ref.check("oracle", ref.oracle)
    for cls in ref.classes:
        _, zd = ref.ratios(cls, ref.d32[cls], *er.rule(cls, case[0]))
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


@pytest.mark.parametrize("case", TILE_CASES, ids=_id)
def test_tile_scenes_are_what_their_names_say(case):
    ref = er.reference(case)
    which, inp, d = case[5].kind, ref.inp, ref.dense
    W, H = inp.image_width, inp.image_height
    lists = er.tile_lists(ref)
    gy, gx = lists.shape
    blended, where = _blended(ref)
    tile_of_pixel = (np.arange(H)[:, None] // 16 * gx + np.arange(W)[None] // 16).reshape(-1)
    tiles_blended = lambda i: set(tile_of_pixel[where[i]].tolist())
    grad_classes = [c for c in ref.classes if c not in er.PIXEL_CLASSES]
    # (dL_drotations of an isotropic Gaussian is zero up to rounding: left out for the classes built isotropic)
    nonzero_row = lambda i, but=(): all(np.abs(ref.d64[c][i]).max() > 0 for c in grad_classes if c not in but)
    zero_row = lambda i: all(np.abs(ref.d64[c][i]).max() == 0 and np.abs(ref.oracle[c][i]).max() == 0 for c in grad_classes)
    # the dense tile: a raw list beyond every batch size, next to lists shorter than one backward chunk
    tx, ty = er.DENSE_TILE[which]
    assert len(_rows(ref, "dense_tile")) == er.N_DENSE[which] and lists[ty, tx] >= max(er.DENSE_LIST, er.N_DENSE[which])
    assert all(blended[i] and tiles_blended(i) == {ty * gx + tx} for i in _rows(ref, "dense_tile"))
    for ny in range(max(0, ty - 1), min(gy, ty + 2)):
        for nx in range(max(0, tx - 1), min(gx, tx + 2)):
            assert (nx, ny) == (tx, ty) or lists[ny, nx] < er.CHK, (nx, ny, int(lists[ny, nx]))
    # corners: blended in four tiles each
    assert len(_rows(ref, "corner")) == (12 if which == "t1" else 4)
    for i in _rows(ref, "corner"):
        assert len(tiles_blended(i)) == 4, (i, tiles_blended(i))
    if which == "t1":
        assert (gx, gy) == (7, 3) and W - 16 * (gx - 1) == 1 and H - 16 * (gy - 1) == 1
        # spanning: one rect over every tile, blended in every tile, first and last of every list
        front, back = _rows(ref, "spanning_front")[0], _rows(ref, "spanning_back")[0]
        for i in (front, back):
            assert ref.tiles_touched[i] == gx * gy and np.asarray(inp.opacities).reshape(-1)[i] <= np.float32(0.1) and nonzero_row(i)
        # (the rear one not in the opaque tile, nor in the strip of one pixel row under it, which the opaque Gaussians end as well)
        assert len(tiles_blended(front)) == gx * gy and len(tiles_blended(back)) >= gx * gy - 2
        vis = [i for i in d["order"].tolist() if ref.radii[i] > 0]
        assert vis[0] == front and vis[-1] == back
        # the opaque tile: every pixel's walk ends on the Gaussians at the front, within a quarter of the list
        ox, oy = er.OPAQUE_TILE
        in_tile = tile_of_pixel == oy * gx + ox
        assert not d["alive"][-1][in_tile].any(), "a pixel of the opaque tile that never stops"
        pos = {g: k for k, g in enumerate(i for i in d["order"].tolist() if (oy * gx + ox) in _member_tiles(ref, i, tile_of_pixel))}
        assert len(pos) == lists[oy, ox]
        last = max(pos[i] + 1 for i in range(len(blended)) if where[i][in_tile].any())
        assert 4 * last <= lists[oy, ox], (last, int(lists[oy, ox]))
        if not case[5].mask_only:
            n_contrib = ref.fwd.state.field(so.F_N_CONTRIB).reshape(-1)[in_tile]
            assert int(n_contrib.max()) == last
        for i in _rows(ref, "hidden"):
            assert ref.radii[i] > 0 and not blended[i] and zero_row(i)
        # the one-pixel tile column and tile row: Gaussians blended there alone, with gradients
        px, py = np.arange(W * H) % W, np.arange(W * H) // W
        for cls, coord, edge in (("last_column", px, W - 1), ("last_row", py, H - 1)):
            assert len(_rows(ref, cls)) == 3
            for i in _rows(ref, cls):
                assert blended[i] and (coord[where[i]] == edge).all() and nonzero_row(i, ("dL_drotations",)), (cls, i)
    else:
        assert (gx, gy) == (12, 2) and H - 16 * (gy - 1) == 1
        band = list(er.EMPTY_BAND)
        ranges = ref.fwd.state.field(so.F_RANGES).reshape(-1, 2)
        assert len(band) >= 3 and (lists[0, band] == 0).all() and (ranges[band] == 0).all()
        assert lists[0, band[0] - 1] > 0 and lists[0, band[-1] + 1] > 0
        assert (tx, ty) == (gx - 2, 0)       # the last full tile of the top tile row
    # the runs the range scan cuts: not those of equal tile counts, one of a single tile, one of three or more
    model, equal = er.model_runs(ref)
    assert sum(a != b for a, b in zip(model[1:8], equal[1:8])) >= 3, (model, equal)
    lengths = np.diff(model)
    assert (lengths == 1).any() and lengths.max() >= 3, model


def test_tile_rule_sees_a_contribution_lost_from_one_tile():
    """What the many-tile tests are for: the rows of the two spanning Gaussians are sums over all 21 tiles, and a kernel that loses
    ONE tile's share of such a row -- the dense tile's, that of the 1 x 16 tile (6, 0), or that of the single pixel that is tile
    (6, 2) -- is rejected on that row in every gradient class.  The share is the dense float64 gradient of the loss restricted to
    the tile; it is taken out of a copy of the oracle's row."""
    import torch
    ref = er.reference(er.tile_case("t1", "rgb"))
    inp = ref.inp
    W, H = inp.image_width, inp.image_height
    gx = (W + 15) // 16
    tile_of_pixel = np.arange(H)[:, None] // 16 * gx + np.arange(W)[None] // 16
    grad_classes = [c for c in ref.classes if c not in er.PIXEL_CLASSES]
    rows = [_rows(ref, "spanning_front")[0], _rows(ref, "spanning_back")[0]]
    for tx, ty in (er.DENSE_TILE["t1"], (6, 0), (6, 2)):
        dL = (ref.dL * (tile_of_pixel == ty * gx + tx)[None]).astype(np.float32)
        share, _, _ = er._dense(inp, dL, None, torch.float64, True, False)
        for cls in grad_classes:
            mutated = ref.oracle[cls].copy()
            mutated[rows] -= share[cls][rows]
            r, _ = ref.ratios(cls, mutated, *er.rule(cls, "tiles"))
            print(f"tile ({tx}, {ty}) lost, {cls}: error / bound {r[rows[0]]:.1f} (front) {r[rows[1]]:.1f} (back)")
            assert (r[rows] > 1.0).all(), (tx, ty, cls, r[rows])
            assert (np.delete(r, rows) <= 1.0).all()
