"""2D-to-3D score lifting on the GPU (seganygaussians_amd/lifting.py, csrc/lift.h): per-Gaussian votes against the dense float64
reference per row, over reused buffers, on scenes of many tiles and long lists against the CPU oracle's backward, and the
multi-view mask against a restatement of the reference's loop.

votes[g, k] = sum_p alpha_g(p) T_g(p) scores[k, p] is mathematically dL_dcolors of the blend backward with dL_dpixels = scores (for
one channel: dL_dmask of the mask-only pair), so every comparison uses that class's existing rule and constants: the per-row rule
of tests/raster_edge_ref.py (FACTOR / FLOOR of er.rule, E32 from the oracle and dense32, zero rows exact) and hp.compare_gradients'
criterion.  No tolerance is introduced here."""
import math

import numpy as np
import pytest
import torch

import seganygaussians_amd
from oracle import saga_oracle as so
from seganygaussians_amd import lifting, scenes
from seganygaussians_amd import rasterizer as R
from tests import helpers as hp
from tests import raster_edge_ref as er

seganygaussians_amd.install_dropin()
pytestmark = pytest.mark.gpu


def _geometry(g):
    """The geometry arguments of lift_scores from a hp.GpuRun's tensors (an absent one is an empty tensor there)."""
    opt = lambda t: t if t.numel() else None
    return dict(scales=opt(g.scales), rotations=opt(g.rots), cov3D_precomp=opt(g.cov), viewmatrix=g.view, projmatrix=g.proj,
                tanfovx=g.inp.tanfovx, tanfovy=g.inp.tanfovy, scale_modifier=g.inp.scale_modifier)


def _name(case, full_lists):
    return f"lift {case[0]} {case[1]}x{case[2]} C{case[3]} {case[5].kind or ''}{case[5].L or ''} P{case[5].P} full_lists={full_lists}"


def _class_and_scores(ref):
    if ref.case[5].mask_only:
        return "dL_dmask", np.asarray(ref.dLm, np.float32).reshape(1, ref.inp.image_height, ref.inp.image_width)
    return "dL_dcolors", np.asarray(ref.dL, np.float32)


def _merge(worst, w):
    for k, v in w.items():
        worst[k] = max(worst.get(k, 0.0), v)


def _lift_case(case, full_lists, worst):
    ref = er.reference(case)
    cls, scores = _class_and_scores(ref)
    g = hp.GpuRun(ref.inp)
    s = torch.as_tensor(scores).to(g.dev)
    P, K = g.P, s.shape[0]
    name = _name(case, full_lists)
    with R.forward_flags(full_lists=full_lists, exact_exp=True):
        votes, st = lifting.lift_scores(s, g.means3D, g.opac, return_state=True, **_geometry(g))
        filled = torch.full((P, K), 7.0, device=g.dev)
        assert lifting.lift_scores(s, g.means3D, g.opac, out=filled, **_geometry(g)) is filled
    assert votes.shape == (P, K)
    np.testing.assert_array_equal(st.radii.cpu().numpy(), ref.radii, err_msg=name + ": radii")
    if full_lists:
        assert st.num_rendered == ref.fwd.num_rendered, name
    _merge(worst, ref.check(name, {cls: votes.cpu().numpy()}, classes=[cls]))
    untouched = np.abs(ref.d64[cls]).max(axis=1) == 0
    assert (filled.cpu().numpy()[untouched] == 7.0).all(), name + ": a row that blends nowhere was written"


EDGE_CONFIGS = ["mask_only", "rgb", "cov3d", "c16", "c17", "c32", "modifier", "c48", "c64"]
LIST_CONFIGS = ["mask_only", "rgb", "c17", "c64"]
SMALL_CONFIGS = ["rgb", "c16", "c64"]
FULL = pytest.mark.parametrize("full_lists", [True, False], ids=["full", "lean"])


@FULL
@pytest.mark.parametrize("cfg", EDGE_CONFIGS)
def test_edge_scene_against_dense64(cfg, full_lists):
    """The 37 x 21 scene of designed classes: every channel-block shape (1, 3, 16, 17, 32, 48, 64 channels), the precomputed
    covariance and the scale modifier."""
    worst = {}
    _lift_case(er.edge_case(cfg), full_lists, worst)


@FULL
@pytest.mark.parametrize("cfg", LIST_CONFIGS)
def test_list_lengths_against_dense64(cfg, full_lists):
    """The 16 x 16 scene whose list ends one below, at and one above every kernel batch size (CHK, the lift's chunk, and the 64
    entries of its scan block among them), for the contributing entries and for the raw list."""
    worst = {}
    for case in er.list_cases(cfg):
        _lift_case(case, full_lists, worst)
    print(f"worst error / bound, lift {cfg} lists full_lists={full_lists}: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@FULL
@pytest.mark.parametrize("cfg", SMALL_CONFIGS)
def test_small_sizes_one_gaussian_and_all_culled(cfg, full_lists):
    """16 x 16, 1 x 1, 40 x 5 and 5 x 40 images, P = 1, and a scene in which every Gaussian is culled."""
    worst = {}
    for case in er.small_cases(cfg):
        _lift_case(case, full_lists, worst)


@FULL
@pytest.mark.parametrize("tile", [("t1", "c64"), ("t2", "c32")], ids=["t1-c64", "t2-c32"])
def test_many_tile_scenes_against_dense64(tile, full_lists):
    """The 97 x 33 and 177 x 17 scenes of er.tile_cases() (21 and 24 tiles: a vote row summed from every tile, XCD runs of uneven
    length, empty ranges between occupied tiles, one-pixel tile columns and rows) under their table, er.MUTUAL_TILES."""
    worst = {}
    _lift_case(er.tile_case(*tile), full_lists, worst)


def test_reuse_reads_the_buffers_of_any_forward():
    """Lifts over the state of an earlier lift, of a feature forward and of a mask-only forward of the same view: each under the rule
    of the first test, and none of them changes a byte of the three buffers."""
    case = er.edge_case("c32")
    ref = er.reference(case)
    g = hp.GpuRun(ref.inp)
    inp = ref.inp
    W, H = inp.image_width, inp.image_height
    s = torch.as_tensor(np.asarray(ref.dL, np.float32)).to(g.dev)
    with R.forward_flags(full_lists=False, exact_exp=True):
        _, st_lift = lifting.lift_scores(s, g.means3D, g.opac, return_state=True, **_geometry(g))
        fw = hp.GpuRun(inp).forward(full_lists=False, exact_exp=True)
        st_fwd = lifting.state_of_forward(fw.num_rendered, fw.radii, fw.geom, fw.binning, fw.img, W, H)
        mask = torch.rand(g.P, device=g.dev)
        nr, _, radii, geom, binning, img = R.rasterize_mask_gaussians_native(
            g.means3D, g.opac, mask, g.scales, g.rots, inp.scale_modifier, g.cov, g.view, g.proj, inp.tanfovx, inp.tanfovy, H, W,
            False, False)
        st_mask = lifting.state_of_forward(nr, radii, geom, binning, img, W, H)
    for what, st in (("lift", st_lift), ("forward", st_fwd), ("mask forward", st_mask)):
        before = [b.clone() for b in (st.geom, st.binning, st.img)]
        votes = lifting.lift_scores(s, g.means3D, g.opac, state=st)
        torch.cuda.synchronize()
        for b, a, field in zip(before, (st.geom, st.binning, st.img), ("geometry", "binning", "image")):
            assert torch.equal(a, b), f"reuse over the state of a {what}: the {field} buffer changed"
        ref.check(f"lift reuse over a {what}", {"dL_dcolors": votes.cpu().numpy()}, classes=["dL_dcolors"])
    # the forward's own backward still runs on its buffers after the lift
    got = fw.backward(ref.dL)["dL_dcolors"]
    ref.check("backward after a lift over its buffers", {"dL_dcolors": got}, classes=["dL_dcolors"])


_ORACLE = {}


def _oracle(scene, inp, dL):
    """The CPU oracle's forward and backward of a scene, computed once per process."""
    if scene not in _ORACLE:
        fwd = so.forward(inp)
        _ORACLE[scene] = (fwd, so.backward(inp, fwd, dL))
    return _ORACLE[scene]


_MANY = {
    "cfg1": lambda: hp.inputs_from_config("cfg1"),
    "long_lists": lambda: hp.make_inputs(20_000, 96, 64, 3, seed=14, focal=40.0, log_scale=math.log(0.2), log_scale_std=0.4,
                                         z_range=(2.0, 9.0)),
}


@FULL
@pytest.mark.parametrize("scene", list(_MANY))
def test_many_tiles_and_long_lists_against_the_oracle(scene, full_lists):
    """cfg1: 256 tiles, more than the eight XCD runs the tiles are dealt over.  long_lists: full tile lists between 2048 and 12288
    entries -- many scan blocks and ring wrap-arounds per item, walks that end long before the list does."""
    inp = _MANY[scene]()
    H, W = inp.image_height, inp.image_width
    dL = scenes.make_grad_image(3, H, W, seed=2)
    fwd, bwd = _oracle(scene, inp, dL)
    g = hp.GpuRun(inp)
    with R.forward_flags(full_lists=full_lists, exact_exp=True):
        votes, st = lifting.lift_scores(torch.as_tensor(dL).to(g.dev), g.means3D, g.opac, return_state=True, **_geometry(g))
    np.testing.assert_array_equal(st.radii.cpu().numpy(), fwd.radii)
    if full_lists:
        assert st.num_rendered == fwd.num_rendered
        from seganygaussians_amd import _lib
        _, off = _lib.image_layout(W, H)
        tiles = ((W + 15) // 16) * ((H + 15) // 16)
        r = st.img.cpu().numpy()[off["ranges"]:off["ranges"] + 8 * tiles].view(np.uint32).reshape(-1, 2).astype(np.int64)
        longest = int((r[:, 1] - r[:, 0]).max())
        assert tiles == 256 if scene == "cfg1" else 2048 < longest <= 12288, (tiles, longest)
    rep = hp.compare_gradients({"dL_dcolors": votes.cpu().numpy()}, bwd, rtol=hp.RTOL, flip_frac=hp.GRAD_FLIP_FRAC)
    print(f"lift {scene} full_lists={full_lists}: fraction outside tolerance {rep}")


class _Camera:
    """The attributes of the reference's Camera (scene/cameras.py) that get_3d_mask and render_mask read."""

    def __init__(self, cam, dev):
        self.image_width, self.image_height = cam.image_width, cam.image_height
        self.FoVx, self.FoVy = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
        self.world_view_transform = torch.as_tensor(cam.viewmatrix).to(dev)
        self.full_proj_transform = torch.as_tensor(cam.projmatrix).to(dev)
        self.camera_center = torch.as_tensor(cam.campos).to(dev)


def _reference_loop(cameras, scores, means3D, opac, scales, rots):
    """clip_utils.get_3d_mask (clip_utils/__init__.py:291-330) through gaussian_renderer.render_mask (:108-190), restated: per
    view a render of the zero mask repeated to three colours_precomp channels (:153, :156) over a zero background (:304), the score
    image resized to the render (:309), loss = -(target * render).sum() (:311), backward (:313), tmp_mask -= grad (:319)."""
    import diff_gaussian_rasterization as dgr
    P = means3D.shape[0]
    tmp_mask = torch.zeros((P, 1), device=means3D.device, requires_grad=True)
    for view, gt_score in zip(cameras, scores):
        if gt_score is None:
            continue
        settings = dgr.GaussianRasterizationSettings(
            image_height=int(view.image_height), image_width=int(view.image_width), tanfovx=math.tan(view.FoVx * 0.5),
            tanfovy=math.tan(view.FoVy * 0.5), bg=torch.zeros(3, device=means3D.device), scale_modifier=1.0,
            viewmatrix=view.world_view_transform, projmatrix=view.full_proj_transform, sh_degree=0, campos=view.camera_center,
            prefiltered=False, debug=False)
        screenspace_points = torch.zeros_like(means3D, requires_grad=True) + 0
        mask3 = tmp_mask.squeeze().unsqueeze(-1).repeat([1, 3])
        rendered, _ = dgr.GaussianRasterizer(raster_settings=settings)(
            means3D=means3D, means2D=screenspace_points, shs=None, colors_precomp=mask3, opacities=opac, scales=scales,
            rotations=rots, cov3D_precomp=None)
        target = torch.nn.functional.interpolate(gt_score.unsqueeze(0).unsqueeze(0).float(), size=rendered.shape[-2:],
                                                 mode="bilinear").squeeze(0)
        loss = -(target * rendered).sum()
        loss.backward()
        grad_score = tmp_mask.grad.clone()
        with torch.no_grad():
            tmp_mask = tmp_mask - grad_score
        tmp_mask.requires_grad = True
    return tmp_mask.detach()


def test_multi_view_mask_is_the_reference_loops():
    """vote_3d_mask over three orbit cameras (the middle one skipped), half-resolution score images with exact zeros: 3 votes is the
    reference loop's accumulator within hp.RTOL, and zero EXACTLY where that is zero, so the thresholded masks are equal.  Both
    sides take every alpha >= 1/255 decision with expf, and the lift's T recurrence is the forward's."""
    dev = torch.device("cuda:0")
    W, H, P, focal = 160, 120, 3000, 130.0
    sc = scenes.make_scene(P, W, H, focal, 3, math.log(0.05), 0.6, seed=5)
    cams = [_Camera(scenes.orbit_camera(W, H, focal, a, t), dev) for a, t in ((-0.25, 0.0), (0.0, 0.05), (0.3, -0.04))]
    rng = np.random.default_rng(8)
    scores = []
    for k in range(3):
        v = rng.uniform(0.25, 1.0, (H // 2, W // 2)).astype(np.float32)
        v[rng.uniform(size=v.shape) < 0.5] = 0.0
        v[:, : W // 8] = 0.0   # a band of the image without any score: Gaussians that only reach it get no vote
        scores.append(torch.as_tensor(v).to(dev))
    scores[1] = None
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(dev)
    means3D, opac, scales, rots = t(sc.means3D), t(sc.opacities), t(sc.scales), t(sc.rotations)
    with R.forward_flags(exact_exp=True):
        mask, votes = lifting.vote_3d_mask(cams, scores, means3D, opac, scales=scales, rotations=rots)
        want = _reference_loop(cams, scores, means3D, opac, scales, rots)
    assert mask.shape == votes.shape == want.shape == (P, 1) and mask.dtype == torch.bool
    got, want = votes.cpu().numpy(), want.cpu().numpy()
    print(f"multi-view mask: {int((want > 0).sum())} of {P} selected, {int((want == 0).sum())} without a vote")
    assert 0 < (want > 0).sum() < P and (want == 0).any()
    hp.assert_close("3 votes", 3.0 * got, want, rtol=hp.RTOL)
    np.testing.assert_array_equal(got == 0, want == 0, err_msg="rows without a vote")
    np.testing.assert_array_equal(mask.cpu().numpy(), want > 0, err_msg="the thresholded mask")
