"""GPU tests of the viewer frame (seganygaussians_amd/viewer.py, csrc/viewer.h) against the float64 restatement of
tests/viewer_ref.py, whose docstring derives every bound used here.

Frame: mask and score equal select_by_similarity(..., pre="eps", half_shift=True) bit for bit; every frame value lies within the
bound of its enabled components; the pixels whose float64 margin |t_k - threshold| is inside the band are excused where the decision
shows, and may be at most 1 % of a case.  Moments: |d mean| <= (C / 2 + 4) 2^-24, |d cov| <= (B + 2 C + 32) 2^-24 with
B = mi_view_moments_block(); the basis against Weyl's and Davis-Kahan's bounds on the planted case."""
import functools

import numpy as np
import pytest
import torch

from seganygaussians_amd import _lib
from seganygaussians_amd.segmentation import select_by_similarity, similarity_scores
from seganygaussians_amd.viewer import (ViewerFrame, feature_covariance, feature_pca_basis, gui_pca_sample, prompt_features,
                                        viewer_frame)
from tests import segmentation_ref as ref
from tests import viewer_ref as vr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CAP = 0.01
GUARD = 64


def dev(t):
    return None if t is None else t.to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def view_case(shape, C, Q, seed):
    return vr.make_view_case(shape, C, Q, seed)


def run_frame(c, thr, modes, preview, cluster, **kw):
    return viewer_frame(dev(c.features), dev(c.rgb), proj=dev(c.proj), queries=dev(c.queries), gates=dev(c.gates), threshold=thr,
                        cluster_rgb=dev(cluster), modes=modes, preview=preview, **kw)


def check_frame(c, thr, modes, preview, cluster, what=""):
    got = run_frame(c, thr, modes, preview, cluster)
    want = vr.frame64(c.features, c.rgb, c.proj, c.queries, c.gates, thr, cluster, modes, preview)
    H, W = c.features.shape[1:]
    assert isinstance(got, ViewerFrame) and got.frame.shape == (H, W, 3) and got.frame.dtype == torch.float32 and got.frame.is_contiguous()
    worst, share = vr.frame_errors(got.frame.cpu(), want)
    print(f"frame {what} {tuple(c.features.shape)} Q={0 if c.queries is None else c.queries.shape[0]} modes={modes} preview={preview} "
          f"cluster={cluster is not None}: worst error / bound = {worst:.3f}, excused {share:.5f}")
    if c.queries is None:
        assert got.mask is None and got.score is None
    else:
        mask, score = select_by_similarity(dev(c.features), dev(c.queries), thr, dev(c.gates), pre="eps", half_shift=True)
        assert got.mask.dtype == torch.bool and got.mask.shape == (H, W) and got.score.dtype == torch.float32
        assert torch.equal(got.mask, mask) and torch.equal(bits(got.score), bits(score))
        assert not (got.mask.cpu() != want.mask)[~want.band].any()
    assert worst <= 1.0
    assert share <= CAP
    return got


# ---- the frame ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", vr.FRAME_CASES, ids=lambda c: f"{c[0]}-C{c[1]}-Q{c[2]}")
def test_frame_shapes_channels_queries(case):
    shape, C, Q, seed, thr = case
    c = view_case(shape, C, Q, seed)
    check_frame(c, thr, vr.MODES, True, c.cluster_rgb)
    check_frame(c, thr, ("pca", "similarity"), False, None)
    check_frame(c, thr, ("similarity",), False, None)
    check_frame(c, thr, (), True, None)


@pytest.mark.parametrize("preview", [False, True])
@pytest.mark.parametrize("with_cluster", [False, True])
def test_every_mode_subset(preview, with_cluster):
    shape, C, Q, seed, thr = vr.MODE_CASE
    c = view_case(shape, C, Q, seed)
    no_click = vr.make_view_case(shape, C, 0, seed)
    for modes in vr.ALL_MODE_SUBSETS:
        check_frame(c, thr, modes, preview, c.cluster_rgb if with_cluster else None)
        check_frame(no_click, thr, modes, preview, c.cluster_rgb if with_cluster else None, what="no click")


def test_modes_as_the_gui_names_them():
    """A string, a list, a set and repeats name the same frame; rgb and cluster components are exact copies."""
    shape, C, Q, seed, thr = vr.MODE_CASE
    c = view_case(shape, C, Q, seed)
    a = run_frame(c, thr, "cluster", False, c.cluster_rgb).frame
    assert torch.equal(a.cpu(), c.cluster_rgb.permute(1, 2, 0))
    assert torch.equal(run_frame(c, thr, ["cluster", "cluster"], False, c.cluster_rgb).frame, a)
    assert torch.equal(run_frame(c, thr, {"rgb"}, False, None).frame.cpu(), c.rgb.permute(1, 2, 0))
    assert torch.equal(run_frame(c, thr, (), False, c.cluster_rgb).frame.cpu(), c.rgb.permute(1, 2, 0))
    got = run_frame(c, thr, ("rgb",), True, None)
    assert torch.equal(got.frame.cpu(), c.rgb.permute(1, 2, 0) * got.mask.cpu().unsqueeze(-1))


def test_pca_component_is_the_scores_call():
    """The "pca" component against clip(similarity_scores(..., post=False) * 0.5 + 0.5, 0, 1): the same fmaf chain, so at most one
    float32 rounding of the multiply-add apart."""
    for shape, C, seed in (((6, 65), 33, 8), ((4, 256), 64, 9), ((5, 13), 3, 7), ((2, 130), 256, 11)):
        c = view_case(shape, C, 0, seed)
        got = run_frame(c, 0.5, ("pca",), False, None).frame
        s = similarity_scores(dev(c.features), dev(c.proj.t().contiguous()), pre="eps", post=False).permute(1, 2, 0)
        want = torch.clip(s * 0.5 + 0.5, 0, 1)
        assert (got - want).abs().max().item() <= 2.0 ** -24


def test_zero_feature_rows():
    shape, C, Q, seed, thr = vr.MODE_CASE
    c = vr.make_view_case(shape, C, Q, seed)
    c.features[:, 2, 5] = 0.0
    c.features[:, 0, 0] = 0.0
    got = check_frame(c, 0.4, vr.MODES, True, None)
    # u = 0: t = 1/2 for every query, the PCA image is mid-grey
    assert got.mask[2, 5].item() and got.score[2, 5].item() == 0.5
    pca = run_frame(c, 0.4, ("pca",), False, None).frame
    assert pca[2, 5].tolist() == [0.5, 0.5, 0.5] and pca[0, 0].tolist() == [0.5, 0.5, 0.5]
    got = check_frame(c, 0.6, ("rgb", "similarity"), True, None)
    assert not got.mask[2, 5].item() and got.score[2, 5].item() == 0.0
    assert got.frame[2, 5].tolist() == [0.0, 0.0, 0.25]                  # (rgb * 0 + jet(0)) / 2


def test_unaligned_feature_base_and_out_reuse():
    for shape, C, Q, seed, thr in (((8, 8), 32, 16, 6, 0.7), ((2, 6), 31, 4, 4, 0.5), ((6, 342), 1, 5, 15, 0.5)):
        c = view_case(shape, C, Q, seed)
        want = run_frame(c, thr, vr.MODES, True, c.cluster_rgb)
        N = shape[0] * shape[1]
        for off in (1, 2, 3):        # a base 4, 8 and 12 bytes past a 16-byte boundary
            flat = torch.zeros(off + C * N, device=DEV)
            feats = flat[off:].view((C,) + shape)
            feats.copy_(c.features)
            assert feats.is_contiguous() and feats.data_ptr() % 16 == 4 * off
            got = viewer_frame(feats, dev(c.rgb), proj=dev(c.proj), queries=dev(c.queries), gates=dev(c.gates), threshold=thr,
                               cluster_rgb=dev(c.cluster_rgb), modes=vr.MODES, preview=True)
            for a, b in zip(got, want):
                assert torch.equal(bits(a.float()), bits(b.float()))
        out = torch.full(shape + (3,), -7.0, device=DEV)
        got = run_frame(c, thr, vr.MODES, True, c.cluster_rgb, out=out)
        assert got.frame is out and torch.equal(out, want.frame)
        got = run_frame(c, thr, ("rgb",), False, None, out=out)          # the same buffer, the next frame
        assert got.frame is out and torch.equal(out.cpu(), c.rgb.permute(1, 2, 0))


def test_frame_runs_are_bit_identical():
    c = view_case((5, 413), 32, 4, 14)
    a = run_frame(c, 0.55, vr.MODES, True, c.cluster_rgb)
    b = run_frame(c, 0.55, vr.MODES, True, c.cluster_rgb)
    for x, y in zip(a, b):
        assert torch.equal(bits(x.float()), bits(y.float()))


@pytest.mark.parametrize("case", [((5, 13), 33, 5, 7, 0.5), ((6, 342), 1, 5, 15, 0.5), ((2, 6), 31, 4, 4, 0.5)], ids=lambda c: f"{c[0]}-C{c[1]}")
def test_frame_guard_words(case):
    """The C-ABI call with every output inside a larger buffer: nothing outside frame [N][3], mask [N] and score [N] changes."""
    shape, C, Q, seed, thr = case
    c = view_case(shape, C, Q, seed)
    N = shape[0] * shape[1]
    L = _lib.load()
    frame = torch.full((GUARD + 3 * N + GUARD,), -3.0, device=DEV)
    score = torch.full((GUARD + N + GUARD,), -5.0, device=DEV)
    mask = torch.full((GUARD + N + GUARD,), 77, device=DEV, dtype=torch.uint8)
    f, rgb, clu, proj, q, g = (dev(t).contiguous() for t in (c.features, c.rgb, c.cluster_rgb, c.proj, c.queries, c.gates))
    rc = L.mi_view_frame(N, C, f.data_ptr(), rgb.data_ptr(), clu.data_ptr(), proj.data_ptr(), Q, q.data_ptr(), g.data_ptr(), thr, 15, 1,
                         frame.data_ptr() + 4 * GUARD, mask.data_ptr() + GUARD, score.data_ptr() + 4 * GUARD,
                         torch.cuda.current_stream(DEV).cuda_stream)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    want = run_frame(c, thr, vr.MODES, True, c.cluster_rgb)
    assert torch.equal(frame[GUARD:-GUARD], want.frame.reshape(-1)) and torch.equal(score[GUARD:-GUARD], want.score.reshape(-1))
    assert torch.equal(mask[GUARD:-GUARD].bool(), want.mask.reshape(-1)) and int(mask[GUARD:-GUARD].max()) <= 1
    for buf, word in ((frame, -3.0), (score, -5.0), (mask, 77)):
        assert (buf[:GUARD] == word).all() and (buf[-GUARD:] == word).all()


# ---- moments --------------------------------------------------------------------------------------------------------------------

def moment_block():
    return int(_lib.load().mi_view_moments_block())


def check_moments(feats, index, pre, what=""):
    B = moment_block()
    mean, cov, n = feature_covariance(dev(feats), None if index is None else dev(index), pre=pre)
    wmean, wcov, wn = vr.moments64(feats, index, pre)
    C = wmean.numel()
    assert n == wn and mean.shape == (C,) and cov.shape == (C, C) and mean.dtype == cov.dtype == torch.float64 and mean.is_cuda
    bm, bc = vr.moment_bounds(C, B)
    scale = 1.0
    if pre == "none":        # rows are not unit rows: the bounds scale with the largest |u| and its square
        scale = float(ref.rows_of(feats)[0].double().norm(dim=-1).max().clamp_min(1.0))
    em = (mean.cpu() - wmean).abs().max().item() / (bm * scale)
    ec = (cov.cpu() - wcov).abs().max().item() / (bc * scale * scale)
    print(f"moments {what} {tuple(feats.shape)} n={n} pre={pre}: mean error / bound = {em:.3f}, cov error / bound = {ec:.3f}")
    assert em <= 1.0 and ec <= 1.0
    assert torch.equal(cov, cov.t())
    return mean, cov


def moment_rows(layout, n, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, C, generator=g) + 0.5 if layout == "points" else torch.randn(C, 1, n, generator=g) + 0.5


@pytest.mark.parametrize("C", [1, 2, 3, 31, 32, 33, 64, 65, 256])
@pytest.mark.parametrize("layout", ["points", "image"])
def test_moments_over_rows_and_channels(layout, C):
    B = moment_block()
    pres = ("eps", "l2", "none")
    for i, n in enumerate(sorted({1, 2, 31, 32, 33, 63, 64, 65, B - 1, B, B + 1, 3 * B + 7})):
        feats = moment_rows(layout, n, C, seed=1000 * C + n)
        check_moments(feats, None, pres[i % 3], what=layout)
        table = moment_rows(layout, 3 * B + 7, C, seed=77 + C)
        g = torch.Generator().manual_seed(n)
        index = torch.randint(0, 3 * B + 7, [n], generator=g)           # repeats as randint produces them
        check_moments(table, index, pres[(i + 1) % 3], what=layout + " indexed")


@pytest.mark.parametrize("case", [("points", 70_001, 32), ("points", 30_000, 64), ("image", 30_001, 33), ("points", 4000, 256),
                                  ("image", 2500, 65), ("points", 66_000, 3)], ids=lambda c: f"{c[0]}-{c[1]}-C{c[2]}")
def test_moments_many_workgroups(case):
    """More tiles than workgroups (the tile loop of a workgroup), several groups of output blocks, both loads of the points layout."""
    layout, n, C = case
    feats = moment_rows(layout, n, C, seed=n + C)
    check_moments(feats, None, "eps", what=layout)
    index = gui_pca_sample(n, n // 2 + 1)
    m1, c1 = check_moments(feats, index, "eps", what=layout + " sampled")
    m2, c2 = feature_covariance(dev(feats), dev(index))[:2]
    assert torch.equal(m1, m2) and torch.equal(c1, c2)                   # two runs, the same bits


def test_moments_pre_modes_index_forms_and_unaligned_base():
    feats = moment_rows("points", 103, 32, seed=5)
    for pre in ("none", "l2", "eps"):
        check_moments(feats, None, pre)
        check_moments(feats, torch.tensor([7]), pre, what="one row")
        check_moments(feats, torch.tensor([5, 5, 5, 102, 0, 5]), pre, what="repeats")
    m, c = check_moments(feats, torch.arange(103), "eps")
    m0, c0 = check_moments(feats, None, "eps")
    assert torch.equal(m, m0) and torch.equal(c, c0)                      # the identity index is no index
    m1, c1, _ = feature_covariance(dev(feats), torch.arange(103), pre="eps")   # an index on the host is moved
    assert torch.equal(m1, m0) and torch.equal(c1, c0)
    flat = torch.zeros(1 + 103 * 32, device=DEV)
    view = flat[1:].view(103, 32)
    view.copy_(feats)
    m2, c2, _ = feature_covariance(view, None, pre="eps")                # the scalar loads fill the same tile
    assert torch.equal(m2, m0) and torch.equal(c2, c0)
    img = feats.t().contiguous().reshape(32, 1, 103)
    m3, c3 = check_moments(img, None, "eps", what="image")
    assert torch.equal(m3, m0) and torch.equal(c3, c0)                    # the layouts share everything after the load


def test_moments_degenerate_rows():
    B = moment_block()
    C = 32
    one = moment_rows("points", 1, C, seed=9)
    same = one.expand(2 * B + 3, C).contiguous()
    zero = torch.zeros(B + 1, C)
    mixed = torch.cat([moment_rows("points", 40, C, seed=10), torch.zeros(3, C)])
    for feats in (one, same, zero, mixed):
        mean, cov = check_moments(feats, None, "eps")
        proj, w = feature_pca_basis(dev(feats), 3)
        assert proj.shape == (C, 3) and proj.dtype == torch.float32 and proj.is_cuda and w.shape == (3,) and w.dtype == torch.float64
        assert (proj.t().double().cpu() @ proj.double().cpu() - torch.eye(3, dtype=torch.float64)).abs().max() <= 1e-6
    mean, cov, _ = feature_covariance(dev(zero))
    assert not mean.any() and not cov.any()
    mean, cov, _ = feature_covariance(dev(same))
    bm, bc = vr.moment_bounds(C, B)
    assert cov.abs().max().item() <= bc


def test_moments_guard_words():
    """The C-ABI call with mean, cov and the workspace inside larger buffers: nothing outside them changes."""
    L = _lib.load()
    for layout, n, C in (("points", 103, 33), ("image", 2500, 65), ("points", 4000, 256)):
        feats = dev(moment_rows(layout, n, C, seed=3)).contiguous()
        nbytes = int(L.mi_view_moments_workspace_bytes(n, C))
        assert nbytes % 8 == 0
        ws = torch.full((GUARD + nbytes // 8 + GUARD,), -9.0, device=DEV, dtype=torch.float64)
        mean = torch.full((GUARD + C + GUARD,), -9.0, device=DEV, dtype=torch.float64)
        cov = torch.full((GUARD + C * C + GUARD,), -9.0, device=DEV, dtype=torch.float64)
        rc = L.mi_view_moments(0 if layout == "image" else 1, n, C, feats.data_ptr(), None, n, 2, ws.data_ptr() + 8 * GUARD, nbytes,
                               mean.data_ptr() + 8 * GUARD, cov.data_ptr() + 8 * GUARD, torch.cuda.current_stream(DEV).cuda_stream)
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        wmean, wcov, _ = feature_covariance(feats)
        assert torch.equal(mean[GUARD:-GUARD], wmean) and torch.equal(cov[GUARD:-GUARD], wcov.reshape(-1))
        for buf in (ws, mean, cov):
            assert (buf[:GUARD] == -9.0).all() and (buf[-GUARD:] == -9.0).all()
        rc = L.mi_view_moments(1, n, C, feats.data_ptr(), None, n, 2, ws.data_ptr() + 8 * GUARD, nbytes - 8, mean.data_ptr(), cov.data_ptr(), None)
        assert rc != 0 and "workspace" in _lib.last_error()


def basis_checks(proj, w, cov, wcov, n_components=3):
    """Orthonormality, the sign convention, Weyl's bound on the eigenvalues and Davis-Kahan's on the vectors."""
    proj = proj.double().cpu()
    assert (proj.t() @ proj - torch.eye(n_components, dtype=torch.float64)).abs().max() <= 1e-6
    k = proj.abs().argmax(dim=0)
    assert (proj.gather(0, k[None]) > 0).all()
    wproj, ww, w_all = vr.basis64(wcov, n_components)
    E = (cov.cpu() - wcov).norm().item()
    assert (w.cpu() - ww).abs().max().item() <= E
    gaps = vr.eigen_gaps(w_all, n_components)
    assert (gaps >= 0.2 * ww).all()
    cos = (proj * wproj).sum(0).clamp(-1.0, 1.0)
    angle = torch.atan2((proj - wproj * cos[None]).norm(dim=0), cos)
    print(f"basis: |E|_F = {E:.3e}, angles {angle.tolist()}, allowed {(2 * E / gaps + 1e-6).tolist()}")
    assert (angle <= 2 * E / gaps + 1e-6).all()


def test_planted_basis():
    feats = vr.planted_features(**vr.PLANTED)
    for index in (None, gui_pca_sample(feats.shape[0], 4000)):
        idx = None if index is None else dev(index)
        proj, w = feature_pca_basis(dev(feats), 3, index=idx)
        _, cov, _ = feature_covariance(dev(feats), idx)
        _, wcov, _ = vr.moments64(feats, index)
        basis_checks(proj, w, cov, wcov)
    proj3, w3 = feature_pca_basis(dev(feats), 3)
    proj1, w1 = feature_pca_basis(dev(feats), 1)
    assert proj1.shape == (32, 1) and torch.equal(proj1[:, 0], proj3[:, 0]) and torch.equal(w1, w3[:1])


def test_rendered_scene_end_to_end():
    """A small scene through the rasterizer: the basis of its feature table, a click, and the frame of its feature render."""
    from seganygaussians_amd import install_dropin
    from tests import helpers as hp
    install_dropin()
    import diff_gaussian_rasterization as rgb_mod
    import diff_gaussian_rasterization_contrastive_f as feat_mod
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(DEV)

    def render(mod, C):
        inp = hp.make_inputs(1500, 96, 64, C, seed=0)
        settings = mod.GaussianRasterizationSettings(
            image_height=inp.image_height, image_width=inp.image_width, tanfovx=inp.tanfovx, tanfovy=inp.tanfovy, bg=t(inp.bg),
            scale_modifier=1.0, viewmatrix=t(inp.viewmatrix), projmatrix=t(inp.projmatrix), sh_degree=0, campos=t(inp.campos),
            prefiltered=False, debug=False)
        means3D = t(inp.means3D)
        with torch.no_grad():
            out = mod.GaussianRasterizer(settings)(means3D=means3D, means2D=torch.zeros_like(means3D), shs=None,
                                                   colors_precomp=t(inp.colors_precomp), opacities=t(inp.opacities),
                                                   scales=t(inp.scales), rotations=t(inp.rotations), cov3D_precomp=None)
        return out[0], t(inp.colors_precomp)
    rendered, table = render(feat_mod, 32)
    rgb, _ = render(rgb_mod, 3)
    assert rendered.shape == (32, 64, 96) and rgb.shape == (3, 64, 96)
    proj, w = feature_pca_basis(table, 3, index=gui_pca_sample(table.shape[0], 1000))
    gates = torch.linspace(0.2, 1.0, 32, device=DEV)
    y0, x0 = divmod(int(rendered.norm(dim=0).argmax()), 96)              # two covered pixels, the second named past the edges
    y1, x1 = divmod(int(rendered[:16].norm(dim=0).argmax()), 96)
    queries = prompt_features(rendered, [(y0, x0), (64 + y1, 96 + x1)], gates)
    assert queries.shape == (2, 32) and (queries.norm(dim=-1) - 1).abs().max() <= 1e-5
    thr = 0.75
    got = viewer_frame(rendered, rgb, proj=proj, queries=queries, gates=gates, threshold=thr, modes=vr.MODES, preview=True)
    want = vr.frame64(rendered.cpu(), rgb.cpu(), proj.cpu(), queries.cpu(), gates.cpu(), thr, None, vr.MODES, True)
    worst, share = vr.frame_errors(got.frame.cpu(), want)
    print(f"rendered scene: worst error / bound = {worst:.3f}, excused {share:.5f}, selected {got.mask.float().mean().item():.3f}")
    assert worst <= 1.0 and share <= CAP
    assert got.mask[y0, x0].item() and got.mask[y1, x1].item()           # a clicked pixel selects itself: t = 1 > threshold
    mask, score = select_by_similarity(rendered, queries, thr, gates, pre="eps", half_shift=True)
    assert torch.equal(got.mask, mask) and torch.equal(bits(got.score), bits(score))
