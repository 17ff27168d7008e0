"""CPU checks of the viewer frame: the float64 restatement (tests/viewer_ref.py) against the reference's own float32 lines, the share
of pixels the band excuses and the eigen-gaps for exactly the seeds and shapes the GPU test uses, the argument checks of
seganygaussians_amd/viewer.py before any launch, and the exports.  No GPU."""
import ctypes
import os

import pytest
import torch

import seganygaussians_amd
from seganygaussians_amd import _lib, build
from seganygaussians_amd import viewer as vw
from tests import viewer_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 0.01


def _literal(c, thr, cluster, modes, preview):
    return vr.literal32_fetch_data(c.features, c.rgb, c.proj, c.gates, None if c.queries is None else c.queries.t().contiguous(), thr,
                                   None if cluster is None else cluster.permute(1, 2, 0).contiguous(), modes, preview)


@pytest.mark.parametrize("case", [vr.MODE_CASE, ((6, 65), 33, 5, 8, 0.55), ((3, 5), 3, 0, 2, 0.5)], ids=lambda c: f"{c[0]}-C{c[1]}-Q{c[2]}")
def test_fetch_data_lines_match_restatement(case):
    """Every mode subset, preview on and off, with and without a cluster render: the reference's float32 frame (np.interp Jet, numpy
    averaging) lies within the yardstick's bound of the float64 frame at every pixel the band does not excuse."""
    shape, C, Q, seed, thr = case
    c = vr.make_view_case(shape, C, Q, seed)
    c.features[:, 0, 0] = 0.0                                # a background pixel of a zero-background render
    for modes in vr.ALL_MODE_SUBSETS:
        for preview in (False, True):
            for cluster in (None, c.cluster_rgb):
                want = vr.frame64(c.features, c.rgb, c.proj, c.queries, c.gates, thr, cluster, modes, preview)
                lit = _literal(c, thr, cluster, modes, preview)
                worst, share = vr.frame_errors(lit, want)
                assert worst <= 1.0, (modes, preview, cluster is not None, worst)
                assert want.frame.shape == lit.shape == shape + (3,)
    # no mode behaves as "rgb" (:703); without a click "similarity" and "cluster" show the scene
    want = vr.frame64(c.features, c.rgb, c.proj, None, None, thr, None, (), False)
    assert torch.equal(want.frame, c.rgb.double().permute(1, 2, 0)) and want.mask is None
    want = vr.frame64(c.features, c.rgb, c.proj, None, None, thr, None, ("cluster", "similarity"), True)
    assert torch.equal(want.frame, c.rgb.double().permute(1, 2, 0))


def test_jet_restatement_is_np_interp():
    s = torch.cat([torch.linspace(-0.25, 1.25, 1201, dtype=torch.float64), torch.arange(9, dtype=torch.float64) / 8])
    want = torch.from_numpy(vr.literal32_grayscale_to_colormap(s.numpy()))
    assert (vr.jet64(s) - want).abs().max() <= 1e-15
    assert vr.jet64(torch.tensor([0.0, 0.5, 1.0, -3.0, 7.0])).tolist() == [[0, 0, 0.5], [0.5, 1, 0.5], [0.5, 0, 0], [0, 0, 0.5], [0.5, 0, 0]]


@pytest.mark.parametrize("case", vr.FRAME_CASES + [vr.MODE_CASE], ids=lambda c: f"{c[0]}-C{c[1]}-Q{c[2]}")
def test_excused_share_of_the_gpu_cases(case):
    """For the seeds and shapes of the GPU test the float64 reference alone keeps the excused pixels under the cap."""
    shape, C, Q, seed, thr = case
    c = vr.make_view_case(shape, C, Q, seed)
    want = vr.frame64(c.features, c.rgb, c.proj, c.queries, c.gates, thr, c.cluster_rgb, vr.MODES, True)
    assert want.band.double().mean().item() <= CAP
    if Q:
        assert abs(float(c.queries.norm(dim=-1).max()) - 1.0) < 1e-6
    else:
        assert want.mask is None and not want.excused.any()


def test_pca_lines_match_restatement():
    feats = vr.planted_features(**vr.PLANTED)
    lit, randint = vr.literal32_do_pca(feats, 5000)
    assert torch.equal(randint, vw.gui_pca_sample(feats.shape[0], 5000))
    mean, cov, n = vr.moments64(feats, randint, pre="eps")
    proj, w, w_all = vr.basis64(cov)
    assert n == 5000
    # up to sign: the reference's sign is LAPACK's
    cos = (lit.double() * proj).sum(0).abs()
    assert (cos >= 1 - 1e-6).all(), cos
    assert (proj.t() @ proj - torch.eye(3, dtype=torch.float64)).abs().max() <= 1e-12
    k = proj.abs().argmax(dim=0)
    assert (proj.gather(0, k[None]) > 0).all()
    prod, pw = vw.basis_from_covariance(cov, 3)
    assert torch.equal(prod, proj) and torch.equal(pw, w)


def test_planted_eigen_gaps_of_the_gpu_case():
    """The planted case of the GPU test: the gap of each of the first three eigenvalues is at least 20 % of the eigenvalue."""
    feats = vr.planted_features(**vr.PLANTED)
    for index in (None, vw.gui_pca_sample(feats.shape[0], 4000)):
        _, cov, _ = vr.moments64(feats, index, pre="eps")
        _, w, w_all = vr.basis64(cov)
        gaps = vr.eigen_gaps(w_all, 3)
        assert (gaps >= 0.2 * w).all(), (gaps, w)


def test_gui_pca_sample_is_the_seeded_draw():
    torch.manual_seed(1234)
    before = torch.random.get_rng_state()
    got = vw.gui_pca_sample(1_000_003)
    assert torch.equal(torch.random.get_rng_state(), before)          # the global generator has not moved
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        want = torch.randint(0, 1_000_003, [200_000])
    assert got.dtype == torch.int64 and torch.equal(got, want)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(7)
        want = torch.randint(0, 10, [33])
    assert torch.equal(vw.gui_pca_sample(10, 33, seed=7), want)
    with pytest.raises(ValueError, match="P >= 1"):
        vw.gui_pca_sample(0)


def test_prompt_features_are_the_reference_rows():
    c = vr.make_view_case((7, 9), 32, 1, 31)
    sems = c.features.clone().permute(1, 2, 0)
    sems /= (torch.norm(sems, dim=-1, keepdim=True) + 1e-6)
    featmap = torch.nn.functional.normalize(sems * c.gates.unsqueeze(0).unsqueeze(0), dim=-1, p=2)
    clicks = [(2, 3), (7 + 1, 9 + 4), (-1, -2)]                          # (y, x); the last two wrap
    got = vw.prompt_features(c.features, clicks, c.gates)
    want = torch.stack([featmap[y % 7, x % 9, :] for y, x in clicks])
    assert got.shape == (3, 32) and (got - want).abs().max() <= 1e-6
    with pytest.raises(ValueError, match=r"\(C, H, W\)"):
        vw.prompt_features(torch.zeros(4, 8), [(0, 0)])


def test_bad_inputs_refused_before_any_launch():
    f, rgb = torch.zeros(8, 4, 5), torch.zeros(3, 4, 5)
    q, proj = torch.zeros(2, 8), torch.zeros(8, 3)
    frame = lambda f_=f, rgb_=rgb, **k: vw.viewer_frame(f_, rgb_, **k)
    cov = lambda f_, **k: vw.feature_covariance(f_, **k)
    basis = lambda f_, **k: vw.feature_pca_basis(f_, **k)
    # the list of the segmentation queries, for all three calls
    for fn in (frame, cov, basis):
        with pytest.raises(ValueError, match="GPU"):
            fn(f)
        with pytest.raises(ValueError, match="float32"):
            fn(f.double())
        with pytest.raises(ValueError, match="float32"):
            fn(f.numpy())
        with pytest.raises(ValueError, match="256"):
            fn(torch.zeros(257, 2, 2))
        with pytest.raises(ValueError, match="rows"):
            fn(torch.zeros(8, 0, 5))
        with pytest.raises(ValueError, match="requires grad"):
            fn(f.clone().requires_grad_())
        with torch.no_grad(), pytest.raises(ValueError, match="GPU"):   # allowed with grad mode off; then the device check
            fn(f.clone().requires_grad_())
    for fn in (cov, basis):
        with pytest.raises(ValueError, match=r"\(C, H, W\) or \(P, C\)"):
            fn(torch.zeros(8))
        with pytest.raises(ValueError, match=r"\(C, H, W\) or \(P, C\)"):
            fn(torch.zeros(1, 2, 3, 8))
        with pytest.raises(ValueError, match="pre"):
            fn(f, pre="L2")
        with pytest.raises(ValueError, match="out of range"):
            fn(torch.zeros(10, 8), index=torch.tensor([0, 10]))
        with pytest.raises(ValueError, match="out of range"):
            fn(f, index=torch.tensor([-1]))
        with pytest.raises(ValueError, match="out of range"):
            fn(f, index=torch.tensor([3, 20, 3]))                        # an image has H W = 20 rows
        with pytest.raises(ValueError, match="int64"):
            fn(f, index=torch.tensor([1], dtype=torch.int32))
        with pytest.raises(ValueError, match="index"):
            fn(f, index=torch.zeros(0, dtype=torch.int64))
        with pytest.raises(ValueError, match="GPU"):
            fn(torch.zeros(10, 8), index=torch.tensor([0, 9, 9]))        # a valid index: on to the device check
    with pytest.raises(ValueError, match="n_components"):
        basis(f, n_components=9)
    with pytest.raises(ValueError, match="n_components"):
        basis(torch.zeros(10, 2), n_components=3)
    with pytest.raises(ValueError, match="n_components"):
        basis(f, n_components=0)
    with pytest.raises(ValueError, match=r"\(C, H, W\)"):
        frame(torch.zeros(10, 8))
    with pytest.raises(ValueError, match="rgb"):
        frame(rgb_=torch.zeros(3, 4, 6))
    with pytest.raises(ValueError, match="rgb"):
        frame(rgb_=torch.zeros(4, 5, 3))
    with pytest.raises(ValueError, match="float32"):
        frame(rgb_=rgb.half())
    with pytest.raises(ValueError, match="cluster_rgb"):
        frame(cluster_rgb=torch.zeros(3, 5, 4))
    with pytest.raises(ValueError, match="cluster_rgb"):
        frame(cluster_rgb=torch.zeros(3, 4, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="proj"):
        frame(proj=torch.zeros(3, 8), modes=("pca",))
    with pytest.raises(ValueError, match="proj"):
        frame(proj=torch.zeros(8, 2))
    with pytest.raises(ValueError, match="proj"):
        frame(modes=("pca",))                                            # the mode needs the basis
    with pytest.raises(ValueError, match="unknown mode"):
        frame(modes=("rgb", "depth"))
    with pytest.raises(ValueError, match="unknown mode"):
        frame(modes="RGB")
    with pytest.raises(ValueError, match="must be"):
        frame(queries=torch.zeros(2, 7))
    with pytest.raises(ValueError, match="float32"):
        frame(queries=q.half())
    with pytest.raises(ValueError, match="16"):
        frame(queries=torch.zeros(17, 8))
    with pytest.raises(ValueError, match="queries"):
        frame(queries=torch.zeros(0, 8))
    with pytest.raises(ValueError, match="gates"):
        frame(queries=q, gates=torch.zeros(7))
    with pytest.raises(ValueError, match="gates"):
        frame(queries=q, gates=torch.zeros(8, dtype=torch.float64))
    with pytest.raises(ValueError, match="threshold"):
        frame(queries=q, threshold=float("nan"))
    with pytest.raises(ValueError, match="threshold"):
        frame(queries=q, threshold="high")
    with pytest.raises(ValueError, match="out must be"):
        frame(out=torch.zeros(4, 5, 4))
    with pytest.raises(ValueError, match="out must be"):
        frame(out=torch.zeros(3, 4, 5).permute(1, 2, 0))
    with pytest.raises(ValueError, match="requires grad"):
        frame(queries=q.clone().requires_grad_())
    with pytest.raises(ValueError, match="GPU"):                         # everything valid: on to the device check
        frame(proj=proj, queries=q, gates=torch.ones(8), cluster_rgb=rgb, modes=vr.MODES, preview=True, out=torch.zeros(4, 5, 3))


def test_abi_exported_and_checks_arguments():
    build.build_library()
    L = _lib.load()
    names = ["mi_view_moments_workspace_bytes", "mi_view_moments_block", "mi_view_moments", "mi_view_frame"]
    assert _lib.DECLARED["mi_viewer.h"] == names and set(names) <= set(_lib.ALL_EXPORTS)
    for name in names:
        assert ctypes.cast(getattr(L, name), ctypes.c_void_p).value
    assert {"viewer.h", "seg_row.h", "mi_viewer.hip"} <= set(build.SOURCES)
    includers = [f for f in build.SOURCES if '"viewer.h"' in open(os.path.join(build.SRC_DIR, f)).read()]
    assert includers == ["mi_viewer.hip"]
    includers = [f for f in build.SOURCES if '"seg_row.h"' in open(os.path.join(build.SRC_DIR, f)).read()]
    assert includers == ["segment.h", "viewer.h"]
    B = L.mi_view_moments_block()
    assert B > 0 and B % 2 == 0                                          # whole k-steps of the 32x32x2 instruction
    # the workspace: zero out of range, growing with the rows up to the cap of workgroups, 8-byte granular
    assert L.mi_view_moments_workspace_bytes(0, 32) == 0 and L.mi_view_moments_workspace_bytes(10, 0) == 0
    assert L.mi_view_moments_workspace_bytes(10, 257) == 0
    assert 0 < L.mi_view_moments_workspace_bytes(1, 1) <= L.mi_view_moments_workspace_bytes(5 * B, 1)
    assert L.mi_view_moments_workspace_bytes(1 << 30, 64) == L.mi_view_moments_workspace_bytes(1 << 29, 64) <= 64 << 20
    assert L.mi_view_moments_workspace_bytes(1 << 30, 256) <= 64 << 20 and L.mi_view_moments_workspace_bytes(77, 33) % 8 == 0
    # argument checks run before any launch: no device needed
    m = lambda *a: L.mi_view_moments(*a)
    assert m(2, 4, 4, 8, None, 4, 2, 8, 1 << 20, 8, 8, None) != 0 and "layout" in _lib.last_error()
    assert m(1, 0, 4, 8, None, 4, 2, 8, 1 << 20, 8, 8, None) != 0 and "N >= 1" in _lib.last_error()
    assert m(1, 4, 257, 8, None, 4, 2, 8, 1 << 20, 8, 8, None) != 0 and "256" in _lib.last_error()
    assert m(1, 4, 4, 8, None, 0, 2, 8, 1 << 20, 8, 8, None) != 0 and "n >= 1" in _lib.last_error()
    assert m(1, 4, 4, 8, None, 5, 2, 8, 1 << 20, 8, 8, None) != 0 and "n <= N" in _lib.last_error()
    assert m(1, 4, 4, 8, None, 4, 3, 8, 1 << 20, 8, 8, None) != 0 and "pre" in _lib.last_error()
    assert m(1, 4, 4, None, None, 4, 2, 8, 1 << 20, 8, 8, None) != 0 and "null" in _lib.last_error()
    assert m(1, 4, 4, 8, None, 4, 2, 8, 1 << 20, None, 8, None) != 0 and "null" in _lib.last_error()
    assert m(1, 4, 4, 8, None, 4, 2, None, 1 << 20, 8, 8, None) != 0 and "workspace" in _lib.last_error()
    assert m(1, 4, 4, 8, None, 4, 2, 8, 16, 8, 8, None) != 0 and "workspace" in _lib.last_error()
    assert m(1, 4, 4, 8, None, 4, 2, 12, 1 << 20, 8, 8, None) != 0 and "workspace" in _lib.last_error()
    fr = lambda *a: L.mi_view_frame(*a)
    assert fr(0, 4, 8, 8, None, None, 0, None, None, 0.5, 1, 0, 8, None, None, None) != 0 and "N >= 1" in _lib.last_error()
    assert fr(4, 257, 8, 8, None, None, 0, None, None, 0.5, 1, 0, 8, None, None, None) != 0 and "256" in _lib.last_error()
    assert fr(4, 4, 8, 8, None, None, 17, 8, None, 0.5, 1, 0, 8, 8, 8, None) != 0 and "16" in _lib.last_error()
    assert fr(4, 4, 8, 8, None, None, 0, None, None, 0.5, 0, 0, 8, None, None, None) != 0 and "modes" in _lib.last_error()
    assert fr(4, 4, 8, 8, None, None, 0, None, None, 0.5, 16, 0, 8, None, None, None) != 0 and "modes" in _lib.last_error()
    assert fr(4, 4, None, 8, None, None, 0, None, None, 0.5, 1, 0, 8, None, None, None) != 0 and "null" in _lib.last_error()
    assert fr(4, 4, 8, 8, None, None, 0, None, None, 0.5, 1, 0, None, None, None, None) != 0 and "null" in _lib.last_error()
    assert fr(4, 4, 8, 8, None, None, 0, None, None, 0.5, 2, 0, 8, None, None, None) != 0 and "basis" in _lib.last_error()
    assert fr(4, 4, 8, 8, None, None, 1, 8, None, 0.5, 1, 0, 8, None, 8, None) != 0 and "mask and score" in _lib.last_error()
    assert fr(4, 4, 8, 8, None, None, 1, None, None, 0.5, 1, 0, 8, 8, 8, None) != 0 and "mask and score" in _lib.last_error()
    assert fr(4, 4, 8, 8, None, None, 1, 8, None, float("nan"), 1, 0, 8, 8, 8, None) != 0 and "NaN" in _lib.last_error()


def test_module_exports():
    for name in ("ViewerFrame", "feature_covariance", "feature_pca_basis", "gui_pca_sample", "prompt_features", "viewer_frame"):
        assert getattr(seganygaussians_amd, name) is getattr(vw, name)
    with pytest.raises(AttributeError):
        seganygaussians_amd.no_such_name
    assert vw.VIEW_MODES == _lib.MI_VIEW_MODES and tuple(vw.VIEW_MODES) == vr.MODES
    assert vw.ViewerFrame._fields == ("frame", "mask", "score")
    hdr = open(os.path.join(ROOT, "include", "mi_viewer.h")).read()
    for name, bit in _lib.MI_VIEW_MODES.items():
        assert f"#define MI_VIEW_{name.upper()} {bit}\n" in hdr
