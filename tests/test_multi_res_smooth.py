"""Multi-resolution KNN feature smoothing on the GPU (knn_smooth.py, include/mi_knn_smooth.h: mi_knn_smooth_multi_*): the HIP
kernels against the binary64 restatement tests/multi_res_smooth_ref.py (pinned to the reference's own method by the fixture,
tests/test_multi_res_smooth_host.py).  Every case prints the float32 reference expression's own error next to the kernels'."""
import os

import numpy as np
import pytest
import torch

import seganygaussians_amd
from seganygaussians_amd import knn_smooth as ks
from tests import edge_ref as er
from tests import multi_res_smooth_ref as mref

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multi_res_smooth", "multi_res_smooth.npz")

# out and dL/dF: the criterion of this kernel family (tests/test_knn_smooth.py): atol = TOL * max |want|, rtol = 0.  One tolerance
# for the whole tensor: it holds the LARGEST rows to 2e-5 and says nothing about a row far below max |want| (dL/dF_j scales with
# 1 / |F_j|; where zero feature rows put s * 1e12 into dL/dF it allows 3e8 next to ordinary rows of 5).  The rows are held one by
# one by edge_ref.multi_res_check, which _check applies as well (the rule and its cases: tests/test_multi_res_smooth_edges.py).
TOL = 2e-5
# dL/dw (a C-term dot product), same criterion.  The reference expression in float32 torch on the CPU, on the inputs of every case
# of this file, is within 1.19e-6 * max |want| of the restatement (largest: C=64 P=700 sum32 weights=row normalize_out=True; each
# case prints its own figure): inside 2e-5, so 2e-5 it is (the rule otherwise: 4 x the reference's own error).
# Measured apart, because max |want| says nothing there: under normalize_out with parallel level means (L = 1, or P = 1) dL/dw
# cancels to zero (mref.dw_term_scale), max |want| is below 1.6e-6 of the terms and the float32 reference is 0.02 ... 170 x
# max |want| off.  Those cases take the terms that cancel, max |dL/dret_i| * |mean_{l,i}|, as the scale instead; against it the
# float32 reference is within 1.6e-7, so 2e-5 again.
DW_TOL = 2e-5


def _gpu(F, levels, w, normalize_out, g, w_grad=True):
    dev = torch.device("cuda:0")
    f = torch.tensor(F, device=dev, requires_grad=True)
    mr = ks.MultiResNeighbourMap([(torch.as_tensor(pm), torch.as_tensor(idx).to(dev)) for pm, idx in levels])
    wt = None if w is None else torch.tensor(w, device=dev, requires_grad=w_grad)
    out = ks.multi_res_smooth_point_features(f, mr, wt, normalize_out)
    out.backward(torch.tensor(g, device=dev))
    torch.cuda.synchronize()
    return out.detach().cpu().numpy(), f.grad.cpu().numpy(), None if wt is None or wt.grad is None else wt.grad.cpu().numpy()


def _close(name, got, want, tol, rows=None, scale=None):
    if rows is not None:
        got, want = got[rows], want[rows]
    scale = np.abs(want).max() if scale is None else scale
    err = np.abs(got - want).max()
    print(f"    {name}: max |err| {err:.3e} = {err / scale if scale else 0.0:.2e} of scale {scale:.3e} (allowed {tol:.0e})")
    assert np.isfinite(got).all(), name
    np.testing.assert_allclose(got, want, rtol=0, atol=tol * scale, err_msg=name)


def _check(label, F, levels, w, normalize_out, g):
    want = mref.forward_backward(F, levels, w, normalize_out, g)
    noise = mref.fp32_reference_error(F, levels, w, normalize_out, g, want)
    print(f"  {label}: float32 reference expression vs binary64: out {noise[0]:.2e}, dF {noise[1]:.2e}, dw {noise[2] if noise[2] is None else format(noise[2], '.2e')}")
    got = _gpu(F, levels, w, normalize_out, g)
    _close("out", got[0], want[0], TOL)
    _close("dF", got[1], want[1], TOL)
    if w is None:
        assert got[2] is None
    else:
        assert got[2].shape == np.asarray(w).shape
        cancels = normalize_out and (len(levels) == 1 or len(F) == 1)
        _close("dw", got[2], want[2], DW_TOL, scale=mref.dw_term_scale(F, levels, w, normalize_out, g) if cancels else None)
    er.multi_res_check(f"  {label}", F, levels, w, g, normalize_out, *got)       # and every row on its own scale
    return got, want


LEVEL_SHAPES = {"default": ((0.1, 0.5, 1.5), (4, 4, 16)), "sum32": ((0.1, 0.5, 1.5), (8, 8, 16)), "L1": ((0.5,), (16,)),
                "L4": ((0.05, 0.1, 0.5, 1.5), (2, 4, 8, 16))}


@pytest.mark.parametrize("shape", sorted(LEVEL_SHAPES))
@pytest.mark.parametrize("P", [1, 33, 700])       # below, just above, and no multiple of the 32 / 16 rows of a workgroup
@pytest.mark.parametrize("C", [32, 64])
def test_hip_matches_restatement(C, P, shape):
    """Every width, row count and level layout; per case the three forms of the weights and normalize_out both ways.  Among
    them: a level of rate >= 1 (every point a member, every row its own nearest: the same Gaussian through two levels of one
    row), subsets smaller than k at P = 1 and 33 (hand-built maps may repeat a member), weights with zeros and negatives."""
    rates, Ks = LEVEL_SHAPES[shape]
    xyz, F, g, levels = mref.make_case(P, C, Ks, rates=rates, seed=C + P)
    if rates[-1] >= 1:
        assert levels[-1][0].all() and np.array_equal(levels[-1][1][:, 0], np.arange(P))
    for kind in (None, "full", "row"):
        w = mref.make_weights(kind, P, len(Ks), seed=P)
        if kind == "full" and len(Ks) > 1 and P > 1:
            assert (w == 0).any() and (w < 0).any()
        for normalize_out in (False, True):
            _check(f"C={C} P={P} {shape} weights={kind} normalize_out={normalize_out}", F, levels, w, normalize_out, g)


def test_subset_of_exactly_k_points_and_empty_lists():
    """Level 0's subset has exactly k_0 = 4 points: every row references the same 4 Gaussians, whose inverse lists hold all P
    rows; alone (L = 1) it leaves every other Gaussian with an empty list, i.e. a zero gradient.  Two feature rows are zero."""
    P, C = 700, 32
    xyz, F, g, levels = mref.make_case(P, C, (4, 4, 16), rates=(None, 0.5, 1.5), counts=(4, None, None), seed=5, zero_rows=(3, 411))
    members = np.flatnonzero(levels[0][0])
    F[members[0]] = 0.0                                          # a zero row among the four that every row reaches
    assert len(members) == 4 and (np.sort(levels[0][1], axis=1) == np.arange(4)).all()
    composed = ks.compose_levels([(torch.as_tensor(pm), torch.as_tensor(idx)) for pm, idx in levels])[0].numpy()
    lengths = np.bincount(composed.reshape(-1), minlength=P)     # of the inverse lists
    assert (lengths[members] >= P).all() and lengths.sum() == P * 24
    # the same Gaussian through two levels of one row: a member of level 0 is its own nearest there and in level 2
    assert composed[members[1], 0] == members[1] and composed[members[1], 8] == members[1]
    w = mref.make_weights("full", P, 3, seed=5)
    for normalize_out in (False, True):
        _check(f"exactly-k subset, normalize_out={normalize_out}", F, levels, w, normalize_out, g)
    single = levels[:1]
    (out, dF, dw), _ = _check("exactly-k subset alone (L = 1)", F, single, mref.make_weights("row", P, 1, seed=5), True, g)
    others = np.setdiff1d(np.arange(P), members)
    assert (dF[others] == 0).all() and np.abs(dF[members[1:]]).max() > 0
    assert np.isfinite(dF[members[0]]).all()                     # |F| < 1e-12: the s / eps branch


def test_row_with_all_weights_zero_stays_finite():
    """ret = 0 under normalize_out: out = 0, dL/dret = dL/dout / 1e-9 (the r > 0 guard), which reaches dL/dw of that row and, through
    zero weights, nothing else.  The row's dL/dw sets max |want|; the other rows are also compared on their own scale."""
    P, C = 97, 32
    xyz, F, g, levels = mref.make_case(P, C, (4, 4, 16), rates=(0.1, 0.5, 1.5), seed=9)
    w = mref.make_weights("full", P, 3, seed=9)
    w[40] = 0.0
    (out, dF, dw), want = _check("all weights of row 40 zero", F, levels, w, True, g)
    assert (out[40] == 0).all() and np.abs(dw[40]).max() > 1e6
    rest = np.arange(P) != 40
    _close("dw, other rows", dw, want[2], DW_TOL, rows=rest)


def test_feature_gradient_only():
    """Weights that do not require a gradient: dL/dF alone (no dL/dw buffer; without normalize_out no pass A either)."""
    P, C = 333, 64
    xyz, F, g, levels = mref.make_case(P, C, (4, 4, 16), rates=(0.1, 0.5, 1.5), seed=21)
    w = mref.make_weights("full", P, 3, seed=21)
    for normalize_out in (False, True):
        want = mref.forward_backward(F, levels, w, normalize_out, g)
        out, dF, dw = _gpu(F, levels, w, normalize_out, g, w_grad=False)
        assert dw is None
        _close("out", out, want[0], TOL)
        _close("dF", dF, want[1], TOL)
    dev = torch.device("cuda:0")
    mr = ks.MultiResNeighbourMap([(torch.as_tensor(pm), torch.as_tensor(idx).to(dev)) for pm, idx in levels])
    with torch.no_grad():
        out = ks.multi_res_smooth_point_features(torch.tensor(F, device=dev), mr, torch.tensor(w, device=dev), True)
    _close("out, no_grad", out.cpu().numpy(), want[0], TOL)
    # weights only
    f, wt = torch.tensor(F, device=dev), torch.tensor(w, device=dev, requires_grad=True)
    ks.multi_res_smooth_point_features(f, mr, wt, True).backward(torch.tensor(g, device=dev))
    _close("dw alone", wt.grad.cpu().numpy(), want[2], DW_TOL)
    # refusals of the host layer
    with pytest.raises(ValueError):
        ks.multi_res_smooth_point_features(f[:-1], mr)
    with pytest.raises(ValueError):
        ks.multi_res_smooth_point_features(f, mr, wt[:, :2])
    with pytest.raises(RuntimeError, match="GPU"):
        ks.multi_res_smooth_point_features(f, mr, wt.detach().cpu())
    with pytest.raises(ValueError):
        ks.multi_res_smooth_point_features(torch.zeros(P, 48, device=dev), mr)
    ks.multi_res_smooth_point_features(f, mr)                    # and a refusal leaves nothing behind


def test_two_runs_are_bitwise_equal():
    P, C = 700, 32
    xyz, F, g, levels = mref.make_case(P, C, (4, 4, 16), rates=(None, 0.5, 1.5), counts=(4, None, None), seed=31)
    for kind in ("full", "row"):
        w = mref.make_weights(kind, P, 3, seed=31)
        a, b = _gpu(F, levels, w, True, g), _gpu(F, levels, w, True, g)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def _fixture():
    z = np.load(FIXTURE)
    return z, [(z[f"level{l}.point_mask"], z[f"level{l}.m"].astype(np.int64)) for l in range(3)]


def test_fixture_through_the_function():
    """The results recorded from the reference's own method (binary64): P = 300, C = 32, default rates and Ks."""
    z, levels = _fixture()
    for tag, w in (("none", None), ("weighted", z["weights"])):
        out, dF, dw = _gpu(z["features"], levels, w, False, z["grad_out"])
        _close(f"{tag}.out", out, z[f"{tag}.out"], TOL)
        _close(f"{tag}.dF", dF, z[f"{tag}.dF"], TOL)
        if w is not None:
            _close(f"{tag}.dw", dw, z[f"{tag}.dw"], DW_TOL)


def test_fixture_through_the_patched_method():
    """The method that install_dropin(fuse_smoothing=True) binds, on a stub class: from the reference's generator state it draws
    the fixture's subsets, the HIP search finds the fixture's maps, and values and gradients are the recorded ones; state it
    finds (the fixture's maps) is used as it is."""
    z, levels = _fixture()
    dev = torch.device("cuda:0")

    class FeatureGaussianModel:
        def __init__(self):
            self.get_xyz = torch.tensor(z["xyz"], device=dev)
            self._point_features = torch.tensor(z["features"], device=dev, requires_grad=True)
            self.multi_res_feature_smooth_map = []

        def get_smoothed_point_features(self, K=16, dropout=0.5):
            raise AssertionError("not under test")

        def get_multi_resolution_smoothed_point_features(self, sample_rates=(0.1, 0.5, 1.5), Ks=(4, 4, 16), smooth_weights=None):
            raise AssertionError("the reference's method must not run inside the fused limits")

    seganygaussians_amd.install_dropin()
    seganygaussians_amd.patch_feature_model(FeatureGaussianModel)
    g = torch.tensor(z["grad_out"], device=dev)

    def run(pc, tag):
        w = None if tag == "none" else torch.tensor(z["weights"], device=dev, requires_grad=True)
        pc._point_features.grad = None
        out = pc.get_multi_resolution_smoothed_point_features(smooth_weights=w)
        out.backward(g)
        _close(f"{tag}.out", out.detach().cpu().numpy(), z[f"{tag}.out"], TOL)
        _close(f"{tag}.dF", pc._point_features.grad.cpu().numpy(), z[f"{tag}.dF"], TOL)
        if w is not None:
            _close(f"{tag}.dw", w.grad.cpu().numpy(), z[f"{tag}.dw"], DW_TOL)

    built = FeatureGaussianModel()
    torch.manual_seed(int(z["seed"]))
    run(built, "weighted")
    for l, mrf in enumerate(built.multi_res_feature_smooth_map):
        assert (mrf["rate"], mrf["K"]) == ((0.1, 0.5, 1.5)[l], (4, 4, 16)[l])
        assert np.array_equal(mrf["point_mask"].numpy(), levels[l][0])
        assert np.array_equal(mrf["m"].cpu().numpy(), levels[l][1])
    cached = built._mi_multi_res_map[1]
    run(built, "none")
    assert built._mi_multi_res_map[1] is cached                   # the composed map: once per set of maps

    given = FeatureGaussianModel()
    given.multi_res_feature_smooth_map = [
        {"rate": r, "K": k, "point_mask": torch.as_tensor(pm), "m": torch.as_tensor(m).to(dev)}
        for (pm, m), r, k in zip(levels, (0.1, 0.5, 1.5), (4, 4, 16))]
    state = torch.get_rng_state()
    run(given, "weighted")
    assert torch.equal(torch.get_rng_state(), state)              # nothing drawn
    # MultiResNeighbourMap.from_points: the same draws from a generator of its own, the same maps
    mr = ks.MultiResNeighbourMap.from_points(given.get_xyz, generator=torch.Generator().manual_seed(int(z["seed"])))
    assert torch.equal(mr.nmap.idx, cached.nmap.idx) and mr.level_k == [4, 4, 16]
