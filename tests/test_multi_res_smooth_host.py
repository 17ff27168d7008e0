"""Multi-resolution feature smoothing, host side (no GPU): the binary64 restatement (tests/multi_res_smooth_ref.py) against the
fixture recorded from the reference's own method (tests/golden/make_multi_res_smooth_golden.py), the subset draws, the
composition of the levels' maps, the limits, and the drop-in binding."""
import os
import types

import numpy as np
import pytest
import torch

import seganygaussians_amd
from seganygaussians_amd import knn_smooth as ks
from tests import multi_res_smooth_ref as mref

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multi_res_smooth", "multi_res_smooth.npz")


def fixture_levels(z):
    return [(z[f"level{l}.point_mask"], z[f"level{l}.m"]) for l in range(len(z["Ks"]))]


@pytest.mark.parametrize("tag", ["none", "weighted"])
def test_restatement_equals_the_reference_fixture(tag):
    z = np.load(FIXTURE)
    assert z["features"].shape == (300, 32) and tuple(z["Ks"]) == (4, 4, 16) and tuple(z["rates"]) == (0.1, 0.5, 1.5)
    w = z["weights"] if tag == "weighted" else None
    out, dF, dw = mref.forward_backward(z["features"], fixture_levels(z), w, False, z["grad_out"])
    np.testing.assert_allclose(out, z[f"{tag}.out"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(dF, z[f"{tag}.dF"], rtol=1e-9, atol=1e-12)
    if w is not None:
        assert z["weights"].shape == (300, 3)
        np.testing.assert_allclose(dw, z[f"{tag}.dw"], rtol=1e-9, atol=1e-12)


def test_fixture_masks_are_the_reference_draws():
    """The fixture's subsets are the method's own `torch.rand(P) < r` draws after torch.manual_seed(seed), level after level;
    draw_point_masks (what MultiResNeighbourMap.from_points uses) repeats them from the same generator state."""
    z = np.load(FIXTURE)
    torch.manual_seed(int(z["seed"]))
    got = ks.draw_point_masks(300, tuple(z["rates"]))
    gen = torch.Generator().manual_seed(5)
    want = [torch.rand(300, generator=gen) < r for r in (0.1, 0.5, 1.5)]
    own = ks.draw_point_masks(300, (0.1, 0.5, 1.5), generator=torch.Generator().manual_seed(5))
    for l in range(3):
        assert np.array_equal(got[l].numpy(), z[f"level{l}.point_mask"])
        assert torch.equal(own[l], want[l])
    assert bool(got[2].all())                    # a rate >= 1: every point is a member


class _Stub:
    """What the method reads of a FeatureGaussianModel."""

    def __init__(self, xyz, feats):
        self.get_xyz, self._point_features, self.multi_res_feature_smooth_map = xyz, feats, []

    def get_multi_resolution_smoothed_point_features(self, sample_rates=(0.1, 0.5, 1.5), Ks=(4, 4, 16), smooth_weights=None):
        return "reference", tuple(sample_rates), tuple(Ks), smooth_weights


def _bruteforce_knn_points(p1, p2, K=1, **_):
    d = torch.cdist(p1[0].double(), p2[0].double())
    return types.SimpleNamespace(idx=d.topk(K, dim=1, largest=False).indices[None])


@pytest.fixture
def patched_stub(monkeypatch):
    seganygaussians_amd.install_dropin()
    import pytorch3d.ops
    monkeypatch.setattr(pytorch3d.ops, "knn_points", _bruteforce_knn_points)
    cls = type("FeatureGaussianModel", (_Stub,), {"get_smoothed_point_features": lambda self, K=16, dropout=0.5: "reference"})
    seganygaussians_amd.patch_feature_model(cls)
    return cls


def test_fused_method_draws_in_the_reference_order_and_keeps_its_state(patched_stub):
    """Same generator state -> the same `torch.rand(P) < r` per level, in level order, stored in the reference's state layout; the
    same rebuild condition (only a level whose rate or K changed draws again).  On CPU tensors the kernels are refused."""
    cls = patched_stub
    g = torch.Generator().manual_seed(0)
    pc = cls(torch.randn(200, 3, generator=g), torch.randn(200, 32, generator=g))
    torch.manual_seed(77)
    want = [torch.rand(200) < r for r in (0.1, 0.5, 1.5)]
    after = torch.get_rng_state()
    torch.manual_seed(77)
    with pytest.raises(RuntimeError, match="GPU"):            # the maps are built, then the kernels refuse CPU tensors
        pc.get_multi_resolution_smoothed_point_features()
    assert torch.equal(torch.get_rng_state(), after)
    state = pc.multi_res_feature_smooth_map
    assert [sorted(m) for m in state] == [["K", "m", "point_mask", "rate"]] * 3
    assert [(m["rate"], m["K"]) for m in state] == [(0.1, 4), (0.5, 4), (1.5, 16)]
    for l in range(3):
        assert torch.equal(state[l]["point_mask"], want[l]) and tuple(state[l]["m"].shape) == (200, (4, 4, 16)[l])
        assert int(state[l]["m"].max()) < int(want[l].sum())
    # same arguments: nothing is drawn; level 1 changed: one draw, the other levels' entries stay the same objects
    kept = [m["m"] for m in state]
    with pytest.raises(RuntimeError, match="GPU"):
        pc.get_multi_resolution_smoothed_point_features()
    assert torch.equal(torch.get_rng_state(), after) and all(a["m"] is b for a, b in zip(pc.multi_res_feature_smooth_map, kept))
    want1 = torch.rand(200) < 0.6
    torch.set_rng_state(after)
    with pytest.raises(RuntimeError, match="GPU"):
        pc.get_multi_resolution_smoothed_point_features(sample_rates=(0.1, 0.6, 1.5))
    state = pc.multi_res_feature_smooth_map
    assert state[0]["m"] is kept[0] and state[2]["m"] is kept[2] and state[1]["rate"] == 0.6
    assert torch.equal(state[1]["point_mask"], want1)


def test_outside_the_fused_limits_the_reference_method_runs(patched_stub):
    cls = patched_stub
    g = torch.Generator().manual_seed(1)
    pc = cls(torch.randn(50, 3, generator=g), torch.randn(50, 32, generator=g))
    before = torch.get_rng_state()
    assert pc.get_multi_resolution_smoothed_point_features((0.5,) * 5, (2,) * 5)[0] == "reference"                 # L > 4
    assert pc.get_multi_resolution_smoothed_point_features((0.5, 0.5, 1.5), (16, 16, 4))[0] == "reference"       # sum k > 32
    # a subset smaller than its K: the reference's method finds the generator and the state as they were before the call
    assert pc.get_multi_resolution_smoothed_point_features((1.5, 0.0), (4, 4)) == ("reference", (1.5, 0.0), (4, 4), None)
    assert torch.equal(torch.get_rng_state(), before) and pc.multi_res_feature_smooth_map == []
    pc48 = cls(pc.get_xyz, torch.randn(50, 48, generator=g))
    assert pc48.get_multi_resolution_smoothed_point_features()[0] == "reference"                                   # C not in {32, 64}
    with pytest.raises(AssertionError):                                                                               # the reference's own assertion
        pc.get_multi_resolution_smoothed_point_features((0.5, 0.5), (4, 4, 4))
    with pytest.raises(AssertionError):
        pc.get_multi_resolution_smoothed_point_features((0.5, 0.5), (4, 4), smooth_weights=torch.ones(50, 3))
    # without a reference method to hand over to, the limits raise
    with pytest.raises(ValueError, match="sum"):
        ks.fused_get_multi_resolution_smoothed_point_features(_Stub(pc.get_xyz, pc._point_features), (0.5, 0.5, 1.5), (16, 16, 4))


def test_patch_binds_when_the_method_exists_and_tolerates_its_absence(patched_stub):
    cls = patched_stub
    assert cls.get_multi_resolution_smoothed_point_features is ks.fused_get_multi_resolution_smoothed_point_features
    assert cls._reference_get_multi_resolution_smoothed_point_features(cls(None, None))[0] == "reference"
    assert cls.get_smoothed_point_features is ks.fused_get_smoothed_point_features
    seganygaussians_amd.patch_feature_model(cls)                      # idempotent
    cls._mi_fused_smoothing = False
    seganygaussians_amd.patch_feature_model(cls)                      # and never takes the fused method for the reference's
    assert cls._reference_get_multi_resolution_smoothed_point_features(cls(None, None))[0] == "reference"

    class Bare:
        def get_smoothed_point_features(self, K=16, dropout=0.5):
            return "reference"

    seganygaussians_amd.patch_feature_model(Bare)
    assert Bare.get_smoothed_point_features is ks.fused_get_smoothed_point_features
    assert not hasattr(Bare, "get_multi_resolution_smoothed_point_features")
    assert not hasattr(Bare, "_reference_get_multi_resolution_smoothed_point_features")


def test_composition_gives_global_indices():
    """compose_levels: column block l of the composed map is sub_l[idx_l], sub_l = nonzero(point_mask_l)."""
    z = np.load(FIXTURE)
    levels = [(torch.as_tensor(pm), torch.as_tensor(m)) for pm, m in fixture_levels(z)]
    composed, level_k = ks.compose_levels(levels)
    assert level_k == [4, 4, 16] and tuple(composed.shape) == (300, 24)
    c0 = 0
    for pm, idx in levels:
        sub = np.flatnonzero(pm.numpy())
        assert np.array_equal(composed[:, c0:c0 + idx.size(1)].numpy(), sub[idx.numpy()])
        c0 += idx.size(1)
    assert np.array_equal(composed[:, 8].numpy(), np.arange(300))       # rate 1.5: the subset is the cloud, nearest = itself
    # the map the kernels see gives the restatement's result when read as ONE level over the whole cloud per column block
    F = torch.as_tensor(z["features"], dtype=torch.float64)
    n = torch.nn.functional.normalize(F, dim=-1, p=2)
    want = sum(n[composed[:, a:b]].mean(dim=1) for a, b in ((0, 4), (4, 8), (8, 24)))
    np.testing.assert_allclose(want.numpy(), z["none.out"], rtol=1e-9, atol=1e-12)


def test_limits_and_bad_shapes_raise():
    pm = torch.tensor([True, False, True, True])
    idx = torch.tensor([[0, 1], [1, 2], [2, 0], [0, 0]])
    composed, level_k = ks.compose_levels([(pm, idx)])
    assert level_k == [2] and composed.tolist() == [[0, 2], [2, 3], [3, 0], [0, 0]]
    bad = [
        [],                                                         # no level
        [(pm, idx)] * 5,                                            # L > 4
        [(pm, idx.repeat(1, 9))] * 2,                               # sum k = 36 > 32
        [(pm, torch.tensor([[0, 3]] * 4))],                         # index outside the subset of 3
        [(pm, torch.tensor([[0, -1]] * 4))],                        # the search's padding value
        [(pm, idx[:3])],                                            # rows != P
        [(pm, idx[:, 0])],                                          # not (P, k)
        [(pm, idx[:, :0])],                                         # k = 0
        [(pm.float(), idx)],                                        # mask not bool
        [(pm, idx.float())],                                        # float indices
        [(torch.zeros(4, dtype=torch.bool), idx)],                  # empty subset
        [(pm, idx), (pm[:3], idx[:3])],                             # levels of different P
    ]
    for levels in bad:
        with pytest.raises(ValueError):
            ks.compose_levels(levels)
    with pytest.raises(RuntimeError, match="GPU"):                  # no CPU path
        ks.MultiResNeighbourMap([(pm, idx)])
    with pytest.raises(RuntimeError, match="GPU"):
        ks.multi_res_smooth_point_features(torch.zeros(4, 32), object())


def test_c_abi_refuses_bad_arguments_before_any_hip_call():
    """In the style of tests/test_abi.py's REFUSED: the pointers are never read."""
    import ctypes
    from seganygaussians_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    k = lambda *v: (ctypes.c_int * len(v))(*v)
    fwd = lambda P, C, L, lk: lib.mi_knn_smooth_multi_forward(P, C, L, lk, 8, 8, 0, 8, 8, 0, None)
    bwd = lambda P, C, L, lk: lib.mi_knn_smooth_multi_backward(P, C, L, lk, 8, 8, 8, 8, 0, 8, 8, 8, 8, None, 0, None)
    for call in (fwd, bwd):
        for args, msg in (((4, 48, 3, k(4, 4, 16)), "knn_smooth: need C in {32, 64} and 1 <= L <= 4 levels"),
                          ((4, 32, 0, k(4)), "knn_smooth: need C in {32, 64} and 1 <= L <= 4 levels"),
                          ((4, 32, 5, k(1, 1, 1, 1, 1)), "knn_smooth: need C in {32, 64} and 1 <= L <= 4 levels"),
                          ((-1, 32, 1, k(4)), "knn_smooth: need C in {32, 64} and 1 <= L <= 4 levels"),
                          ((4, 32, 1, None), "knn_smooth: need C in {32, 64} and 1 <= L <= 4 levels"),
                          ((4, 64, 3, k(4, 0, 16)), "knn_smooth: need 1 <= k <= 32 in every level"),
                          ((4, 64, 3, k(16, 16, 1)), "knn_smooth: need sum of level k <= 32"),
                          ((1 << 27, 32, 3, k(4, 4, 16)), "knn_smooth: more than 2^27 Gaussians")):
            assert call(*args) != 0, args
            assert _lib.last_error() == msg, args
        assert call(0, 32, 3, k(4, 4, 16)) == 0            # P == 0: nothing to do, no launch
    assert {"mi_knn_smooth_multi_forward", "mi_knn_smooth_multi_backward"} <= set(_lib.ALL_EXPORTS)
