"""KNN feature smoothing (csrc/knn_smooth.h) at the edges of its C ABI: every K from 1 to 32, column subsets up to mask bit 31,
P that does not fill a lane group's wave or workgroup, index maps that are no KNN maps (random, duplicates, no self, a hub,
unreferenced rows), the norm clamps, and row scales from 1e-15 to 1e15 in one table -- against the float64 oracle
(oracle/knn_smooth_oracle.py) under the per-row rule of tests/edge_ref.py:

    every output row i:           |product - f64| <= max(4 * E32, 2^-22 * magnitude of the summed terms)
    every gradient row dL/dF_j:   |product - f64| <= max(4 * E32, 2^-21 * magnitude of the summed terms)

E32 is the error of the reference's own PyTorch expression in float32 on the CPU, on that very input.  The magnitude of a
dL/dF_j row is sum |dL/dm rows that reference j| / max(|F_j|, 1e-12), so neither a small-gradient row (dL/dF_j scales with
1 / |F_j|) nor a row whose terms cancel hides under another row's scale.

Measured on the CPU (test_float32_reference_in_another_order_meets_the_rule, every case below): the same float32 expression in a
second evaluation order (channels permuted, columns gathered last to first) meets 4 * E32 on the out rows with the floor at 2^-22
of the terms (it needs 3.9 * 2^-24), but not on the dL/dF rows: a row of 32 or 64 elements is a small sample, and where E32 happens
to be small the other order lies up to 4.7 * 2^-24 of the terms away from float64 (map-duplicates, C = 64).  As the rule says, the
floor is widened there, not the factor: 2^-21 of the terms for dL/dF rows (edge_ref.KNN_GRAD_FLOOR).  With it the second order's
worst error / bound is 0.96 (out rows) and 0.59 (dL/dF rows)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import knn_smooth_oracle as ko
from tests import edge_ref as er
from tests.test_knn_smooth import _reference_expression

KS = (1, 2, 5, 16, 31, 32)
PS = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 4099)   # 4099 rows: 8 (C = 32) or 16 (C = 64) lanes each, the last workgroup partial
MAPS = ("random", "duplicates", "no_self", "hub", "unreferenced")


def _table(P, C, rng, lo=0.1, hi=3.0):
    F = rng.normal(size=(P, C)).astype(np.float32) * rng.uniform(lo, hi, size=(P, 1)).astype(np.float32)
    return F, rng.normal(size=(P, C)).astype(np.float32)


def _map(kind, P, K, rng):
    idx = rng.integers(0, P, size=(P, K)).astype(np.int64)
    if kind == "duplicates":                       # the same j two or three times in a row
        if K >= 2:
            idx[:, K - 1] = idx[:, 0]
        if K >= 3:
            idx[::2, K // 2] = idx[::2, 0]
    elif kind == "no_self":
        idx = rng.integers(0, P - 1, size=(P, K)).astype(np.int64)
        idx += idx >= np.arange(P)[:, None]
        assert (idx != np.arange(P)[:, None]).all()
    elif kind == "hub":                            # every entry of the map is row 3: its inverse list is P K long
        idx[:] = 3
    elif kind == "unreferenced":                   # nobody references the upper half
        idx = rng.integers(0, P // 2, size=(P, K)).astype(np.int64)
    return idx


def _column_sets(K):
    sets = {"single": (K // 2,), "last": (K - 1,), "all": tuple(range(K))}
    if K == 32:
        sets["with_31"] = (0, 7, 30, 31)          # mask bit 31 through ctypes and the `ent & 31` decode
    return sets


def _norm_edge_table(C, rng):
    """Zero rows, rows under the 1e-12 clamp of F.normalize, rows just above it, and scales from 1e-15 to 1e15: float32 squares
    between 1e-30 and 1e30, their sums over 64 channels far from both ends of the float32 range."""
    P = 600
    F, g = _table(P, C, rng, 1.0, 1.0)
    unit = F / np.linalg.norm(F.astype(np.float64), axis=1, keepdims=True)
    F = unit * 10.0 ** rng.uniform(-15, 15, size=(P, 1))
    F[0:10] = 0.0
    F[10:30] = unit[10:30] * 1e-14                 # |F| < 1e-12: the clamp branch, dF = s * 1e12
    F[30:40] = unit[30:40] * 0.7e-12
    F[40:60] = unit[40:60] * 1.5e-12               # just above: the ordinary branch
    F[60], F[61] = unit[60] * 1e-15, unit[61] * 1e15
    return F.astype(np.float32), g, _map("random", P, 5, rng)


def _cancelling_pairs(C, rng):
    """k = 2 and the two neighbours exactly n and -n: m = 0, the output is exactly 0 and dm = g * 1e9 (normalize_out)."""
    P = 64
    F, g = _table(P, C, rng)
    F[1::2] = -F[0::2]
    t = rng.integers(0, P // 2, size=P)
    return F, g, np.stack([2 * t, 2 * t + 1], axis=1).astype(np.int64)


def cases():
    """(name, C, builder) of every parity case; builder() -> (F, idx, g, cols).  Shared by the GPU test and by the CPU check that
    the float32 reference in another evaluation order meets the same rule."""
    out = []
    for C in (32, 64):
        for K in KS:
            for cname, cols in _column_sets(K).items():
                def b(C=C, K=K, cols=cols):
                    rng = np.random.default_rng(1000 * K + C)
                    F, g = _table(300, C, rng)
                    return F, _map("random", 300, K, rng), g, cols
                out.append((f"K{K}-{cname}-C{C}", C, b))
        for P in PS:
            def b(C=C, P=P):
                rng = np.random.default_rng(7 * P + C)
                F, g = _table(P, C, rng)
                return F, _map("random", P, 5, rng), g, (0, 2, 4) if P % 2 else tuple(range(5))
            out.append((f"P{P}-C{C}", C, b))
        for kind in MAPS:
            def b(C=C, kind=kind):
                rng = np.random.default_rng(len(kind) + C)
                F, g = _table(3000, C, rng)
                return F, _map(kind, 3000, 16, rng), g, (3, 0, 7, 12, 9, 15, 1, 4) if kind != "hub" else tuple(range(16))
            out.append((f"map-{kind}-C{C}", C, b))

        def b(C=C):
            F, g, idx = _norm_edge_table(C, np.random.default_rng(C))
            return F, idx, g, (0, 1, 3, 4)
        out.append((f"norm-edges-C{C}", C, b))

        def b(C=C):
            F, g, idx = _cancelling_pairs(C, np.random.default_rng(C + 1))
            return F, idx, g, (0, 1)
        out.append((f"cancel-C{C}", C, b))
    return out


CASES = cases()
CASE_IDS = [c[0] for c in CASES]


# ---- CPU: the oracle is general, the float32 reference is finite, and the rule is one float32 itself can meet -------------------

@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("K", KS)
def test_oracle_takes_any_k_and_any_map(K, kind):
    """oracle/knn_smooth_oracle.py against the reference expression by float64 autograd (tests/test_knn_smooth.py) for every K
    and for maps with duplicates, without self, with a hub and with unreferenced rows."""
    rng = np.random.default_rng(K)
    F, g = _table(200, 32, rng)
    idx = _map(kind, 200, K, rng)
    for cols in _column_sets(K).values():
        for normalize_out in (True, False):
            f, ret = _reference_expression(F, idx, cols, normalize_out)
            ret.backward(torch.tensor(g, dtype=torch.float64))
            np.testing.assert_allclose(ko.forward(F, idx, cols, normalize_out), ret.detach().numpy(), rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(ko.backward(F, idx, cols, g, normalize_out), f.grad.numpy(), rtol=1e-9, atol=1e-11)


@pytest.mark.parametrize("C", [32, 64])
def test_oracle_and_float32_reference_on_the_norm_edges(C):
    """The oracle equals float64 autograd on zero rows, clamped rows and 30 decades of row scale -- and the float32 reference
    stays finite there, so E32 is a number.  With n and -n as the only neighbours both give exactly 0 and the zero subgradient."""
    F, g, idx = _norm_edge_table(C, np.random.default_rng(C))
    for normalize_out in (True, False):
        f, ret = _reference_expression(F, idx, (0, 1, 3, 4), normalize_out)
        ret.backward(torch.tensor(g, dtype=torch.float64))
        want = ko.backward(F, idx, (0, 1, 3, 4), g, normalize_out)
        np.testing.assert_allclose(ko.forward(F, idx, (0, 1, 3, 4), normalize_out), ret.detach().numpy(), rtol=1e-12, atol=1e-13)
        assert (np.abs(want - f.grad.numpy()).max(axis=1) <= 1e-9 * np.abs(want).max(axis=1)).all()      # per row: 30 decades of scale
        o32, g32 = er.knn_expression(F, idx, (0, 1, 3, 4), normalize_out, g, torch.float32)
        assert np.isfinite(o32).all() and np.isfinite(g32).all()
    F, g, idx = _cancelling_pairs(C, np.random.default_rng(C + 1))
    f, ret = _reference_expression(F, idx, (0, 1), True)
    ret.backward(torch.tensor(g, dtype=torch.float64))
    assert not ret.detach().numpy().any() and not ko.forward(F, idx, (0, 1), True).any()
    np.testing.assert_allclose(ko.backward(F, idx, (0, 1), g, True), f.grad.numpy(), rtol=1e-9)
    o32, g32 = er.knn_expression(F, idx, (0, 1), True, g, torch.float32)
    assert not o32.any() and np.isfinite(g32).all()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_float32_reference_in_another_order_meets_the_rule(case):
    """The rule must be one that float32 can meet: the reference expression in float32 with the channels permuted and the columns
    gathered last to first is put through the very check the kernels get.  (Its figures are in this module's docstring.)"""
    name, C, build = case
    F, idx, g, cols = build()
    perm = np.random.default_rng(5).permutation(C)
    for normalize_out in (True, False):
        out, dF = er.knn_expression(F, idx, cols, normalize_out, g, torch.float32, channel_perm=perm, reverse_cols=True)
        er.knn_check(f"{name} norm={int(normalize_out)} (f32, second order)", F, idx, cols, g, normalize_out, out, dF)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

def _gpu(F, idx, g, cols, normalize_out):
    from seganygaussians_amd import knn_smooth as ks
    dev = torch.device("cuda:0")
    f = torch.tensor(F, device=dev, requires_grad=True)
    nmap = ks.NeighbourMap(torch.tensor(idx, device=dev))
    out = ks.smooth_point_features(f, nmap, cols, normalize_out)
    out.backward(torch.tensor(g, device=dev))
    return out.detach().cpu().numpy(), f.grad.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_hip_meets_the_rule(case):
    """Forward and backward of the HIP kernels, normalize_out both ways, every row under the rule.  Rows nobody references get
    dL/dF exactly 0; neighbours n and -n give exactly 0 out."""
    name, C, build = case
    F, idx, g, cols = build()
    for normalize_out in (True, False):
        out, dF = _gpu(F, idx, g, cols, normalize_out)
        er.knn_check(f"{name} norm={int(normalize_out)}", F, idx, cols, g, normalize_out, out, dF)
        referenced = np.zeros(F.shape[0], bool)
        referenced[np.unique(idx[:, list(cols)])] = True
        assert not dF[~referenced].any(), "a row no selected column references received a gradient"
        if name.startswith("cancel") and normalize_out:
            assert not out.any()


@pytest.mark.gpu
@pytest.mark.parametrize("C", [32, 64])
def test_hip_unselected_columns_are_inert(C):
    """Rows reachable only through unselected columns: changing their features changes no output row and no dL/dF row, bit for
    bit (their own dL/dF is exactly 0: no selected column references them)."""
    rng = np.random.default_rng(C)
    P, K, cols = 500, 6, (0, 2, 5)
    F, g = _table(P, C, rng)
    idx = rng.integers(0, P - 40, size=(P, K)).astype(np.int64)
    idx[:, [1, 3, 4]] = rng.integers(P - 40, P, size=(P, 3))          # the last 40 rows: only through columns 1, 3, 4
    F2 = F.copy()
    F2[P - 40:] = rng.normal(size=(40, C)).astype(np.float32) * 100.0
    F2[P - 1] = 0.0
    for normalize_out in (True, False):
        out, dF = _gpu(F, idx, g, cols, normalize_out)
        out2, dF2 = _gpu(F2, idx, g, cols, normalize_out)
        assert np.array_equal(out.view(np.uint32), out2.view(np.uint32))
        assert np.array_equal(dF.view(np.uint32), dF2.view(np.uint32))
        assert not dF[P - 40:].any()
        er.knn_check(f"inert C{C} norm={int(normalize_out)}", F2, idx, cols, g, normalize_out, out2, dF2)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [32, 64])
def test_hip_is_deterministic(C):
    """No atomics anywhere: two runs agree bit for bit, forward and backward -- also through a hub's P K long inverse list."""
    for kind in ("random", "hub"):
        rng = np.random.default_rng(C)
        F, g = _table(3000, C, rng)
        idx = _map(kind, 3000, 16, rng)
        a, b = _gpu(F, idx, g, None, True), _gpu(F, idx, g, None, True)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.gpu
def test_hip_refusals():
    from seganygaussians_amd import _lib
    from seganygaussians_amd import knn_smooth as ks
    dev = torch.device("cuda:0")
    idx = torch.randint(0, 50, (50, 4), device=dev)
    nmap = ks.NeighbourMap(idx)
    for C in (16, 31, 33, 48, 128):
        with pytest.raises(RuntimeError, match=r"knn_smooth: need C in \{32, 64\} and 1 <= K <= 32"):
            ks.smooth_point_features(torch.randn(50, C, device=dev), nmap)
    for K in (0, 33):
        with pytest.raises(ValueError, match=r"knn_idx must have shape \(P, K\) with 1 <= K <= 32"):
            ks.NeighbourMap(torch.zeros((50, K), dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError, match="knn_smooth: no neighbour column selected"):
        ks.smooth_point_features(torch.randn(50, 32, device=dev), nmap, cols=())
    with pytest.raises(ValueError, match="neighbour column 4 outside"):
        ks.smooth_point_features(torch.randn(50, 32, device=dev), nmap, cols=(4,))
    for bad in (-1, 50):
        broken = idx.clone()
        broken[7, 2] = bad
        with pytest.raises(ValueError, match=r"knn_idx holds indices outside \[0, P\)"):
            ks.NeighbourMap(broken)
    with pytest.raises(ValueError, match="features has 49 rows, the neighbour map 50"):
        ks.smooth_point_features(torch.randn(49, 32, device=dev), nmap)
    # the C ABI itself refuses K = 0 and K = 33 before it launches anything (both entry points)
    L = _lib.load()
    f = torch.randn(50, 32, device=dev)
    o = torch.empty_like(f)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for K in (0, 33):
        assert L.mi_knn_smooth_forward(50, 32, K, p(nmap.idx), 1, p(f), p(o), 1, None) != 0
        assert "1 <= K <= 32" in _lib.last_error()
        assert L.mi_knn_smooth_backward(50, 32, K, p(nmap.idx), p(nmap.inv_offsets), p(nmap.inv_entries), 1, p(f), p(f), p(o), p(o), 1,
                                        None) != 0
        assert "1 <= K <= 32" in _lib.last_error()
    assert L.mi_knn_smooth_backward(50, 32, 4, p(nmap.idx), p(nmap.inv_offsets), p(nmap.inv_entries), 0, p(f), p(f), p(o), p(o), 1, None) != 0
    assert "no neighbour column selected" in _lib.last_error()
