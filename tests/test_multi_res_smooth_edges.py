"""Multi-resolution KNN feature smoothing (csrc/knn_smooth.h: knn_smooth_multi_{fwd,bwd_ret,bwd_feat}_kernel, mi_knn_smooth_multi_*,
knn_smooth._MultiResSmooth) at its edges: every number of levels, a level of k = 1 at either end, all 32 columns (entry bit 31),
P that does not fill a lane group's wave or workgroup, maps that are no KNN maps (random, one Gaussian through two levels, no
self, a hub, unreferenced rows, nothing but the row itself), the norm clamps and 30 decades of row scale, weights over 12 decades, levels that cancel, rows
and levels of weight zero -- against float64 autograd (tests/multi_res_smooth_ref.py) under the per-group rule of
tests/edge_ref.py (multi_res_check):

    every out row i:                      |product - f64| <= max(4 * E32, 2^-22 * magnitude of the summed terms)
    every dL/dF_j row:                    |product - f64| <= max(4 * E32, 2^-21 * magnitude of the summed terms)
    every dL/dw entry (row under
    normalize_out, where a row's
    entries cancel against each other):   |product - f64| <= max(4 * E32, 2^-22 * magnitude of the summed terms)

E32 is the error of the reference's own expression in float32 torch on the CPU, on that very input and in that group.  The
magnitudes are those of the TERMS (edge_ref.multi_res_magnitudes): a dL/dF_j row is measured against
sum (|w_il| / k_l) |terms of dL/dret_i| / max(|F_j|, 1e-12) over its references, so neither a small-gradient row (dL/dF_j scales
with 1 / |F_j|) nor a row whose terms cancel hides under another row's scale.

Measured on the CPU (test_float32_reference_in_another_order_meets_the_rule, every case below, normalize_out both ways): the same
float32 expression in two other evaluation orders -- the channels permuted and restored; the levels and each level's columns
walked last to first -- meets the rule with the floors as they stand (2^-22 / 2^-21 / 2^-22, none widened).  Worst error / bound:

    order               out rows    dL/dF rows    dL/dw entries    dL/dw rows (normalize_out)
    channels permuted   0.848       0.543         0.430            0.431
    last to first       0.809       0.555         0.431            0.426

(out rows: map-hub, C = 64 and map-random, C = 32, normalize_out; dL/dF rows: norm-edges-weights-spread, C = 32 and map-self-only,
C = 64; dL/dw: levels (32,), P = 4099 and map-hub, C = 32.)  The HIP kernels on an MI355X: 0.899, 0.520, 0.415 and 0.365.

The hub's weights are the absolute values of the usual ones.  Every level mean of the hub is the same vector n_3, so under
normalize_out ret_i = (sum_l w_il) n_3 and dL/dw_i is the dot product of n_3 with a vector orthogonal to it: its float32 error
grows with the cancellation in sum_l w_il, a condition number sum |w_il| / |sum w_il| that the magnitude of the terms does not
carry and that E32 carries only as one sample per row.  With signed weights the channel-permuted order measured error / bound
2.33 at the one row (condition number 95) where E32 happened to be 0.4 * 2^-24 of the terms against an error of 9.3 * 2^-24, while
error / (magnitude * condition number) stayed below 1.8 * 2^-24 in all 2000 rows: a property of that input, not of a floor.
Non-negative weights keep the hub's dL/dw under the rule with condition number 1; signed weights meet every other map.

What the suite found: pass B of the backward (knn_smooth_multi_bwd_feat_kernel) summed a whole inverse list into one plain
float32 running sum.  Where a list holds the same addend many times (map-self-only below; a cloud of one point in
tests/test_multi_res_smooth.py) every step rounds the same way: the kernel was 8.3 (P = 1, C = 64, default levels,
normalize_out: error / bound 1.035 on the GPU) to 11.8 (map-self-only, C = 32: 1.476, 13 of 200 rows over, in a numpy float32
restatement of that kernel's order which gives the GPU's P = 1 figures to the last digit) * 2^-24 of the terms off, above the
dL/dF floor of 8 * 2^-24, where both float32 orders stay below 0.56 of the bound.  The sum is compensated now (Kahan), and the
same two cases give 0.136 and 0.454 on the GPU.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import edge_ref as er
from tests import multi_res_smooth_ref as mref
from tests.test_knn_smooth_edges import _norm_edge_table, _table

LAYOUTS = ((1,), (32,), (1, 31), (31, 1), (1, 1, 1, 1), (29, 1, 1, 1), (8, 8, 8, 8), (4, 4, 16))
PS = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 4099)   # 4099 rows: 8 (C = 32) or 16 (C = 64) lanes each, the last workgroup partial
MAPS = ("random", "two_levels", "no_self", "hub", "unreferenced")
DEFAULT_KS = (4, 4, 16)
RATES = (0.1, 0.5, 1.5, 0.3)


def _hand_levels(idxs):
    """Hand-built maps: every point_mask all true, so a level's idx holds global indices."""
    P = idxs[0].shape[0]
    return [(np.ones(P, dtype=bool), np.ascontiguousarray(i, dtype=np.int64)) for i in idxs]


def _maps(kind, P, Ks, rng):
    idxs = [rng.integers(0, P, size=(P, k)).astype(np.int64) for k in Ks]
    if kind == "two_levels":                       # the same Gaussian through the first and the last level of one row
        idxs[-1][:, Ks[-1] - 1] = idxs[0][:, 0]
    elif kind == "no_self":
        for a in idxs:
            a[:] = rng.integers(0, P - 1, size=a.shape)
            a += a >= np.arange(P)[:, None]
            assert (a != np.arange(P)[:, None]).all()
    elif kind == "hub":                            # every entry of every level is row 3: its inverse list is P * Ktot long
        for a in idxs:
            a[:] = 3
    elif kind == "unreferenced":                   # nobody references the upper half
        idxs = [rng.integers(0, P // 2, size=(P, k)).astype(np.int64) for k in Ks]
    return _hand_levels(idxs)


def _norm_edges(C, spread_weights):
    rng = np.random.default_rng(C)
    F, g, _ = _norm_edge_table(C, rng)
    P = F.shape[0]
    levels = _maps("random", P, DEFAULT_KS, rng)
    w = mref.make_weights("full", P, 3, seed=C)
    if spread_weights:
        w = (w * 10.0 ** rng.uniform(-6, 6, size=w.shape)).astype(np.float32)
    return F, levels, w, g


def _cancelling_levels(C):
    """Two levels with the same map and weights (a, -a): ret is exactly 0, the output exactly 0, dL/dret = g * 1e9 under
    normalize_out, and every dL/dF row is a sum of terms that cancel."""
    rng = np.random.default_rng(C + 1)
    P = 300
    F, g = _table(P, C, rng)
    idx = rng.integers(0, P, size=(P, 5))
    a = rng.normal(size=(P, 1)).astype(np.float32)
    return F, _hand_levels([idx, idx.copy()]), np.concatenate([a, -a], axis=1), g


def _zero_weights(C):
    """Row 40: all weights zero (ret = 0: dL/dret = g / 1e-9 under normalize_out, reaching only that row's dL/dw).  Level 1: its
    whole weight column zero."""
    rng = np.random.default_rng(C + 2)
    P = 300
    F, g = _table(P, C, rng)
    w = mref.make_weights("full", P, 3, seed=C)
    w[40] = 0.0
    w[:, 1] = 0.0
    return F, _maps("random", P, DEFAULT_KS, rng), w, g


def cases():
    """(name, builder) of every parity case; builder() -> (F, levels, w, g).  Shared by the GPU test and by the CPU check that
    the float32 reference in another evaluation order meets the same rule.  Every case runs normalize_out both ways."""
    out = []
    for C in (32, 64):
        for Ks in LAYOUTS:
            def b(C=C, Ks=Ks):
                xyz, F, g, levels = mref.make_case(300, C, Ks, rates=RATES[:len(Ks)], seed=sum(Ks) + 7 * len(Ks) + C)
                return F, levels, mref.make_weights("full", 300, len(Ks), seed=len(Ks)), g
            out.append((f"levels{'_'.join(map(str, Ks))}-C{C}", b))
        for n, P in enumerate(PS):
            def b(C=C, P=P, kind=(None, "full", "row")[n % 3]):
                if P <= 33:                    # real subsets; one smaller than its k is cycled through
                    xyz, F, g, levels = mref.make_case(P, C, DEFAULT_KS, rates=RATES[:3], seed=7 * P + C)
                else:
                    rng = np.random.default_rng(7 * P + C)
                    F, g = _table(P, C, rng)
                    levels = _maps("random", P, DEFAULT_KS, rng)
                return F, levels, mref.make_weights(kind, P, 3, seed=P), g
            out.append((f"P{P}-C{C}", b))

        def b(C=C):
            xyz, F, g, levels = mref.make_case(1, C, DEFAULT_KS, rates=RATES[:3], seed=C)
            return F, levels, mref.make_weights("row", 1, 3, seed=1), g
        out.append((f"P1-shared-C{C}", b))
        for kind in MAPS:
            def b(C=C, kind=kind):
                rng = np.random.default_rng(len(kind) + C)
                P, Ks = 1000, (8, 8, 16) if kind == "hub" else DEFAULT_KS
                F, g = _table(P, C, rng)
                w = mref.make_weights("full", P, 3, seed=len(kind))
                return F, _maps(kind, P, Ks, rng), np.abs(w) if kind == "hub" else w, g     # the hub's weights: module docstring
            out.append((f"map-{kind}-C{C}", b))
        def b(C=C):                                # every column of every level is the row itself: a list of 32 equal addends
            rng = np.random.default_rng(C + 4)
            F, g = _table(200, C, rng)
            return F, _hand_levels([np.repeat(np.arange(200)[:, None], k, axis=1) for k in (8, 8, 16)]), None, g
        out.append((f"map-self-only-C{C}", b))
        out.append((f"norm-edges-C{C}", lambda C=C: _norm_edges(C, False)))
        out.append((f"norm-edges-weights-spread-C{C}", lambda C=C: _norm_edges(C, True)))
        out.append((f"cancel-C{C}", lambda C=C: _cancelling_levels(C)))
        out.append((f"zero-weights-C{C}", lambda C=C: _zero_weights(C)))
    return out


CASES = cases()
CASE_IDS = [c[0] for c in CASES]


def _referenced(levels, P):
    seen = np.zeros(P, bool)
    for pm, idx in levels:
        seen[np.flatnonzero(pm)[np.unique(idx)]] = True
    return seen


def _exact_properties(name, F, levels, normalize_out, out, dF, dw):
    """What must hold exactly, whoever computed it."""
    assert not dF[~_referenced(levels, F.shape[0])].any(), "a row no column references received a gradient"
    if name.startswith("cancel"):
        assert not out.any()
        assert np.isfinite(dF).all() and np.isfinite(dw).all()
    if name.startswith("zero-weights"):
        assert not out[40].any() and np.isfinite(dF).all() and np.isfinite(dw).all()


# ---- CPU: the rule is one float32 itself can meet, it sees a small row, and its yardstick is finite ---------------------------------

@pytest.mark.parametrize("order", ["channels", "reverse"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_float32_reference_in_another_order_meets_the_rule(case, order):
    """The reference expression in float32 in another evaluation order goes through the very check the kernels get.  (Its worst
    figures are in this module's docstring.)"""
    name, build = case
    F, levels, w, g = build()
    kw = {"channel_perm": np.random.default_rng(5).permutation(F.shape[1])} if order == "channels" else {"reverse": True}
    for normalize_out in (True, False):
        out, dF, dw = mref.float32_expression(F, levels, w, normalize_out, g, **kw)
        er.multi_res_check(f"{name} norm={int(normalize_out)} (f32, {order})", F, levels, w, g, normalize_out, out, dF, dw)
        _exact_properties(name, F, levels, normalize_out, out, dF, dw)


def _default_700():
    xyz, F, g, levels = mref.make_case(700, 32, DEFAULT_KS, rates=(0.1, 0.5, 1.5), seed=32 + 700)
    return F, levels, mref.make_weights("full", 700, 3, seed=700), g


def test_rule_rejects_one_small_gradient_row_off_by_2_to_the_minus_12():
    """P = 700, C = 32, default levels, full weights, normalize_out: each of the 70 dL/dF rows of the smallest maximum, multiplied
    by 1 + 2^-12 in the float32 reference's own result, is rejected (one global tolerance of 2e-5 * max |want| passes them all:
    these rows lie below 1 % of the largest)."""
    F, levels, w, g = _default_700()
    out, dF, dw = mref.float32_expression(F, levels, w, True, g)
    er.multi_res_check("P=700 default, unperturbed", F, levels, w, g, True, out, dF, dw)
    want = mref.forward_backward(F, levels, w, True, g)[1]
    small = np.argsort(np.abs(want).max(axis=1))[:70]
    assert np.abs(want[small]).max() < 0.01 * np.abs(want).max()
    for j in small:
        bad = dF.copy()
        bad[j] *= 1.0 + 2.0 ** -12
        assert np.abs(bad - want).max() <= 2e-5 * np.abs(want).max()          # what the single global tolerance sees: nothing
        with pytest.raises(AssertionError, match="dL/dF"):
            er.multi_res_check(f"row {j} * (1 + 2^-12)", F, levels, w, g, True, out, bad, dw)


@pytest.mark.parametrize("C", [32, 64])
def test_float32_reference_is_finite_on_the_norm_edges(C):
    """Zero rows, clamped rows, 30 decades of row scale and 12 decades of weights: E32 is a number in every group."""
    for spread in (False, True):
        F, levels, w, g = _norm_edges(C, spread)
        norms = np.linalg.norm(F.astype(np.float64), axis=1)
        assert (norms == 0).sum() >= 10 and ((norms > 0) & (norms < 1e-12)).sum() >= 30 and norms.max() > 1e12
        for normalize_out in (True, False):
            for a in mref.float32_expression(F, levels, w, normalize_out, g):
                assert np.isfinite(a).all()
            for a in mref.forward_backward(F, levels, w, normalize_out, g):
                assert np.isfinite(a).all()


@pytest.mark.parametrize("name", ["levels4_4_16-C32", "map-hub-C64", "norm-edges-weights-spread-C32", "P33-C64", "P1-shared-C32"])
def test_magnitudes_bound_what_they_measure(name):
    """The magnitude of the terms is never smaller than the sum itself: every |out| element and every |dL/dw| entry of the float64
    truth lies under its group's magnitude."""
    F, levels, w, g = dict(CASES)[name]()
    for normalize_out in (True, False):
        out, dF, dw = mref.forward_backward(F, levels, w, normalize_out, g)
        mag_o, mag_g, mag_w = er.multi_res_magnitudes(F, levels, w, g, normalize_out)
        assert mag_o.shape == (F.shape[0],) and mag_g.shape == (F.shape[0],)
        assert (np.abs(out).max(axis=1) <= mag_o * (1 + 1e-12)).all()
        assert (mag_g[_referenced(levels, F.shape[0])] > 0).all() and not mag_g[~_referenced(levels, F.shape[0])].any()
        if w is not None:
            assert mag_w.shape == (dw.shape[:1] if normalize_out else dw.shape)
            assert (np.abs(dw) <= (mag_w[:, None] if normalize_out else mag_w) * (1 + 1e-9)).all()


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

def _dev():
    return torch.device("cuda:0")


def _mrmap(levels):
    from seganygaussians_amd import knn_smooth as ks
    return ks.MultiResNeighbourMap([(torch.as_tensor(pm), torch.as_tensor(idx).to(_dev())) for pm, idx in levels])


def _gpu(F, levels, w, g, normalize_out, mr=None):
    from seganygaussians_amd import knn_smooth as ks
    dev = _dev()
    f = torch.tensor(F, device=dev, requires_grad=True)
    wt = None if w is None else torch.tensor(w, device=dev, requires_grad=True)
    out = ks.multi_res_smooth_point_features(f, _mrmap(levels) if mr is None else mr, wt, normalize_out)
    out.backward(torch.tensor(g, device=dev))
    return out.detach().cpu().numpy(), f.grad.cpu().numpy(), None if wt is None else wt.grad.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_hip_meets_the_rule(case):
    """Forward and backward of the HIP kernels, normalize_out both ways, every group under the rule.  Rows nobody references get
    dL/dF exactly 0; levels that cancel and a row of zero weights give exactly 0 out and finite gradients."""
    name, build = case
    F, levels, w, g = build()
    mr = _mrmap(levels)
    for normalize_out in (True, False):
        out, dF, dw = _gpu(F, levels, w, g, normalize_out, mr)
        er.multi_res_check(f"{name} norm={int(normalize_out)}", F, levels, w, g, normalize_out, out, dF, dw)
        _exact_properties(name, F, levels, normalize_out, out, dF, dw)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [32, 64])
def test_hip_zero_weight_level_is_inert(C):
    """Level 1's weight column is zero and the last 40 rows are reachable only through level 1: changing their features changes
    no out row and no other dL/dF row, and their own dL/dF is exactly 0."""
    rng = np.random.default_rng(C)
    P = 500
    F, g = _table(P, C, rng)
    idxs = [rng.integers(0, P - 40, size=(P, k)) for k in DEFAULT_KS]
    idxs[1] = rng.integers(P - 40, P, size=(P, 4))
    levels = _hand_levels(idxs)
    w = mref.make_weights("full", P, 3, seed=C)
    w[:, 1] = 0.0
    F2 = F.copy()
    F2[P - 40:] = rng.normal(size=(40, C)).astype(np.float32) * 100.0
    F2[P - 1] = 0.0
    mr = _mrmap(levels)
    for normalize_out in (True, False):
        out, dF, dw = _gpu(F, levels, w, g, normalize_out, mr)
        out2, dF2, dw2 = _gpu(F2, levels, w, g, normalize_out, mr)
        assert np.array_equal(out, out2)
        assert np.array_equal(dF[:P - 40], dF2[:P - 40])
        assert not dF[P - 40:].any() and not dF2[P - 40:].any()
        er.multi_res_check(f"inert level C{C} norm={int(normalize_out)}", F2, levels, w, g, normalize_out, out2, dF2, dw2)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [32, 64])
def test_hip_is_deterministic(C):
    """No atomics anywhere: two runs agree bit for bit in out, dL/dF and dL/dw -- also through a hub's P * Ktot long list."""
    for kind in ("random", "hub"):
        for wkind in ("full", "row"):
            rng = np.random.default_rng(C)
            P, Ks = 1000, (8, 8, 16)
            F, g = _table(P, C, rng)
            levels = _maps(kind, P, Ks, rng)
            w = mref.make_weights(wkind, P, 3, seed=C)
            mr = _mrmap(levels)
            a, b = _gpu(F, levels, w, g, True, mr), _gpu(F, levels, w, g, True, mr)
            for x, y in zip(a, b):
                assert _same_bits(x, y), (kind, wkind)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [32, 64])
def test_hip_takes_views_like_their_contiguous_copies(C):
    """A transposed view as the feature tensor and a column slice as the weight tensor: the same bits as their contiguous copies,
    and the gradients arrive in the views' own layout."""
    from seganygaussians_amd import knn_smooth as ks
    dev = _dev()
    rng = np.random.default_rng(C + 3)
    P = 333
    F, g = _table(P, C, rng)
    levels = _maps("random", P, DEFAULT_KS, rng)
    w = mref.make_weights("full", P, 3, seed=C)
    mr = _mrmap(levels)
    gt = torch.tensor(g, device=dev)
    for normalize_out in (True, False):
        want = _gpu(F, levels, w, g, normalize_out, mr)
        base = torch.tensor(np.ascontiguousarray(F.T), device=dev, requires_grad=True)            # (C, P)
        wide = torch.zeros(P, 5, device=dev)
        wide[:, 1:4] = torch.tensor(w, device=dev)
        wide.requires_grad_(True)
        f, wt = base.t(), wide[:, 1:4]
        assert not f.is_contiguous() and not wt.is_contiguous()
        out = ks.multi_res_smooth_point_features(f, mr, wt, normalize_out)
        out.backward(gt)
        assert _same_bits(out.detach().cpu().numpy(), want[0])
        assert _same_bits(np.ascontiguousarray(base.grad.t().cpu().numpy()), want[1])
        assert _same_bits(np.ascontiguousarray(wide.grad[:, 1:4].cpu().numpy()), want[2])
        assert not wide.grad[:, 0].any() and not wide.grad[:, 4].any()


GUARD, MARK = 64, 0x5A5A5A5A


def _guarded(n):
    """n float32 words to write into, GUARD canary words past the end; (whole int32 tensor, pointer to its start)."""
    t = torch.full((n + GUARD,), MARK, dtype=torch.int32, device=_dev())
    return t, ctypes.c_void_p(t.data_ptr())


def _abi_inputs(P, C):
    rng = np.random.default_rng(P + C)
    F, g = _table(P, C, rng)
    levels = _maps("random", P, DEFAULT_KS, rng)
    w = mref.make_weights("full", P, 3, seed=P)
    dev = _dev()
    return F, levels, w, g, _mrmap(levels), torch.tensor(F, device=dev), torch.tensor(g, device=dev), torch.tensor(w, device=dev)


@pytest.mark.gpu
@pytest.mark.parametrize("want_dw", [False, True])
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("P", [33, 257])
def test_guard_words_stay_intact(P, C, want_dw):
    """Through the C ABI, with out, dret, dL/dF and dL/dw each followed by 64 canary words: the kernels write their P * C (P * L)
    words -- the same bits the autograd function gives -- and nothing past the end; P = 33 and 257 leave the last workgroup
    partial at both widths."""
    from seganygaussians_amd import _lib
    lib = _lib.load()
    F, levels, w, g, mr, f, gt, wt = _abi_inputs(P, C)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = torch.cuda.current_stream(_dev()).cuda_stream
    for normalize_out in (1, 0):
        out, out_p = _guarded(P * C)
        dret, dret_p = _guarded(P * C)
        dF, dF_p = _guarded(P * C)
        dw, dw_p = _guarded(P * 3)
        assert lib.mi_knn_smooth_multi_forward(P, C, mr.L, mr.level_k_c, p(mr.nmap.idx), p(wt), 0, p(f), out_p, normalize_out, stream) == 0, _lib.last_error()
        assert lib.mi_knn_smooth_multi_backward(P, C, mr.L, mr.level_k_c, p(mr.nmap.idx), p(mr.nmap.inv_offsets), p(mr.nmap.inv_entries), p(wt), 0,
                                                p(f), p(gt), dret_p, dF_p, dw_p if want_dw else None, normalize_out, stream) == 0, _lib.last_error()
        torch.cuda.synchronize()
        for name, t, n in (("out", out, P * C), ("dret", dret, P * C), ("dL_dF", dF, P * C), ("dL_dw", dw, P * 3)):
            assert (t[n:] == MARK).all(), f"{name}: words past the end were written"
        assert want_dw or (dw == MARK).all()
        want = _gpu(F, levels, w, g, bool(normalize_out), mr)
        assert np.array_equal(out[:P * C].cpu().numpy().view(np.uint32), want[0].reshape(-1).view(np.uint32))
        assert np.array_equal(dF[:P * C].cpu().numpy().view(np.uint32), want[1].reshape(-1).view(np.uint32))
        if want_dw:
            assert np.array_equal(dw[:P * 3].cpu().numpy().view(np.uint32), want[2].reshape(-1).view(np.uint32))


@pytest.mark.gpu
def test_c_abi_refusals_launch_nothing():
    """L = 0 and 5, a level of k = 0, levels that sum to 33, C = 48 and a NULL map are refused with their message, by both entry
    points, with every output still untouched afterwards; P = 0 returns 0 and touches nothing either."""
    from seganygaussians_amd import _lib
    lib = _lib.load()
    P, C = 33, 32
    F, levels, w, g, mr, f, gt, wt = _abi_inputs(P, C)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    k = lambda *v: (ctypes.c_int * len(v))(*v)
    stream = torch.cuda.current_stream(_dev()).cuda_stream
    out, out_p = _guarded(P * 64)
    dret, dret_p = _guarded(P * 64)
    dF, dF_p = _guarded(P * 64)
    dw, dw_p = _guarded(P * 5)
    idx = p(mr.nmap.idx)
    fwd = lambda P, C, L, lk, m: lib.mi_knn_smooth_multi_forward(P, C, L, lk, m, p(wt), 0, p(f), out_p, 1, stream)
    bwd = lambda P, C, L, lk, m: lib.mi_knn_smooth_multi_backward(P, C, L, lk, m, p(mr.nmap.inv_offsets), p(mr.nmap.inv_entries), p(wt), 0, p(f),
                                                                  p(gt), dret_p, dF_p, dw_p, 1, stream)
    levels_msg = "knn_smooth: need C in {32, 64} and 1 <= L <= 4 levels"
    for call, null_msg in ((fwd, "knn_smooth: need a neighbour map, features and an output"),
                           (bwd, "knn_smooth: need a neighbour map, its inverse lists, features, a gradient, scratch and an output")):
        for args, msg in (((P, C, 0, k(4), idx), levels_msg),
                          ((P, C, 5, k(4, 4, 4, 4, 4), idx), levels_msg),
                          ((P, C, 3, k(4, 0, 16), idx), "knn_smooth: need 1 <= k <= 32 in every level"),
                          ((P, C, 3, k(16, 16, 1), idx), "knn_smooth: need sum of level k <= 32"),
                          ((P, 48, 3, k(4, 4, 16), idx), levels_msg),
                          ((P, C, 3, k(4, 4, 16), None), null_msg)):
            assert call(*args) != 0, args
            assert _lib.last_error() == msg, args
        assert call(0, C, 3, k(4, 4, 16), idx) == 0
    torch.cuda.synchronize()
    for t in (out, dret, dF, dw):
        assert (t == MARK).all()
    assert fwd(P, C, 3, mr.level_k_c, idx) == 0, _lib.last_error()           # and a refusal leaves nothing behind
    torch.cuda.synchronize()
    assert (out[:P * C] != MARK).any() and (out[P * C:] == MARK).all()
