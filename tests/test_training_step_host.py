"""CPU checks of the fused training step (seganygaussians_amd/training_step.py): the exports and the argument
checks of the C-ABI before any HIP call, the float64 restatements of tests/training_step_ref.py (Adam against torch.optim.Adam,
densify_and_prune on a hand-made table), FusedAdam on CPU tensors (the fallback), and the opt-in patch of install_dropin.  No GPU."""
import copy
import ctypes as C
import importlib
import os
import re
import sys

import numpy as np
import pytest
import torch

import seganygaussians_amd
from seganygaussians_amd import _lib, build
from seganygaussians_amd import training_step as ts
from tests import training_step_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def test_exports_are_mi_train_step_h(lib):
    hdr = open(os.path.join(ROOT, "include", "mi_train_step.h")).read()
    declared = set(re.findall(r"\b(mi_train_[a-z_0-9]+)\s*\(", hdr))
    assert declared == {"mi_train_adam_step", "mi_train_densify_stats", "mi_train_densify_workspace_bytes", "mi_train_densify_plan",
                        "mi_train_densify_counts", "mi_train_densify_apply"} <= set(_lib.ALL_EXPORTS)
    assert _lib.DECLARED["mi_train_step.h"] == ["mi_train_adam_step", "mi_train_densify_stats", "mi_train_densify_workspace_bytes",
                                                "mi_train_densify_plan", "mi_train_densify_counts", "mi_train_densify_apply"]
    assert "mi_train" not in open(os.path.join(ROOT, "include", "mi_rast.h")).read().lower()       # a header of its own
    for name in declared:
        assert C.cast(getattr(lib, name), C.c_void_p).value
    assert "train_step.h" in build.SOURCES and "mi_train_step.hip" in build.SOURCES
    includers = [f for f in build.SOURCES if '"train_step.h"' in open(os.path.join(build.SRC_DIR, f)).read()]
    assert includers == ["mi_train_step.hip"]
    assert (_lib.MI_TRAIN_XYZ, _lib.MI_TRAIN_SCALING, _lib.MI_TRAIN_ROTATION) == tuple(ts.GROUP_KINDS[k] for k in ("xyz", "scaling", "rotation"))
    assert ts.GROUP_KINDS == {"xyz": 2, "scaling": 3, "rotation": 4} and ts.ADAM_MAX_TENSORS == _lib.MI_TRAIN_ADAM_MAX_TENSORS == 16
    assert "#define MI_TRAIN_ADAM_MAX_TENSORS 16\n" in hdr and "#define MI_TRAIN_DENSIFY_MAX_TENSORS 32\n" in hdr
    for k, name in enumerate(("MI_TRAIN_COPY", "MI_TRAIN_MOMENT", "MI_TRAIN_XYZ", "MI_TRAIN_SCALING", "MI_TRAIN_ROTATION")):
        assert re.search(rf"{name} = {k}\b", hdr)


def _tab(vals):
    return (C.c_void_p * len(vals))(*vals)


def test_adam_refused_before_any_hip_call(lib):
    f = lib.mi_train_adam_step
    one = lambda v: _tab([v])
    n1, s1 = (C.c_size_t * 1)(64), (C.c_double * 1)(1e-3)
    ok = (one(4096), one(8192), one(12288), one(16384), n1, s1, 1.0, 0.9, 0.999, 1e-15, None)

    def refused(args, msg):
        assert f(*args) != 0 and msg in _lib.last_error(), _lib.last_error()

    refused((0,) + ok, "n_tensors <= 16")
    p17 = _tab([4096 * (k + 1) for k in range(17)])
    refused((17, p17, p17, p17, p17, (C.c_size_t * 17)(), (C.c_double * 17)(), 1.0, 0.9, 0.999, 1e-15, None), "n_tensors <= 16")
    refused((1, None) + ok[1:], "null table")
    refused((1, one(None)) + ok[1:], "null pointer")
    refused((1,) + ok[:6] + (1.0, 1.0, 0.999, 1e-15, None), "beta")
    refused((1,) + ok[:6] + (1.0, 0.9, 0.999, -1.0, None), "eps")
    refused((1,) + ok[:6] + (float("nan"), 0.9, 0.999, 1e-15, None), "eps")
    refused((1, one(4098)) + ok[1:], "4-byte aligned")
    refused((1, one(4096), one(4096 + 128)) + ok[2:], "overlaps")                          # the gradient inside the parameter
    refused((1, one(4096), one(8192), one(8192 + 252)) + ok[3:], "overlaps")               # exp_avg reaches into the gradient's last float
    refused((1,) + ok[:5] + ((C.c_double * 1)(float("inf")), 1.0, 0.9, 0.999, 1e-15, None), "step size")
    # a call whose tensors are all empty does nothing and succeeds without a device
    assert f(1, one(None), one(None), one(None), one(None), (C.c_size_t * 1)(0), s1, 1.0, 0.9, 0.999, 1e-15, None) == 0


def test_stats_and_densify_refused_before_any_hip_call(lib):
    st = lib.mi_train_densify_stats
    assert st(-1, 8, 8, 8, 8, None, None) != 0 and "negative" in _lib.last_error()
    assert st(4, None, 8, 8, 8, None, None) != 0 and "null" in _lib.last_error()
    assert st(4, 4096, 8192, 4096 + 8, 16384, None, None) != 0 and "overlaps" in _lib.last_error()
    assert st(0, None, None, None, None, None, None) == 0
    wsb = lib.mi_train_densify_workspace_bytes
    assert wsb(0) == 0 and wsb(-5) == 0 and wsb(1 << 30) == 0
    assert wsb(1) > 0 and wsb(1000) >= 1000 + 3 * 4 * 1000 and wsb(1 << 20) < 20 * (1 << 20)
    need = wsb(1000)
    plan = lib.mi_train_densify_plan
    base = dict(P=1000, accum=1 << 20, denom=2 << 20, scaling=3 << 20, opacity=4 << 20, max_grad=2e-4, min_opacity=0.005, extent=5.0,
                percent_dense=0.01, screen=1, ws=8 << 20, ws_bytes=need, split_rows=16 << 20, stream=None)

    def refused(fn, args, msg):
        assert fn(*args.values()) != 0 and msg in _lib.last_error(), _lib.last_error()

    refused(plan, dict(base, P=0), "1 <= P")
    refused(plan, dict(base, ws=None), "null")
    refused(plan, dict(base, ws_bytes=need - 1), "workspace smaller")
    refused(plan, dict(base, opacity=None), "null")
    refused(plan, dict(base, split_rows=None), "null")
    refused(plan, dict(base, max_grad=0.0), "max_grad must be > 0")
    refused(plan, dict(base, max_grad=-1.0), "max_grad must be > 0")
    refused(plan, dict(base, extent=float("nan")), "NaN")
    refused(plan, dict(base, split_rows=(8 << 20) + 64), "overlaps")
    refused(plan, dict(base, scaling=(8 << 20) + need - 4), "overlaps")
    counts = lib.mi_train_densify_counts
    assert counts(1000, 8 << 20, need, None, None) != 0 and "null" in _lib.last_error()
    assert counts(1000, 8 << 20, 16, (C.c_int * 5)(), None) != 0 and "workspace smaller" in _lib.last_error()
    apply = lib.mi_train_densify_apply
    src, dst = _tab([(32 + k) << 20 for k in range(3)]), _tab([(64 + k) << 20 for k in range(3)])
    cols, kinds = (C.c_int * 3)(3, 3, 4), (C.c_int * 3)(_lib.MI_TRAIN_XYZ, _lib.MI_TRAIN_SCALING, _lib.MI_TRAIN_ROTATION)
    good = (C.c_int * 5)(100, 50, 900, 90, 40)
    ab = dict(P=1000, counts=good, n=3, src=src, dst=dst, cols=cols, kinds=kinds, samples=128 << 20, ws=8 << 20, ws_bytes=need, stream=None)
    refused(apply, dict(ab, counts=None), "null table")
    refused(apply, dict(ab, n=2), "n_tensors")
    refused(apply, dict(ab, n=33), "n_tensors")
    refused(apply, dict(ab, counts=(C.c_int * 5)(100, 50, 990, 90, 40)), "counts are not")     # kept originals + splits > P
    refused(apply, dict(ab, counts=(C.c_int * 5)(100, 50, 900, 90, 51)), "counts are not")     # more kept pairs than splits
    refused(apply, dict(ab, counts=(C.c_int * 5)(100, 50, 900, -1, 40)), "counts are not")
    refused(apply, dict(ab, samples=None), "samples")
    refused(apply, dict(ab, cols=(C.c_int * 3)(3, 3, 3)), "rotation has 4 columns")
    refused(apply, dict(ab, cols=(C.c_int * 3)(3, 0, 4)), "cols")
    refused(apply, dict(ab, kinds=(C.c_int * 3)(0, 3, 4)), "exactly one xyz")
    refused(apply, dict(ab, kinds=(C.c_int * 3)(2, 3, 7)), "unknown tensor kind")
    refused(apply, dict(ab, dst=_tab([64 << 20, 32 << 20, 66 << 20])), "overlaps")              # a destination on a source
    refused(apply, dict(ab, src=_tab([32 << 20, None, 34 << 20])), "null pointer")


def test_python_arguments_refused_before_any_launch():
    P = 6
    acc, den, g, r = torch.zeros(P, 1), torch.zeros(P, 1), torch.zeros(P, 3), torch.ones(P, dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        ts.densification_stats(acc, den, g, r)
    with pytest.raises(ValueError, match=r"\(P, 3\)"):
        ts.densification_stats(acc, den, torch.zeros(P, 2), r)
    with pytest.raises(ValueError, match="accum"):
        ts.densification_stats(torch.zeros(P + 1, 1), den, g, r)
    with pytest.raises(ValueError, match="denom"):
        ts.densification_stats(acc, den.double(), g, r)
    with pytest.raises(ValueError, match="radii"):
        ts.densification_stats(acc, den, g, r.float())
    with pytest.raises(ValueError, match="max_radii2D"):
        ts.densification_stats(acc, den, g, r, torch.zeros(P + 2))
    case = ref.densify_case(P, 0, 0)
    args = (case["params"], None, case["accum"], case["denom"], case["max_radii2D"])
    with pytest.raises(ValueError, match="GPU"):
        ts.densify_and_prune(*args, 2e-4, 0.005, 5.0, 0.01, 20)
    with pytest.raises(ValueError, match="max_grad must be > 0"):
        ts.densify_and_prune(*args, 0.0, 0.005, 5.0, 0.01, 20)
    with pytest.raises(ValueError, match="lacks 'opacity'"):
        ts.densify_and_prune({k: v for k, v in case["params"].items() if k != "opacity"}, None, *args[2:], 2e-4, 0.005, 5.0, 0.01, 20)


@pytest.mark.parametrize("eps", [1e-15, 1e-8])
def test_adam_restatement_is_torch_adam_in_float64(eps):
    gen = torch.Generator().manual_seed(3)
    p0 = torch.randn(257, 3, generator=gen, dtype=torch.float64)
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([q], lr=1.6e-4, betas=(0.9, 0.999), eps=eps)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    worst = 0.0
    for step in range(1, 6):
        g = torch.randn(257, 3, generator=gen, dtype=torch.float64) * 10.0 ** float(step - 3)
        q.grad = g.clone()
        opt.step()
        p, m, v, _ = ref.adam_restated(p, g, m, v, step, 1.6e-4, 0.9, 0.999, eps)
        st = opt.state[q]
        worst = max(worst, (q.detach() - p).abs().max().item(), (st["exp_avg"] - m).abs().max().item(), (st["exp_avg_sq"] - v).abs().max().item())
        # rounding of float64 at unit scale: a few 2^-53 of |p| ~ 4, nothing that grows with the step
        assert (q.detach() - p).abs().max().item() <= 8 * 2.0 ** -53 * 4.0
        assert (st["exp_avg"] - m).abs().max().item() <= 4 * 2.0 ** -53 * max(1.0, g.abs().max().item())
        assert (st["exp_avg_sq"] - v).abs().max().item() <= 4 * 2.0 ** -53 * max(1.0, g.abs().max().item() ** 2)
    print(f"adam restatement vs torch.optim.Adam, float64, eps {eps:g}: worst difference {worst:.2e}")


def _six_groups(P, seed, dtype=torch.float32, device="cpu"):
    gen = torch.Generator().manual_seed(seed)
    shapes = {"xyz": (P, 3), "f_dc": (P, 1, 3), "f_rest": (P, 15, 3), "opacity": (P, 1), "scaling": (P, 3), "rotation": (P, 4)}
    lrs = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 2.5e-3 / 20, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3}
    params = {k: torch.nn.Parameter(torch.randn(s, generator=gen).to(dtype).to(device)) for k, s in shapes.items()}
    groups = [{"params": [params[k]], "lr": lrs[k], "name": k} for k in shapes]
    grads = [{k: torch.randn(s, generator=gen).to(dtype).to(device) for k, s in shapes.items()} for _ in range(4)]
    return params, groups, grads


def test_fused_adam_on_cpu_tensors_is_torch_adam_bit_for_bit():
    pa, ga, grads = _six_groups(33, 1)
    pb, gb, _ = _six_groups(33, 1)
    a, b = torch.optim.Adam(ga, lr=0.0, eps=1e-15), ts.FusedAdam(gb, lr=0.0, eps=1e-15)
    assert isinstance(b, torch.optim.Adam) and [g["name"] for g in b.param_groups] == [g["name"] for g in a.param_groups]
    for it, gr in enumerate(grads):
        for k in pa:
            skip = it == 1 and k == "rotation"            # a parameter without a gradient is skipped
            pa[k].grad, pb[k].grad = (None, None) if skip else (gr[k].clone(), gr[k].clone())
        a.step()
        b.step()
        for k in pa:
            assert torch.equal(pa[k], pb[k]), (it, k)
            sa, sb = a.state[pa[k]], b.state[pb[k]]
            assert set(sa) == set(sb) == {"step", "exp_avg", "exp_avg_sq"}
            for key in sa:
                assert type(sa[key]) is type(sb[key]) and sa[key].dtype == sb[key].dtype and sa[key].device == sb[key].device
                assert torch.equal(sa[key], sb[key]), (it, k, key)
    assert b.state[pb["rotation"]]["step"].item() == 3 and b.state[pb["xyz"]]["step"].item() == 4


def test_state_dict_moves_between_fused_adam_and_torch_adam():
    pa, ga, grads = _six_groups(9, 2)
    pb, gb, _ = _six_groups(9, 2)
    pc, gc, _ = _six_groups(9, 2)
    a, b, c = torch.optim.Adam(ga, lr=0.0, eps=1e-15), ts.FusedAdam(gb, lr=0.0, eps=1e-15), torch.optim.Adam(gc, lr=0.0, eps=1e-15)
    for k in pa:
        pa[k].grad = grads[0][k].clone()
    a.step()
    b.load_state_dict(copy.deepcopy(a.state_dict()))      # torch -> fused (a copy: load_state_dict keeps the tensors it is given)
    c.load_state_dict(copy.deepcopy(b.state_dict()))      # fused -> torch
    da, db = a.state_dict(), b.state_dict()
    assert da["param_groups"] == db["param_groups"] and list(da["state"]) == list(db["state"])
    for k in pa:
        with torch.no_grad():
            pb[k].copy_(pa[k])
            pc[k].copy_(pa[k])
        for p in (pa, pb, pc):
            p[k].grad = grads[1][k].clone()
    a.step(), b.step(), c.step()
    for k in pa:
        assert torch.equal(pa[k], pb[k]) and torch.equal(pa[k], pc[k]), k
        assert b.state[pb[k]]["step"].item() == 2 == c.state[pc[k]]["step"].item()
    f = ts.FusedAdam.from_optimizer(a)
    assert [g["name"] for g in f.param_groups] == list(pa) and f.param_groups[0]["params"][0] is pa["xyz"]
    assert f.state[pa["xyz"]] is a.state[pa["xyz"]] and f.defaults["eps"] == 1e-15 and f.param_groups[3]["lr"] == 0.05


# the hand-made table: one row per line; thresholds max_grad 0.25, min_opacity 0.5, percent_dense extent = 1.0, 0.1 extent = 1.0
#          accum denom  max exp(s)  opacity logit   what becomes of it
TABLE = [(0.10, 1.0, 0.5, 2.0),     # 0  kept
         (0.60, 2.0, 0.5, 2.0),     # 1  cloned (g = 0.3)
         (0.90, 3.0, 1.2, 2.0),     # 2  split, children 0.75 stay
         (0.10, 1.0, 0.5, -2.0),    # 3  pruned by opacity
         (0.10, 1.0, 2.0, 2.0),     # 4  pruned by size
         (0.80, 2.0, 2.0, 2.0),     # 5  split, children 1.25 pruned by size
         (0.00, 0.0, 0.5, 2.0),     # 6  denom == 0, accum 0: NaN -> 0, kept
         (0.30, 0.0, 0.5, 2.0),     # 7  denom == 0, accum > 0: inf, cloned
         (0.50, 2.0, 1.0, 0.0),     # 8  every quantity ON its threshold: g >= 0.25 selected, 1.0 > 1.0 false (a clone, kept), 0.5 < 0.5 false
         (0.60, 2.0, 0.5, -2.0),    # 9  cloned, original and clone pruned by opacity
         (0.90, 3.0, 1.2, -2.0),    # 10 split, both children pruned by opacity
         (0.05, 1.0, 0.25, 2.0)]    # 11 kept


def _table_case(dtype):
    rows = np.array(TABLE, np.float64)
    P = len(TABLE)
    rng = np.random.default_rng(5)
    s = np.log(rows[:, 2])[:, None] + np.log(rng.uniform(0.3, 0.9, (P, 3)))
    s[:, 1] = np.log(rows[:, 2])
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
    params = {"xyz": t(rng.normal(0, 1, (P, 3))), "f_dc": t(rng.normal(0, 1, (P, 1, 3))), "f_rest": t(rng.normal(0, 1, (P, 3, 3))),
              "opacity": t(rows[:, 3:4]), "scaling": t(s), "rotation": t(rng.normal(0, 1, (P, 4)))}
    moments = {k: (t(rng.normal(0, 1, tuple(p.shape))), t(rng.uniform(0.5, 1, tuple(p.shape)))) for k, p in params.items()}
    samples = t(rng.normal(0, 1, (6, 3)))
    out = ref.densify_restated(params, moments, t(rows[:, 0:1]), t(rows[:, 1:2]), 0.25, 0.5, 10.0, 0.1, 20, samples, dtype)
    return params, moments, samples, out


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_densify_restatement_on_the_hand_made_table(dtype):
    params, moments, samples, out = _table_case(dtype)
    assert out["counts"] == {"clones": 4, "splits": 3, "kept_originals": 6, "kept_clones": 3, "kept_children": 1}
    # originals not split in order, clones in order, first children, second children
    assert out["origin"].tolist() == [0, 1, 6, 7, 8, 11, 1, 7, 8, 2, 2]
    assert out["kind"].tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 1, 2, 3]
    T, M = out["params"], out["moments"]
    src = out["origin"]
    for k in params:
        copied = slice(0, 9) if k in ("xyz", "scaling") else slice(0, 11)
        assert torch.equal(T[k][copied], params[k][src][copied].to(dtype)), k
        assert torch.equal(M[k][0][:6], moments[k][0][src[:6]].to(dtype)) and torch.equal(M[k][1][:6], moments[k][1][src[:6]].to(dtype))
        assert not M[k][0][6:].any() and not M[k][1][6:].any() and M[k][0].shape == T[k].shape
    # the children of row 2 use samples 0 (first child) and 3 (second child) of the 2 x 3 draws, in the order rows 2, 5, 10
    R = ref.build_rotation(params["rotation"][2:3].to(dtype))[0]
    for child, smp in ((9, 0), (10, 3)):
        want = R @ samples[smp].to(dtype) + params["xyz"][2].to(dtype)
        assert torch.allclose(T["xyz"][child], want, rtol=1e-5, atol=1e-6)
        assert torch.allclose(T["scaling"][child], torch.log(torch.exp(params["scaling"][2].to(dtype)) / 1.6), rtol=1e-5, atol=1e-6)
    # without a screen size the two size prunes do not apply: rows 4 survives and the children of row 5 too
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
    rows = np.array(TABLE, np.float64)
    out2 = ref.densify_restated(params, moments, t(rows[:, 0:1]), t(rows[:, 1:2]), 0.25, 0.5, 10.0, 0.1, None, samples, dtype)
    assert out2["origin"].tolist() == [0, 1, 4, 6, 7, 8, 11, 1, 7, 8, 2, 5, 2, 5]
    assert torch.equal(ref.split_mask(params, t(rows[:, 0:1]), t(rows[:, 1:2]), 0.25, 10.0, 0.1), torch.tensor([i in (2, 5, 10) for i in range(12)]))


def test_densify_case_has_every_class_away_from_its_threshold():
    for P in (12, 257):
        case = ref.densify_case(P, 0, P)
        for name in ref.CLASS_NAMES:
            share = case["classes"].count(name) / P
            assert 0.05 <= share <= 0.30, (P, name, share)
        assert ref.decision_margins(case) > 16
    case = ref.densify_case(12, 0, 1, max_grad=0.25, min_opacity=0.5, extent=10.0, percent_dense=0.1, designated=2)
    assert case["params"]["xyz"].shape[0] == 14 and ref.decision_margins(case) > 16
    assert 0.1 * 10.0 == 1.0 and torch.sigmoid(torch.zeros(1)).item() == 0.5 and torch.exp(torch.zeros(1)).item() == 1.0


class _StandIn:
    """What install_dropin patches of scene.gaussian_model.GaussianModel."""
    SOURCE = ("class GaussianModel:\n"
              "    def training_setup(self, training_args):\n        self.optimizer = 'reference optimizer'\n"
              "    def add_densification_stats(self, viewspace_point_tensor, update_filter):\n        return 'reference stats'\n"
              "    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size):\n        return 'reference densify'\n")


def test_install_dropin_fuse_training_step_patches_a_stand_in(tmp_path, monkeypatch):
    pkg = tmp_path / "scene"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    (pkg / "gaussian_model.py").write_text(_StandIn.SOURCE)
    monkeypatch.syspath_prepend(str(tmp_path))
    for k in ("scene", "scene.gaussian_model"):
        monkeypatch.delitem(sys.modules, k, raising=False)
    try:
        seganygaussians_amd.install_dropin(fuse_training_step=True)
        seganygaussians_amd.install_dropin(fuse_training_step=True)            # one finder, however often it is asked for
        assert sum(isinstance(f, seganygaussians_amd._PatchOnImport) and f.module_name == "scene.gaussian_model" for f in sys.meta_path) == 1
        cls = importlib.import_module("scene.gaussian_model").GaussianModel
        assert not any(isinstance(f, seganygaussians_amd._PatchOnImport) and f.module_name == "scene.gaussian_model" for f in sys.meta_path)
        for _ in range(2):                                                     # already imported: patched at once, idempotently
            seganygaussians_amd.install_dropin(fuse_training_step=True)
            assert cls.training_setup is ts.fused_training_setup
            assert cls.add_densification_stats is ts.fused_add_densification_stats
            assert cls.densify_and_prune is ts.fused_densify_and_prune
            m = cls()
            assert cls._reference_add_densification_stats(m, None, None) == "reference stats"
            assert cls._reference_densify_and_prune(m, 1, 1, 1, 1) == "reference densify"
            cls._reference_training_setup(m, None)
            assert m.optimizer == "reference optimizer"
        # training_setup runs the reference's own, then swaps its Adam for a FusedAdam over the same groups
        q = torch.nn.Parameter(torch.zeros(3, 3))
        cls._reference_training_setup = lambda self, args: setattr(self, "optimizer", torch.optim.Adam([{"params": [q], "lr": 0.5, "name": "xyz"}], lr=0.0, eps=1e-15))
        m = cls()
        m.training_setup(None)
        assert isinstance(m.optimizer, ts.FusedAdam) and m.optimizer.param_groups[0]["name"] == "xyz" and m.optimizer.param_groups[0]["params"][0] is q
        assert m.optimizer.param_groups[0]["lr"] == 0.5 and m.optimizer.defaults["eps"] == 1e-15
    finally:
        sys.meta_path[:] = [f for f in sys.meta_path if not (isinstance(f, seganygaussians_amd._PatchOnImport) and f.module_name == "scene.gaussian_model")]
        for k in ("scene", "scene.gaussian_model"):
            sys.modules.pop(k, None)
