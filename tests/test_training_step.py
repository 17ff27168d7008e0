"""GPU checks of the fused training step (seganygaussians_amd/training_step.py, csrc/train_step.h).

The rule is tests/edge_ref.py: ratios (FACTOR 4, FLOOR 2^-22), one group per row: the truth is the float64 restatement on the CPU
(tests/training_step_ref.py), the yardstick the float32 reference expression on the CPU on the same input (torch.optim.Adam, the
reference's five statistics lines, the densify restatement in float32); every |product - truth| / bound must be <= 1.  Magnitudes of
the floor: parameter |p| + |update|, first moment |m| + |g|, second moment |v| + g^2, child position |xyz| + sum |R||sample|, child
log-scale |s| + log 1.6.  Each test prints its worst ratio (-s)."""
import math

import numpy as np
import pytest
import torch

from seganygaussians_amd import training_step as ts
from tests import training_step_ref as ref
from tests.edge_ref import ratios

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROWS = (1, 3, 4, 5, 63, 64, 65, 1023, 1025, 4099)
B1, B2 = 0.9, 0.999


def _rows(a):
    a = np.asarray(a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else a, np.float64)
    if a.size == 0:
        return np.zeros((0, 1))
    return a.reshape(a.shape[0], -1) if a.ndim else a.reshape(1, 1)


def _rule(product, f64, f32, mag):
    """error / bound per row; an empty tensor gives [0]."""
    m = _rows(mag)
    return ratios(_rows(product), _rows(f64), _rows(f32), m.max(axis=1) if m.size else m.reshape(-1), rows=True)


def _on_device(t, offset=0):
    """A contiguous device copy of t whose storage begins `offset` floats into an allocation."""
    base = torch.empty(t.numel() + offset, device=DEV, dtype=torch.float32)
    out = base[offset:].view(t.shape)
    out.copy_(t)
    return out


def fused_step(tensors, step, eps, offsets=(0, 0, 0, 0), cls=None, steps=1, grads_per_step=None):
    """tensors: list of (p, g, m, v, lr) float32 CPU tensors (g None: no gradient; m None: no state yet).  One FusedAdam over one
    group per tensor, the state set to (step - 1, m, v); `steps` steps.  Returns the optimizer and [(p, m, v)] on the CPU."""
    params = [torch.nn.Parameter(_on_device(p, offsets[0])) for p, *_ in tensors]
    opt = (cls or ts.FusedAdam)([{"params": [q], "lr": lr, "name": str(k)} for k, (q, (*_, lr)) in enumerate(zip(params, tensors))], lr=0.0, betas=(B1, B2), eps=eps)
    for q, (p, g, m, v, lr) in zip(params, tensors):
        if m is not None:
            opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": _on_device(m, offsets[2]), "exp_avg_sq": _on_device(v, offsets[3])}
    for s in range(steps):
        for k, (q, (p, g, m, v, lr)) in enumerate(zip(params, tensors)):
            gk = g if grads_per_step is None else grads_per_step[s][k]
            q.grad = None if gk is None else _on_device(gk, offsets[1])
        opt.step()
    torch.cuda.synchronize()
    out = []
    for q in params:
        st = opt.state.get(q, {})
        out.append((q.detach().cpu(), st["exp_avg"].cpu() if st else None, st["exp_avg_sq"].cpu() if st else None))
    return opt, out


def check_adam(name, tensors, got, step, eps):
    worst = 0.0
    for k, ((p, g, m, v, lr), (gp, gm, gv)) in enumerate(zip(tensors, got)):
        if m is None:
            m, v = torch.zeros_like(p), torch.zeros_like(p)
        t_p, t_m, t_v, upd = ref.adam_restated(p.double(), g.double(), m.double(), v.double(), step, lr, B1, B2, eps)
        y_p, y_m, y_v = ref.torch_adam_step(p, g, m, v, step, lr, B1, B2, eps, torch.float32)
        assert gp.shape == p.shape and gm.shape == p.shape and gv.shape == p.shape
        for what, prod, truth, yard, mag in (("p", gp, t_p, y_p, p.double().abs() + upd), ("m", gm, t_m, y_m, m.double().abs() + g.double().abs()),
                                             ("v", gv, t_v, y_v, v.double().abs() + g.double() ** 2)):
            r = _rule(prod, truth, yard, mag)
            assert (r <= 1.0).all(), (name, k, what, int(np.argmax(~(r <= 1.0))), float(np.nanmax(r)))
            worst = max(worst, float(r.max()))
    print(f"{name}: worst error / bound {worst:.3f}")
    return worst


def _tensor(P, w, seed, gscale=1.0, with_state=True):
    gen = torch.Generator().manual_seed(seed)
    shape = (P, w)
    p = torch.randn(shape, generator=gen)
    g = torch.randn(shape, generator=gen) * gscale
    m = torch.randn(shape, generator=gen) * 0.1 * gscale if with_state else None
    v = torch.rand(shape, generator=gen) * gscale * gscale if with_state else None
    return p, g, m, v


@pytest.mark.parametrize("w", [1, 3, 4, 45])
def test_adam_single_tensor_every_row_count(w):
    worst = 0.0
    for P in ROWS:
        t = [_tensor(P, w, 100 * w + P) + (1.6e-4,)]
        _, got = fused_step(t, 7, 1e-15)
        worst = max(worst, check_adam(f"adam P={P} w={w}", t, got, 7, 1e-15))
    print(f"adam single tensor w={w}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("w", [1, 3, 45])
def test_adam_storage_offset_equals_the_aligned_run(w):
    for P in (1, 5, 65, 1025):
        t = [_tensor(P, w, 7 * w + P) + (2.5e-3,)]
        _, aligned = fused_step(t, 3, 1e-15)
        _, shifted = fused_step(t, 3, 1e-15, offsets=(1, 1, 1, 1))       # float4 body behind a head of three floats
        _, mixed = fused_step(t, 3, 1e-15, offsets=(1, 0, 2, 3))         # the pointers disagree modulo 16: float by float
        for a, b, c in zip(aligned[0], shifted[0], mixed[0]):
            assert torch.equal(a, b) and torch.equal(a, c), (P, w)
        check_adam(f"adam offset P={P} w={w}", t, shifted, 3, 1e-15)


def _six(P, seed, with_state):
    shapes = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
    lrs = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 2.5e-3 / 20, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3}
    out = []
    for k, (name, s) in enumerate(shapes.items()):
        p, g, m, v = _tensor(P, int(np.prod(s)), seed + k, with_state=with_state)
        rs = lambda t: None if t is None else t.reshape((P,) + s)
        out.append((rs(p), rs(g), rs(m), rs(v), lrs[name]))
    return out


def test_adam_six_groups_in_one_launch(monkeypatch):
    from seganygaussians_amd import _lib
    L = _lib.load()
    calls, real = [], L.mi_train_adam_step
    monkeypatch.setattr(L, "mi_train_adam_step", lambda n, *a: (calls.append(n), real(n, *a))[1])     # counts the launches
    for P, state in ((1025, True), (257, False)):       # with a state, and the lazily created one of a first step
        t = _six(P, P, state)
        step = 5 if state else 1
        opt, got = fused_step(t, step, 1e-15)
        check_adam(f"adam six groups P={P}", t, got, step, 1e-15)
        st = opt.state[opt.param_groups[0]["params"][0]]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and st["step"].device.type == "cpu" and st["step"].item() == step
    assert calls == [6, 6], calls
    # seventeen tensors: two launches (16 + 1); the third has no gradient, the fifth no rows
    t = [_tensor(5 + 2 * k, 3, 900 + k) + (1e-3,) for k in range(17)]
    t[2] = (t[2][0], None) + t[2][2:]
    t[4] = tuple(torch.zeros(0, 3) for _ in range(4)) + (1e-3,)
    calls.clear()
    opt, got = fused_step(t, 2, 1e-15)
    assert calls == [16], calls        # 16 tensors carry a gradient: one launch; all 17 below
    assert torch.equal(got[2][0], t[2][0]) and torch.equal(got[2][1], t[2][2]) and torch.equal(got[2][2], t[2][3])      # untouched, bit for bit
    assert opt.state[opt.param_groups[2]["params"][0]]["step"].item() == 1
    assert got[4][0].shape == (0, 3)
    check_adam("adam 17 tensors, one without gradient", [x for k, x in enumerate(t) if k != 2], [x for k, x in enumerate(got) if k != 2], 2, 1e-15)
    t[2] = _tensor(9, 3, 77) + (1e-3,)
    calls.clear()
    _, got = fused_step(t, 2, 1e-15)
    assert calls == [16, 1], calls
    check_adam("adam 17 tensors, two launches", t, got, 2, 1e-15)


@pytest.mark.parametrize("eps", [1e-15, 1e-8])
@pytest.mark.parametrize("step", [1, 1000])
def test_adam_gradient_magnitudes_and_hyper_parameters(eps, step):
    P, w = 16 * 16, 3
    p, g, m, v = _tensor(P, w, 11)
    mags = 10.0 ** torch.linspace(-12, 3, 16).repeat_interleave(16)            # 1e-12 .. 1e3 in one table
    g = torch.sign(g) * mags[:, None] * (0.5 + torch.rand(P, w, generator=torch.Generator().manual_seed(1)))
    m, v = m * mags[:, None], v * mags[:, None] ** 2
    if step == 1:
        m, v = torch.zeros_like(m), torch.zeros_like(v)
    t = [(p, g, m, v, 1.6e-4)]
    _, got = fused_step(t, step, eps)
    check_adam(f"adam magnitudes eps={eps:g} step={step}", t, got, step, eps)
    # exact zeros with zero moments: nothing moves, bit for bit
    z = torch.zeros(65, w)
    _, got = fused_step([(p[:65], z, z, z, 0.05)], step, eps)
    assert torch.equal(got[0][0], p[:65]) and not got[0][1].any() and not got[0][2].any()
    # g = 1e-25: g * g underflows in binary32, in the yardstick too
    tiny = torch.full((65, w), 1e-25) * torch.sign(torch.randn(65, w, generator=torch.Generator().manual_seed(2)))
    t = [(p[:65], tiny, z, z, 0.05)]
    _, got = fused_step(t, step, eps)
    check_adam(f"adam g=1e-25 eps={eps:g} step={step}", t, got, step, eps)


def test_adam_multi_step():
    P, w, lr, eps = 1025, 3, 5e-3, 1e-15
    gen = torch.Generator().manual_seed(21)
    grads = [torch.randn(P, w, generator=gen) * 10.0 ** float(s % 3 - 1) for s in range(20)]
    p0 = torch.randn(P, w, generator=gen)
    # five steps, each from the identical state: that of torch.optim.Adam's float32 run on the CPU
    p, m, v = p0, torch.zeros(P, w), torch.zeros(P, w)
    for s in range(1, 6):
        t = [(p, grads[s - 1], m, v, lr)]
        _, got = fused_step(t, s, eps)
        check_adam(f"adam step {s} of 5", t, got, s, eps)
        p, m, v = ref.torch_adam_step(p, grads[s - 1], m, v, s, lr, B1, B2, eps, torch.float32)
    # one run of 20 steps, checked at the end.  Magnitudes: what was summed into each over the run
    _, got = fused_step([(p0, None, None, None, lr)], 1, eps, steps=20, grads_per_step=[[g] for g in grads])
    tp, tm, tv = p0.double(), torch.zeros(P, w, dtype=torch.float64), torch.zeros(P, w, dtype=torch.float64)
    yp, ym, yv = p0, torch.zeros(P, w), torch.zeros(P, w)
    mag_p, mag_m, mag_v = p0.double().abs(), torch.zeros(P, w, dtype=torch.float64), torch.zeros(P, w, dtype=torch.float64)
    for s in range(1, 21):
        tp, tm, tv, upd = ref.adam_restated(tp, grads[s - 1].double(), tm, tv, s, lr, B1, B2, eps)
        yp, ym, yv = ref.torch_adam_step(yp, grads[s - 1], ym, yv, s, lr, B1, B2, eps, torch.float32)
        mag_p, mag_m, mag_v = mag_p + upd, mag_m + grads[s - 1].double().abs(), mag_v + grads[s - 1].double() ** 2
    worst = 0.0
    for what, prod, truth, yard, mag in (("p", got[0][0], tp, yp, mag_p), ("m", got[0][1], tm, ym, mag_m), ("v", got[0][2], tv, yv, mag_v)):
        r = _rule(prod, truth, yard, mag)
        assert (r <= 1.0).all(), (what, float(np.nanmax(r)))
        worst = max(worst, float(r.max()))
    print(f"adam 20 steps: worst error / bound {worst:.3f}")


def test_adam_reruns_are_bit_identical():
    t = _six(4099, 5, True)
    _, a = fused_step(t, 9, 1e-15)
    _, b = fused_step(t, 9, 1e-15)
    for x, y in zip(a, b):
        assert all(torch.equal(i, j) for i, j in zip(x, y))


# ---- densification statistics ---------------------------------------------------------------------------------------------------

def _stats_expression(accum, denom, max_radii, grad, radii, dtype):
    """train_scene.py:126 and scene/gaussian_model.py:582-584 on the CPU in `dtype`."""
    accum, denom, grad = accum.to(dtype).clone(), denom.to(dtype).clone(), grad.to(dtype)
    vis = radii > 0
    if max_radii is not None:
        max_radii = max_radii.to(dtype).clone()
        max_radii[vis] = torch.max(max_radii[vis], radii[vis])
    accum[vis] += torch.norm(grad[vis, :2], dim=-1, keepdim=True)
    denom[vis] += 1
    return accum, denom, max_radii


@pytest.mark.parametrize("visible", ["some", "none", "all"])
@pytest.mark.parametrize("with_max", [True, False])
def test_densification_stats(visible, with_max):
    worst = 0.0
    for P in ROWS:
        gen = torch.Generator().manual_seed(P)
        radii = torch.randint(-2, 40, (P,), generator=gen, dtype=torch.int32)
        radii = {"some": torch.where(torch.rand(P, generator=gen) < 0.5, radii, torch.zeros_like(radii)), "none": -radii.abs(), "all": radii.abs() + 1}[visible]
        grad = torch.randn(P, 3, generator=gen) * 10.0 ** torch.randint(-8, 1, (P, 1), generator=gen).float()
        accum, denom = torch.rand(P, 1, generator=gen) * 1e-3, torch.randint(0, 5, (P, 1), generator=gen).float()
        max_r = torch.randint(0, 40, (P,), generator=gen).float() if with_max else None
        d = [t.to(DEV) for t in (accum, denom, grad, radii)]
        dm = max_r.to(DEV) if with_max else None
        ts.densification_stats(d[0], d[1], d[2], d[3], dm)
        t64 = _stats_expression(accum, denom, max_r, grad, radii, torch.float64)
        y32 = _stats_expression(accum, denom, max_r, grad, radii, torch.float32)
        assert torch.equal(d[1].cpu(), y32[1]) and (not with_max or torch.equal(dm.cpu(), y32[2]))               # exact
        hidden = radii <= 0
        assert torch.equal(d[0].cpu()[hidden], accum[hidden]) and torch.equal(d[1].cpu()[hidden], denom[hidden])   # untouched, bit for bit
        assert not with_max or torch.equal(dm.cpu()[hidden], max_r[hidden])
        r = _rule(d[0], t64[0], y32[0], accum.double().abs() + grad[:, :2].double().abs().sum(dim=1, keepdim=True))
        assert (r <= 1.0).all(), (P, float(np.nanmax(r)))
        worst = max(worst, float(r.max()))
        # a bool mask (what add_densification_stats receives) selects the same rows
        d2 = [t.to(DEV) for t in (accum, denom)]
        ts.densification_stats(d2[0], d2[1], d[2], (radii > 0).to(DEV))
        assert torch.equal(d2[0], d[0]) and torch.equal(d2[1], d[1])
    print(f"densification stats visible={visible} max_radii2D={with_max}: worst error / bound {worst:.3f}")


# ---- densify and prune ----------------------------------------------------------------------------------------------------------

LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 2.5e-3 / 20, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3}


def run_densify(name, case, max_screen_size, seed=0, with_state=True):
    """The product on the device against the restatement in float64 (truth) and float32 (yardstick) with the very samples the
    product draws under `seed`; then one further FusedAdam step on the new tensors.  Returns the truth."""
    assert ref.decision_margins(case) > 16, "the input has a decision quantity within 16 ulp of its threshold"
    a = case["args"]
    params = {k: torch.nn.Parameter(t.to(DEV)) for k, t in case["params"].items()}
    opt = ts.FusedAdam([{"params": [params[k]], "lr": LRS[k], "name": k} for k in params], lr=0.0, eps=1e-15)
    if with_state:
        for k, q in params.items():
            opt.state[q] = {"step": torch.tensor(3.0), "exp_avg": case["moments"][k][0].to(DEV), "exp_avg_sq": case["moments"][k][1].to(DEV)}
    moments = case["moments"] if with_state else {}
    mask = ref.split_mask(case["params"], case["accum"], case["denom"], a["max_grad"], a["extent"], a["percent_dense"])
    torch.manual_seed(seed)
    stds = torch.exp(params["scaling"].detach()[mask.to(DEV)]).repeat(2, 1)
    samples = torch.normal(mean=torch.zeros((stds.size(0), 3), device=DEV), std=stds).cpu()
    torch.manual_seed(seed)
    accum, denom, max_r = (case[k].to(DEV) for k in ("accum", "denom", "max_radii2D"))
    new, n_accum, n_denom, n_max = ts.densify_and_prune(params, opt, accum, denom, max_r, a["max_grad"], a["min_opacity"], a["extent"],
                                                        a["percent_dense"], max_screen_size)
    torch.cuda.synchronize()
    common = (case["accum"], case["denom"], a["max_grad"], a["min_opacity"], a["extent"], a["percent_dense"], max_screen_size, samples)
    truth = ref.densify_restated(case["params"], moments, *common, torch.float64)
    yard = ref.densify_restated(case["params"], moments, *common, torch.float32)
    src, kind = truth["origin"], truth["kind"]
    assert torch.equal(src, yard["origin"]) and torch.equal(kind, yard["kind"])
    n = src.numel()
    # the row count, the zeroed statistics
    assert n_accum.shape == (n, 1) and n_denom.shape == (n, 1) and n_max.shape == (n,)
    assert n_accum.device == DEV and not n_accum.any() and not n_denom.any() and not n_max.any()
    child = kind >= 2
    worst = 0.0
    for k, t in case["params"].items():
        got = new[k].detach().cpu()
        assert got.shape == (n,) + tuple(t.shape[1:]) and new[k].requires_grad and new[k].is_leaf, k
        rows = ~child if k in ("xyz", "scaling") else torch.ones(n, dtype=torch.bool)
        assert torch.equal(got[rows], t[src][rows]), (name, k)                    # every copied column, bit for bit
        if k in ("xyz", "scaling") and child.any():
            r = _rule(got[child], truth["params"][k][child], yard["params"][k][child], truth["mag_xyz" if k == "xyz" else "mag_scaling"][child, None])
            assert (r <= 1.0).all(), (name, k, float(np.nanmax(r)))
            worst = max(worst, float(r.max()))
        # the optimizer: rebound to the new tensor; survivors keep their moments bit for bit, new rows start at zero
        group = next(g for g in opt.param_groups if g["name"] == k)
        assert group["params"][0] is new[k] and len(group["params"]) == 1 and group["lr"] == LRS[k]
        assert params[k] not in opt.state
        if with_state:
            st = opt.state[new[k]]
            assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and st["step"].item() == 3
            for key, orig in zip(("exp_avg", "exp_avg_sq"), case["moments"][k]):
                want = torch.where((kind == 0).reshape((n,) + (1,) * (t.dim() - 1)), orig[src], torch.zeros(()))
                assert torch.equal(st[key].cpu(), want), (name, k, key)
        else:
            assert new[k] not in opt.state
    assert len(opt.state) == (len(params) if with_state else 0)
    # one further step on the new tensors
    gen = torch.Generator().manual_seed(seed + 1)
    tensors = []
    for k in params:
        g = torch.randn(new[k].shape, generator=gen)
        new[k].grad = g.to(DEV)
        st = opt.state.get(new[k])
        tensors.append((new[k].detach().cpu().clone(), g, st["exp_avg"].cpu().clone() if st else None, st["exp_avg_sq"].cpu().clone() if st else None, LRS[k]))
    opt.step()
    torch.cuda.synchronize()
    got = [(new[k].detach().cpu(), opt.state[new[k]]["exp_avg"].cpu(), opt.state[new[k]]["exp_avg_sq"].cpu()) for k in params]
    step = 4 if with_state else 1
    assert all(opt.state[new[k]]["step"].item() == step for k in params)
    worst = max(worst, check_adam(f"{name}: the step after it", tensors, got, step, 1e-15))
    print(f"{name}: rows {case['params']['xyz'].shape[0]} -> {n} {truth['counts']}; worst error / bound {worst:.3f}")
    return truth


@pytest.mark.parametrize("sh_degree", [0, 3])
@pytest.mark.parametrize("P", [1, 12, 255, 256, 257, 4099])
def test_densify_and_prune(P, sh_degree):
    case = ref.densify_case(P, sh_degree, 10 * P + sh_degree)
    if P >= 12:
        for name in ref.CLASS_NAMES:
            assert 0.05 <= case["classes"].count(name) / P <= 0.30, name
    truth = run_densify(f"densify P={P} sh={sh_degree}", case, 20)
    c = truth["counts"]
    if P >= 12:
        assert c["clones"] > c["kept_clones"] > 0 and c["splits"] > c["kept_children"] > 0 and 0 < c["kept_originals"] < P - c["splits"]


def test_densify_rows_on_their_thresholds():
    """Designated rows with exactly representable activations: s = 0 (exp = 1.0), o = 0 (sigmoid = 0.5), accum / denom = 0.25, against
    thresholds of exactly 1.0 (percent_dense extent and 0.1 extent), 0.5 and 0.25.  `>=` selects them, `>` 1.0 is false twice (a
    clone, not a split; not too big) and `<` 0.5 is false: each is cloned, and the row and its clone stay."""
    case = ref.densify_case(255, 3, 4, max_grad=0.25, min_opacity=0.5, extent=10.0, percent_dense=0.1, designated=4)
    assert 0.1 * 10.0 == 1.0
    truth = run_densify("densify designated rows", case, 20)
    for row in range(255, 259):
        assert ((truth["origin"] == row) & (truth["kind"] == 0)).sum() == 1 and ((truth["origin"] == row) & (truth["kind"] == 1)).sum() == 1


@pytest.mark.parametrize("edge", ["nothing_selected", "everything_pruned", "all_split", "no_screen_size", "denom_zero", "no_state"])
def test_densify_edge_cases(edge):
    P = 257
    pick = {"nothing_selected": ("kept", "low_opacity", "too_big", "denom0_nan"), "everything_pruned": ("low_opacity", "cloned_low_opacity", "split_low_opacity"),
            "all_split": ("split",), "denom_zero": ("denom0_nan", "denom0_inf")}.get(edge)
    classes = None if pick is None else [pick[i % len(pick)] for i in range(P)]
    case = ref.densify_case(P, 3, 31, classes=classes)
    truth = run_densify(f"densify {edge}", case, None if edge == "no_screen_size" else 20, with_state=edge != "no_state")
    c, n = truth["counts"], truth["origin"].numel()
    if edge == "nothing_selected":
        assert c["clones"] == 0 and c["splits"] == 0 and 0 < n < P
    elif edge == "everything_pruned":
        assert n == 0 and c["clones"] > 0 and c["splits"] > 0
    elif edge == "all_split":
        assert c["splits"] == P and n == 2 * P and c["kept_originals"] == 0
    elif edge == "no_screen_size":
        with_size = ref.densify_restated(case["params"], {}, case["accum"], case["denom"], *list(case["args"].values())[:4], 20, torch.zeros(2 * c["splits"], 3))
        assert n > with_size["origin"].numel()
    elif edge == "denom_zero":
        assert c["clones"] == case["classes"].count("denom0_inf") > 0        # accum / 0 = inf is selected, 0 / 0 = NaN -> 0 is not
        assert c["splits"] == 0 and n == P + c["clones"]


def test_densify_reruns_are_bit_identical():
    case = ref.densify_case(4099, 3, 8)
    outs = []
    for _ in range(2):
        params = {k: t.to(DEV) for k, t in case["params"].items()}
        torch.manual_seed(5)
        a = case["args"]
        new, *_ = ts.densify_and_prune(params, None, case["accum"].to(DEV), case["denom"].to(DEV), case["max_radii2D"].to(DEV), a["max_grad"],
                                       a["min_opacity"], a["extent"], a["percent_dense"], 20)
        outs.append({k: v.detach().cpu() for k, v in new.items()})
    assert all(torch.equal(outs[0][k], outs[1][k]) for k in outs[0])


# ---- against the reference's own class ------------------------------------------------------------------------------------------

FIELDS = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}


def test_patched_reference_model_against_the_unpatched_one(request):
    """Two scene.gaussian_model.GaussianModel of 4099 Gaussians at SH degree 3 from the same tensors, one with the methods
    install_dropin(fuse_training_step=True) binds and one with the reference's own, through 6 iterations of add_densification_stats and
    optimizer.step() with a densify_and_prune after the third.  Truth: the float64 restatements chained on the CPU (its samples are
    the same unit normals times its own float64 scales); yardstick: the unpatched model."""
    import copy
    import os
    from argparse import ArgumentParser

    import seganygaussians_amd
    from oracle import build_ref
    if not os.path.exists(build_ref.pyref_path("scene.gaussian_model")):
        pytest.skip("oracle/_ref is absent (it is built from the reference tree by __graft_entry__.build())")
    from tests.ref_env import ReferenceEnv
    P, EXTENT, MAX_GRAD, MIN_OPACITY, SEED = 4099, 8.0, 0.0002, 0.005, 11
    case = ref.densify_case(P, 3, 77, max_grad=MAX_GRAD, min_opacity=MIN_OPACITY, extent=EXTENT, percent_dense=0.01)
    gen = torch.Generator().manual_seed(5)
    # screen-space gradients whose norm is the class's accum / denom in every iteration; rows with denom == 0 are never visible
    ratio = torch.where(case["denom"] > 0, case["accum"] / case["denom"].clamp_min(1), torch.full_like(case["accum"], 3 * MAX_GRAD))
    angle = torch.rand(P, 1, generator=gen) * 6.28
    vgrad = torch.cat((ratio * torch.cos(angle), ratio * torch.sin(angle), torch.randn(P, 1, generator=gen)), dim=1)
    radii = torch.where(case["denom"].reshape(-1) > 0, torch.randint(1, 30, (P,), generator=gen), torch.zeros(P, dtype=torch.long)).to(torch.int32)

    with ReferenceEnv() as env:
        GM = env.mod["scene.gaussian_model"].GaussianModel
        parser = ArgumentParser()
        opt_args = env.mod["arguments"].OptimizationParams(parser).extract(parser.parse_args([]))
        names = ("training_setup", "add_densification_stats", "densify_and_prune")
        Plain = type("PlainGaussianModel", (GM,), {n: GM.__dict__[n] for n in names})          # the reference's own three methods
        seganygaussians_amd.install_dropin(fuse_training_step=True)

        def unpatch():                                   # leave the class as the reference wrote it for whoever uses the module next
            for n in names:
                setattr(GM, n, Plain.__dict__[n])
                delattr(GM, "_reference_" + n)
            del GM._mi_fused_training_step
        request.addfinalizer(unpatch)
        assert GM.densify_and_prune is ts.fused_densify_and_prune and Plain.densify_and_prune is GM._reference_densify_and_prune

        def model(cls):
            m = cls(3)
            m.spatial_lr_scale = 1.0
            for k, f in FIELDS.items():
                setattr(m, f, torch.nn.Parameter(case["params"][k].to(DEV)))
            m.max_radii2D = torch.zeros(P, device=DEV)
            m.training_setup(opt_args)
            return m

        fused, plain = model(GM), model(Plain)
        assert isinstance(fused.optimizer, ts.FusedAdam) and type(plain.optimizer) is torch.optim.Adam
        assert [(g["name"], g["lr"]) for g in fused.optimizer.param_groups] == [(g["name"], g["lr"]) for g in plain.optimizer.param_groups]
        lrs = {g["name"]: g["lr"] for g in plain.optimizer.param_groups}
        z64 = lambda t: torch.zeros(t.shape, dtype=torch.float64)
        T = {k: t.double() for k, t in case["params"].items()}
        M = {k: (z64(t), z64(t)) for k, t in T.items()}
        mag = {k: {"p": t.abs(), "m": z64(t), "v": z64(t)} for k, t in T.items()}
        accum64, denom64 = torch.zeros(P, 1, dtype=torch.float64), torch.zeros(P, 1, dtype=torch.float64)
        step, worst = 0, 0.0

        def compare(it):
            nonlocal worst
            for k, f in FIELDS.items():
                a, b = getattr(fused, f), getattr(plain, f)
                assert a.shape == b.shape == T[k].shape, (it, k)
                sa, sb = fused.optimizer.state[a], plain.optimizer.state[b]
                for what, prod, truth, yard in (("p", a, T[k], b), ("m", sa["exp_avg"], M[k][0], sb["exp_avg"]), ("v", sa["exp_avg_sq"], M[k][1], sb["exp_avg_sq"])):
                    r = _rule(prod, truth, yard.detach().cpu(), mag[k][what])
                    assert (r <= 1.0).all(), (it, k, what, int(np.argmax(~(r <= 1.0))), float(np.nanmax(r)))
                    worst = max(worst, float(r.max()))
            assert fused.xyz_gradient_accum.shape == plain.xyz_gradient_accum.shape == accum64.shape
            r = _rule(fused.xyz_gradient_accum, accum64, plain.xyz_gradient_accum.cpu(), accum64)
            assert (r <= 1.0).all(), (it, "accum", float(np.nanmax(r)))
            assert torch.equal(fused.denom.cpu().double(), denom64) and torch.equal(plain.denom.cpu().double(), denom64)

        def iteration(it, models):
            nonlocal step, accum64, denom64
            n = T["xyz"].shape[0]
            g = {k: torch.randn(T[k].shape, generator=gen) * 10.0 ** float(it % 3 - 2) for k in FIELDS}
            vis = radii[:n] > 0 if n == P else torch.rand(n, generator=gen) < 0.5
            vg = vgrad if n == P else torch.randn(n, 3, generator=gen) * 1e-4
            for m in models:
                for k, f in FIELDS.items():
                    getattr(m, f).grad = g[k].to(DEV)
                view = type("ViewspacePoints", (), {"grad": vg.to(DEV)})()
                m.add_densification_stats(view, vis.to(DEV))
                m.optimizer.step()
            accum64[vis] += torch.norm(vg.double()[vis, :2], dim=-1, keepdim=True)
            denom64[vis] += 1
            step += 1
            for k in FIELDS:
                p, m_, v_, upd = ref.adam_restated(T[k], g[k].double(), M[k][0], M[k][1], step, lrs[k], B1, B2, 1e-15)
                T[k], M[k] = p, (m_, v_)
                mag[k] = {"p": mag[k]["p"] + upd, "m": mag[k]["m"] + g[k].double().abs(), "v": mag[k]["v"] + g[k].double() ** 2}

        for it in range(1, 4):
            iteration(it, (fused, plain))
            compare(it)
        # densify and prune after the third iteration, both under the same seed
        state = {"params": {k: getattr(plain, f).detach().cpu() for k, f in FIELDS.items()}, "accum": plain.xyz_gradient_accum.cpu(),
                 "denom": plain.denom.cpu(), "designated": 0, "args": dict(max_grad=MAX_GRAD, min_opacity=MIN_OPACITY, extent=EXTENT, percent_dense=0.01)}
        assert ref.decision_margins(state) > 16, "a decision quantity came within 16 ulp of its threshold"
        before = {k: getattr(fused, f).detach().cpu().clone() for k, f in FIELDS.items()}
        for m in (fused, plain):
            torch.manual_seed(SEED)
            m.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, 20)
        mask = ref.split_mask(T, accum64, denom64, MAX_GRAD, EXTENT, 0.01)
        n_split = int(mask.sum())
        torch.manual_seed(SEED)
        z = torch.normal(mean=torch.zeros((2 * n_split, 3), device=DEV), std=torch.ones((2 * n_split, 3), device=DEV)).cpu().double()
        out = ref.densify_restated(T, M, accum64, denom64, MAX_GRAD, MIN_OPACITY, EXTENT, 0.01, 20, z * torch.exp(T["scaling"][mask]).repeat(2, 1), torch.float64)
        src, kind = out["origin"], out["kind"]
        n = src.numel()
        assert 0 < n_split < P and n != P
        for k, f in FIELDS.items():
            got = getattr(fused, f).detach().cpu()
            rows = kind < 2 if k in ("xyz", "scaling") else torch.ones(n, dtype=torch.bool)
            assert got.shape[0] == n and torch.equal(got[rows], before[k][src][rows]), k                 # copied columns, bit for bit
            orig = (kind == 0).reshape((n,) + (1,) * (T[k].dim() - 1))
            extra = out["mag_xyz" if k == "xyz" else "mag_scaling"][:, None] if k in ("xyz", "scaling") else 0.0
            mag[k] = {"p": mag[k]["p"][src] + extra, "m": torch.where(orig, mag[k]["m"][src], 0.0), "v": torch.where(orig, mag[k]["v"][src], 0.0)}
            T[k], M[k] = out["params"][k], out["moments"][k]
        accum64, denom64 = torch.zeros(n, 1, dtype=torch.float64), torch.zeros(n, 1, dtype=torch.float64)
        assert not fused.max_radii2D.any() and fused.max_radii2D.shape == plain.max_radii2D.shape == (n,)
        compare("densify")
        for it in range(4, 7):
            iteration(it, (fused, plain))
            compare(it)
        # capture() of the patched model restores into an unpatched one, and the next step agrees
        restored = Plain(3)
        restored.restore(copy.deepcopy(fused.capture()), opt_args)
        assert type(restored.optimizer) is torch.optim.Adam and restored._xyz is not fused._xyz
        plain = restored
        iteration(7, (fused, restored))
        compare(7)
    print(f"patched GaussianModel against the unpatched one, 6 iterations + densify ({P} -> {n} rows) + restore: worst error / bound {worst:.3f}")
