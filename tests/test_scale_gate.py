"""GPU checks of scale conditioning (seganygaussians_amd/scale_gate.py, csrc/scale_gate.h).

Fit and transform have no tolerance: their arithmetic is specified operation by operation, so the tables are compared as int64 and
the outputs as int32 bit patterns with the fixture written from scikit-learn (tests/golden/scale_gate/scale_gate.npz) and with the
restatement of tests/scale_gate_ref.py.  The two gate tolerances are derived where they are used."""
import numpy as np
import pytest
import torch

from seganygaussians_amd import _lib
from seganygaussians_amd import scale_gate as sg
from tests import scale_gate_ref as sr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return sr.load_cases()


@pytest.fixture(scope="module")
def tables(golden):
    """One ScaleQuantile per case, loaded from scikit-learn's own table: the transform tests do not depend on the fit kernel."""
    return {name: sg.ScaleQuantile.from_state_dict(c, DEV) for name, c in golden[0].items()}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


@pytest.mark.parametrize("name", sr.CASES)
def test_fit_gives_scikit_learns_table(golden, name):
    cases, versions = golden
    c = cases[name]
    if name == "subsample":
        np.random.seed(versions["seed"])
    sq = sg.ScaleQuantile.fit(dev(c["data"]))
    assert sq.n_quantiles_ == c["quantiles"].size and sq.quantiles.dtype == torch.float64 and sq.quantiles.device == DEV
    assert np.array_equal(bits(sq.quantiles), bits(c["quantiles"])) and np.array_equal(bits(sq.references), bits(c["references"]))
    # a column, as the reference passes the scales, is the same fit
    if name == "subsample":
        np.random.seed(versions["seed"])
    assert np.array_equal(bits(sg.ScaleQuantile.fit(dev(c["data"]).reshape(-1, 1)).quantiles), bits(c["quantiles"]))


def test_fit_without_subsample_and_with_other_table_sizes(golden):
    data = golden[0]["subsample"]["data"]
    state = np.random.get_state()[1].copy()
    sq = sg.ScaleQuantile.fit(dev(data), subsample=None)
    assert np.array_equal(np.random.get_state()[1], state)      # nothing drawn
    assert np.array_equal(bits(sq.quantiles), bits(sr.fit_quantiles(data, subsample=None)[0]))
    data = golden[0]["gamma"]["data"]
    for nq in (1, 2, 3, 64, 999, 1000, 1024):
        sq = sg.ScaleQuantile.fit(dev(data), n_quantiles=nq)
        quantiles, references = sr.fit_quantiles(data, n_quantiles=nq)
        assert sq.n_quantiles_ == nq and np.array_equal(bits(sq.quantiles), bits(quantiles)), nq
        assert np.array_equal(bits(sq.references), bits(references)), nq
    nothing = sg.ScaleQuantile.fit(torch.full((70,), float("nan"), device=DEV))      # no value at all: NaN quantiles, as numpy gives
    assert nothing.n_quantiles_ == 70 and bool(torch.isnan(nothing.quantiles).all())


def test_state_dict_round_trip(golden, tables):
    c, sq = golden[0]["gamma"], tables["gamma"]
    state = sq.state_dict()
    assert set(state) == {"quantiles", "references"} and np.array_equal(bits(state["quantiles"]), bits(c["quantiles"]))
    again = sg.ScaleQuantile.from_state_dict({k: v.cpu() for k, v in state.items()}, DEV)
    assert np.array_equal(bits(again.quantiles), bits(c["quantiles"])) and np.array_equal(bits(again.references), bits(c["references"]))
    column = sg.ScaleQuantile.from_state_dict({"quantiles": c["quantiles"].reshape(-1, 1), "references": c["references"]}, DEV)      # quantiles_
    assert column.n_quantiles_ == 1000 and np.array_equal(bits(column.quantiles), bits(c["quantiles"]))


@pytest.mark.parametrize("name", sr.CASES)
def test_transform_gives_scikit_learns_bits(golden, tables, name):
    c, sq = golden[0][name], tables[name]
    x = dev(c["queries"])
    out = sq.transform(x)
    assert out.shape == x.shape and out.dtype == torch.float32 and out.device == DEV
    assert np.array_equal(bits(out), bits(c["outputs"]))      # NaN positions included: a NaN has its own pattern
    assert np.array_equal(np.isnan(out.cpu().numpy()), np.isnan(c["queries"]))
    # both kernels (the table read where it lies up to 64 scales, staged in LDS above), one and several workgroups, other shapes
    for n in (1, 63, 64, 65, 1000, 1025):
        pick = (np.arange(n) * 7 + n) % c["queries"].size
        assert np.array_equal(bits(sq.transform(x[dev(pick)])), bits(c["outputs"][pick])), n
    for shape in ((5, 1), (2, 3, 4)):
        count = int(np.prod(shape))
        out = sq.transform(x[-count:].reshape(shape))
        assert out.shape == shape and np.array_equal(bits(out), bits(c["outputs"][-count:].reshape(shape))), shape
    assert sq.transform(x[:0]).shape == (0,)


def _scales_and_u(golden, tables, n, seed):
    """n scales of the gamma case's queries, both ends of the table among them where there is room, and their u."""
    c = golden[0]["gamma"]
    finite = c["queries"][np.isfinite(c["queries"])]
    rng = np.random.default_rng(seed)
    x = finite[rng.integers(0, finite.size, n)]
    if n >= 4:
        x[1], x[2] = np.float32(c["quantiles"][0]), np.float32(c["quantiles"][-1])      # u == 0 and u == 1
    x = dev(x)
    return x, tables["gamma"].transform(x)


def _parameters(C, seed):
    g = torch.Generator().manual_seed(seed)
    w, b = torch.rand(C, 1, generator=g) * 16 - 8, torch.rand(C, generator=g) * 16 - 8
    return w.to(DEV), b.to(DEV)


@pytest.mark.parametrize("C", [1, 32, 33, 64, 256])
def test_gates_forward_against_float64(golden, tables, C):
    """|ours - f64| <= 2^-22 + 2^-25 (|w u| + |b|) per element: z = fl(fl(w u) + b) carries two float32 roundings, half an ulp of
    |w u| and of |z| <= |w u| + |b| each, at most 2^-24 (2 |w u| + |b|) together, and sigmoid' <= 1/4 takes that to at most
    2^-25 (|w u| + |b|); expf, the add and the divide cost at most 4 ulp at sigmoid <= 1, 2^-22."""
    w, b = _parameters(C, C)
    for n in (10, 300):      # the kernel that reads the table where it lies, and the staged one with two workgroups
        x, u = _scales_and_u(golden, tables, n, 100 * C + n)
        gates = sg.scale_gates(x, tables["gamma"], w, b)
        assert gates.shape == (n, C) and gates.dtype == torch.float32 and gates.device == DEV
        u64, w64, b64 = u.double().reshape(-1, 1), w.double().reshape(1, -1), b.double().reshape(1, -1)
        want = torch.sigmoid(u64 * w64 + b64)
        bound = 2.0 ** -22 + 2.0 ** -25 * ((u64 * w64).abs() + b64.abs())
        err = (gates.double() - want).abs()
        print(f"C {C} n {n}: max |ours - f64| / bound = {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())
        # PyTorch's own scale_gate on the same u meets the same bound, so the two lie within twice the bound of each other
        scale_gate = torch.nn.Sequential(torch.nn.Linear(1, C, bias=True), torch.nn.Sigmoid()).to(DEV)
        with torch.no_grad():
            scale_gate[0].weight.copy_(w), scale_gate[0].bias.copy_(b)
            theirs = scale_gate(u.unsqueeze(-1))
        assert bool(((gates.double() - theirs.double()).abs() <= 2 * bound).all())
        assert np.array_equal(bits(sg.scale_gates(x, tables["gamma"], w.reshape(-1), b)), bits(gates))      # weight as (C,)


def test_a_nan_scale_gives_a_nan_row(golden, tables):
    x, _ = _scales_and_u(golden, tables, 70, 5)
    x[3], x[69] = float("nan"), float("nan")
    w, b = _parameters(32, 1)
    for gates in (sg.scale_gates(x, tables["gamma"], w, b), sg.fixed_scale_gates(x, tables["gamma"], 10)):
        nan = torch.isnan(gates)
        assert bool(nan[[3, 69]].all()) and int(nan.sum()) == 2 * 32


@pytest.mark.parametrize("n", [1, 64, 65, 1025])
def test_gates_backward_against_float64_autograd(golden, tables, n):
    """|d_weight - f64| <= 2^-20 sum_n |g s' u| (d_bias: without u): at most 12 ulp of relative error per float32 term; the float64
    accumulation adds nothing visible."""
    for C in (32, 33):
        x, u = _scales_and_u(golden, tables, n, 10 * n + C)
        w, b = _parameters(C, n + C)
        g = torch.randn(n, C, generator=torch.Generator().manual_seed(n)).to(DEV)
        grads = []
        for _ in range(2):
            wp, bp = w.clone().requires_grad_(), b.clone().requires_grad_()
            sg.scale_gates(x, tables["gamma"], wp, bp).backward(g)
            assert wp.grad.shape == (C, 1) and bp.grad.shape == (C,) and wp.grad.dtype == torch.float32
            grads.append((wp.grad, bp.grad))
        assert np.array_equal(bits(grads[0][0]), bits(grads[1][0])) and np.array_equal(bits(grads[0][1]), bits(grads[1][1]))
        w64, b64, u64 = w.double().reshape(-1).requires_grad_(), b.double().requires_grad_(), u.double().reshape(-1, 1)
        s = torch.sigmoid(u64 * w64.reshape(1, -1) + b64.reshape(1, -1))
        s.backward(g.double())
        terms = (g.double() * s * (1 - s)).abs().detach()
        bound_w, bound_b = 2.0 ** -20 * (terms * u64).sum(0), 2.0 ** -20 * terms.sum(0)
        err_w, err_b = (grads[0][0].double().reshape(-1) - w64.grad).abs(), (grads[0][1].double() - b64.grad).abs()
        tiny = 1e-300
        print(f"n {n} C {C}: max error / bound: d_weight {float((err_w / (bound_w + tiny)).max()):.4f} d_bias {float((err_b / (bound_b + tiny)).max()):.4f}")
        assert bool((err_w <= bound_w).all()) and bool((err_b <= bound_b).all())


def test_scales_get_no_gradient(golden, tables):
    x, _ = _scales_and_u(golden, tables, 10, 3)
    w, b = _parameters(32, 2)
    x.requires_grad_()
    sg.scale_gates(x, tables["gamma"], w.requires_grad_(), b.requires_grad_()).sum().backward()
    assert x.grad is None and w.grad is not None and b.grad is not None


@pytest.mark.parametrize("dim", [1, 10, 31])
def test_fixed_gates_are_the_references_expression(golden, tables, dim):
    for n in (10, 300):
        x, u = _scales_and_u(golden, tables, n, dim + n)
        assert float(u[1]) == 0 and float(u[2]) == 1
        gates = sg.fixed_scale_gates(x, tables["gamma"], dim)
        # train_contrastive_feature.py:131 and :243-244
        fixed_scale_gate = torch.tensor([[1 for j in range(32 - dim + i)] + [0 for k in range(dim - i)] for i in range(dim + 1)]).to(DEV)
        want = fixed_scale_gate[((1 - u.squeeze()) * dim).long()]
        assert gates.shape == (n, 32) and gates.dtype == torch.float32 and torch.equal(gates, want.float())
        assert int(gates[1].sum()) == 32 and int(gates[2].sum()) == 32 - dim
    other = sg.fixed_scale_gates(x, tables["gamma"], 3, channels=8)
    assert other.shape == (300, 8) and torch.equal(other.sum(1), (5 + ((1 - u) * 3).long()).float())


def test_get_quantile_func_is_the_references_q_trans(golden):
    c = golden[0]["gamma"]
    q_trans = sg.get_quantile_func(torch.from_numpy(c["data"]), "uniform")      # all_scales lives on the host
    pick = np.r_[200:209, c["queries"].size - 10]      # nine fresh draws and 1e9, above the fitted maximum
    assert c["queries"][pick[-1]] == np.float32(1e9) > c["quantiles"][-1]
    sampled_scales = dev(c["queries"][pick])
    out = q_trans(sampled_scales)
    assert out.shape == (10, 1) and out.device == sampled_scales.device and out.dtype == torch.float32
    assert np.array_equal(bits(out.squeeze()), bits(c["outputs"][pick])) and float(out[-1]) == 1
    assert np.array_equal(bits(q_trans.scale_quantile.quantiles), bits(c["quantiles"]))
    assert np.array_equal(bits(sg.get_quantile_func(dev(c["data"]).reshape(50, 50), "uniform")(sampled_scales)), bits(out))


def test_no_host_synchronisation(golden, tables):
    sq = tables["gamma"]
    x, _ = _scales_and_u(golden, tables, 300, 9)
    w, b = _parameters(32, 4)
    w.requires_grad_(), b.requires_grad_()
    g = torch.ones(300, 32, device=DEV)
    sg.scale_gates(x, sq, w, b).backward(g)      # once outside: the library is loaded and bound
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        sq.transform(x)
        sg.scale_gates(x, sq, w, b).backward(g)
        sg.fixed_scale_gates(x, sq, 10)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()


def test_a_refused_call_sets_the_last_error(tables):
    L, sq = _lib.load(), tables["gamma"]
    x = torch.zeros(4, device=DEV)
    u = torch.empty_like(x)
    args = lambda n, nq: (n, x.data_ptr(), nq, sq.quantiles.data_ptr(), sq.references.data_ptr(), 0, 1, None, None, 0, u.data_ptr(), None, None)
    assert L.mi_scale_gate_forward(*args(0, 1000)) != 0 and _lib.last_error() == "scale gate: need 1 <= n < 2^30 scales"
    assert L.mi_scale_gate_forward(*args(4, 1025)) != 0 and _lib.last_error() == "scale gate: need 1 <= nq <= 1024 quantiles"
    assert L.mi_scale_gate_forward(*args(4, 1000)) == 0
    torch.cuda.synchronize()
