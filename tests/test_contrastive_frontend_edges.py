"""The contrastive front end (csrc/contrastive.h, contrastive_front_end) at the edges of its kernels -- the channel passes of a
ray's wave (lane + 64 k up to C = 256, the last pass partial), the gate batches of the backward (CT_GB = 5) and its LDS passes
(4096 / C gates), 0 to 257 rays against the four rays of a workgroup, rays on corners and borders, equal rays, single-row and
single-column images, the scalar path through an unaligned pointer, zero pixels and zero gates -- against a float64
restatement (tests/edge_ref.py: front_end) under the per-group rule of that module:

    |product - f64| <= max(4 * E32, 2^-22 * magnitude of the terms summed into the group)        (2^-21 for an out row)

with the groups: every out row (n, s, :), the regulariser, the ray-tap part of dL/drendered, every row of dL/dgates, the dense part
of dL/drendered.  The dense and the tap part are bounded apart (at 1080p the dense term is 1e-6 of the tap term); where both are
asked for at once, their sum is held to the sum of the two bounds.  E32 is the same restatement in float32 on the CPU.  Both take
the bilinear taps as float32 computes them (test_float32_taps_are_those_of_interpolate pins them to F.interpolate).

Measured on the CPU (test_float32_reference_in_another_order_meets_the_rule, every case below): the float32 restatement in a
second evaluation order (channels permuted, rays and gates walked last to first) meets the rule at FACTOR = 4 with the floor at
2^-22 of the terms in every group but the out rows.  All elements of an out row share one rounding error, that of the row's
length (a sum of C squares), so E32 of a row is in effect a single draw; where it is small the other order lies up to
6.0 * 2^-24 of the terms away from float64 (N = 32, C = 256).  As the rule says the floor is widened there, not the factor:
2^-21 of the terms for out rows (edge_ref.OUT_ROW_FLOOR).  With it the second order's worst error / bound is: out rows 0.79,
regulariser 0.50, taps 0.45, gate rows 0.70, dense 0.38.

Order of float atomics: the tap gradients of rays that share a tap and the gate gradients of more than two workgroups are added
in an order that changes from run to run, so bit-identity of the backward is asserted only where at most two atomics meet on an
address (no shared taps; S <= 8 for the gates); everywhere else two runs both meet the rule."""
import numpy as np
import pytest
import torch

from seganygaussians_amd.contrastive_frontend import _ContrastiveFrontEnd, contrastive_front_end
from tests import edge_ref as er

UP3 = ((11, 13), (33, 39))        # x3 up-sampling, odd h w (scalar path): neighbouring rays share taps
DOWN = ((40, 36), (13, 9))        # down-sampling, h w % 4 == 0
IDENT = ((16, 20), (16, 20))      # identity, h w % 4 == 0 (vector path)
SIZES = {"up3": UP3, "down": DOWN, "ident": IDENT, "h1": ((1, 9), (4, 18)), "w1": ((7, 1), (14, 3)), "H1": ((6, 8), (1, 16)),
         "odd": ((9, 7), (20, 11)), "full": ((540, 960), (540, 960))}
CHANNELS = (1, 3, 63, 64, 65, 128, 129, 255, 256)
GATES = (1, 4, 5, 6, 10, 11, 32)
RAYS = (0, 1, 3, 4, 5, 257)


def _rays(kind, H, W, S, g):
    if kind == "random":                                  # distinct pixels, any order
        p = torch.randperm(H * W, generator=g)[:S]
        return torch.stack([p // W, p % W], dim=1).int()
    if kind == "repeat":                                  # S draws with replacement: equal rays where S > H W
        p = torch.randint(0, H * W, (S,), generator=g)
        return torch.stack([p // W, p % W], dim=1).int()
    if kind == "corners":
        return torch.tensor([[0, 0], [0, W - 1], [H - 1, 0], [H - 1, W - 1]], dtype=torch.int32)
    if kind == "borders":
        ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        m = (ys == 0) | (ys == H - 1) | (xs == 0) | (xs == W - 1)
        return torch.stack([ys[m], xs[m]], dim=1).int()
    if kind == "twice":                                   # the same ray two times among others
        r = _rays("random", H, W, 6, g)
        r[4] = r[1]
        return r
    if kind == "x64":                                     # the same ray 64 times, and three others
        r = _rays("random", H, W, 67, g)
        r[2:66] = r[0]
        return r
    if kind == "one_pixel":
        return torch.tensor([[H // 2, W // 3]], dtype=torch.int32).repeat(S, 1)
    if kind == "all":
        ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        return torch.stack([ys.reshape(-1), xs.reshape(-1)], dim=1).int()
    raise ValueError(kind)


def make(C=32, size="up3", N=3, rays="random", S=37, seed=0, zero_pixel=False, zero_gate_row=None, zero_gate_channel=None):
    (h, w), (H, W) = SIZES[size]
    g = torch.Generator().manual_seed(1000 * C + 10 * N + S + seed)
    rendered = torch.randn(C, h, w, generator=g)
    if zero_pixel:
        rendered[:, h // 2, w // 2] = 0.0
    gates = torch.rand(N, C, generator=g)
    if zero_gate_row is not None:
        gates[zero_gate_row] = 0.0
    if zero_gate_channel is not None:
        gates[:, zero_gate_channel] = 0.0
    ray_yx = _rays(rays, H, W, S, g)
    up = torch.randn(N, ray_yx.shape[0], C, generator=g)
    return {"rendered": rendered, "gates": gates, "ray_yx": ray_yx, "up": up, "gn": 0.37, "hw": (H, W)}


def _cases():
    c = {}
    for C in CHANNELS:
        c[f"C{C}"] = dict(C=C)
    for N in GATES:
        c[f"N{N}"] = dict(N=N, size="down", S=9)
    c["N32-C256"] = dict(N=32, C=256, S=9)                # two LDS passes of 16 gates: refused by the backward before
    c["N17-C256"] = dict(N=17, C=256, S=5)                # 16 + 1 gates
    c["N32-C129"] = dict(N=32, C=129, S=6)                # passes of 31 gates, the last of one
    c["N31-C255"] = dict(N=31, C=255, S=3)
    for S in RAYS:
        c[f"S{S}"] = dict(S=S, N=6, size="ident")
    c["S257-repeat"] = dict(S=257, N=5, rays="repeat", size="odd")
    for kind in ("corners", "borders", "twice", "x64"):
        for size in ("up3", "down", "ident"):
            c[f"{kind}-{size}"] = dict(rays=kind, size=size, N=4)
    c["one_pixel"] = dict(rays="one_pixel", S=50, N=3)
    for size in ("h1", "w1", "H1", "odd"):
        c[f"all-{size}"] = dict(rays="all", size=size, N=5, C=7)
    c["all-up3"] = dict(rays="all", size="up3", N=2, C=5)
    c["zero_pixel"] = dict(zero_pixel=True, rays="all", size="odd", C=6)
    c["zero_gate_row"] = dict(zero_gate_row=1, N=3, size="ident")
    c["zero_gate_channel"] = dict(zero_gate_channel=2, C=5, size="down")
    return c


CASES = _cases()


def _reference(case):
    a = (case["rendered"], case["hw"], case["ray_yx"], case["gates"])
    return er.front_end(*a, torch.float64, case["up"], case["gn"]), er.front_end(*a, torch.float32, case["up"], case["gn"])


# ---- CPU ------------------------------------------------------------------------------------------------------------------------

def test_float32_taps_are_those_of_interpolate():
    """For every (in, out) size pair of this file: the taps of edge_ref.taps_f32, laid out as a weight matrix, equal index by
    index what F.interpolate(mode='bilinear') makes of float32 one-hot rows."""
    pairs = set()
    for (h, w), (H, W) in SIZES.values():
        pairs |= {(h, H), (w, W)}
    pairs |= {(1080, 1080), (1920, 1920), (360, 1080), (1080, 360)}
    for n_in, n_out in sorted(pairs):
        i0, i1, lam = er.taps_f32(n_out, n_in)
        eye = torch.eye(n_in)
        want = torch.nn.functional.interpolate(eye.reshape(1, n_in, 1, n_in), (1, n_out), mode="bilinear")[0, :, 0, :]   # (in, out)
        lam_t = torch.from_numpy(lam)
        got = eye[:, torch.from_numpy(i0)] * (1 - lam_t) + eye[:, torch.from_numpy(i1)] * lam_t
        assert torch.equal(got, want), (n_in, n_out)
        assert i0.min() >= 0 and i1.max() <= n_in - 1 and (lam >= 0).all() and (lam <= 1).all()


def test_restatement_matches_the_reference_expression():
    """The float64 restatement against train_contrastive_feature.py:237-254 written out with F.interpolate in float64: equal up to
    the float32 rounding of the taps (about n_in 2^-24 of a weight), and exactly where the taps are exact (identity)."""
    from tests.test_contrastive_frontend import _reference
    for size, tol in (("ident", 1e-12), ("up3", 2e-5), ("down", 2e-5)):
        case = make(size=size, rays="all", C=4)
        H, W = case["hw"]
        f64 = er.front_end(case["rendered"], case["hw"], case["ray_yx"], case["gates"], torch.float64, case["up"], case["gn"])
        want = _reference(case["rendered"].double(), (H, W), torch.ones(H, W, dtype=torch.bool), case["gates"].double())
        torch.testing.assert_close(f64["out"], want, rtol=0, atol=tol)
        torch.testing.assert_close(f64["norm"], case["rendered"].double().norm(dim=0).mean(), rtol=1e-14, atol=0)


@pytest.mark.parametrize("name", list(CASES))
def test_float32_reference_in_another_order_meets_the_rule(name):
    """The float32 restatement with the channels permuted and the rays and gates walked last to first, put through the very
    check the kernels get (figures in this module's docstring)."""
    case = make(**CASES[name])
    f64, f32 = _reference(case)
    C = case["rendered"].shape[0]
    other = er.front_end(case["rendered"], case["hw"], case["ray_yx"], case["gates"], torch.float32, case["up"], case["gn"],
                         channel_perm=torch.randperm(C, generator=torch.Generator().manual_seed(1)), reverse=True)
    other["d_both"] = (other["d_tap"].float() + other["d_dense"].float()).double()
    er.front_end_check(name + " (f32, second order)", other, f64, f32)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

def _gpu(case, rendered_dev=None):
    """Forward, then the three gradient paths each alone -- only `out` used, only the norm used, both used."""
    dev = "cuda:0"
    r = (case["rendered"].to(dev) if rendered_dev is None else rendered_dev).requires_grad_(True)
    gt = case["gates"].to(dev).requires_grad_(True)
    up = case["up"].to(dev)
    gn = torch.tensor(case["gn"], device=dev)
    out, norm = contrastive_front_end(r, case["hw"], case["ray_yx"].to(dev), gt)
    res = {"out": out.detach().cpu(), "norm": norm.detach().cpu()}
    res["d_dense"] = torch.autograd.grad(norm, r, gn, retain_graph=True)[0].cpu()
    if out.numel():
        d_tap, d_gates = torch.autograd.grad(out, [r, gt], up, retain_graph=True)
        res["d_tap"], res["d_gates"] = d_tap.cpu(), d_gates.cpu()
        d_both, d_gates2 = torch.autograd.grad([out, norm], [r, gt], [up, gn])
        res["d_both"], res["d_gates_both"] = d_both.cpu(), d_gates2.cpu()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_hip_meets_the_rule(name):
    case = make(**CASES[name])
    f64, f32 = _reference(case)
    got = _gpu(case)
    er.front_end_check(name, got, f64, f32)
    if "d_gates_both" in got:
        er.front_end_check(name + " (gates, both used)", {"d_gates": got["d_gates_both"]}, f64, f32)
    kw = CASES[name]
    if kw.get("zero_pixel"):
        (h, w), _ = SIZES[kw["size"]]
        assert not got["d_dense"][:, h // 2, w // 2].any(), "the dense gradient of a zero pixel is exactly 0"
    if kw.get("zero_gate_row") is not None:
        assert not got["out"][kw["zero_gate_row"]].any()
        assert got["d_gates"][kw["zero_gate_row"]].abs().max() > 1e9          # F.normalize's 1 / eps branch, bounded above
    if kw.get("zero_gate_channel") is not None:
        assert not got["out"][:, :, kw["zero_gate_channel"]].any()


@pytest.mark.gpu
def test_hip_channel_limit_and_dense_only():
    """What include/mi_contrastive.h states: with rays C <= 256 and N <= 32, refused by the FORWARD; without rays (S = 0) only the
    dense part runs and it takes any C."""
    dev = "cuda:0"
    case = make(C=257, size="ident", S=4)
    with pytest.raises(RuntimeError, match="contrastive: at most 256 channels"):
        contrastive_front_end(case["rendered"].to(dev), case["hw"], case["ray_yx"].to(dev), case["gates"].to(dev))
    case = make(C=257, size="ident", S=0)
    f64, f32 = _reference(case)
    got = _gpu(case)
    assert got["out"].shape == (3, 0, 257)
    er.front_end_check("C257-S0", got, f64, f32)
    # N: 32 gates run (test_hip_meets_the_rule[N32-C256]); 33 are refused where the forward is called, not in backward()
    case = make(C=8, N=33, size="ident", S=4)
    r = case["rendered"].to(dev).requires_grad_(True)
    with pytest.raises(RuntimeError, match="contrastive: at most 32 scales"):
        contrastive_front_end(r, case["hw"], case["ray_yx"].to(dev), case["gates"].to(dev))
    case = make(C=256, N=33, size="ident", S=0)          # no rays: nothing to refuse
    f64, f32 = _reference(case)
    er.front_end_check("C256-N33-S0", _gpu(case), f64, f32)


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["ident", "down"])
def test_hip_unaligned_pointer_takes_the_scalar_path(size):
    """h w % 4 == 0 and an aligned `rendered` take the 4-pixel vector path; the same data as a view at a 4-byte storage offset
    takes the scalar path.  Outputs and the dense gradient agree element for element; the regulariser (another reduction tree)
    within the rule."""
    dev = "cuda:0"
    case = make(C=12, size=size, N=4, S=30)
    f64, f32 = _reference(case)
    C, h, w = case["rendered"].shape
    assert (h * w) % 4 == 0
    aligned = case["rendered"].to(dev)
    base = torch.zeros(C * h * w + 1, device=dev)
    base[1:] = aligned.reshape(-1)
    view = base[1:].view(C, h, w).detach()
    assert aligned.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    a, b = _gpu(case, aligned), _gpu(case, view)
    er.front_end_check(f"aligned-{size}", a, f64, f32)
    er.front_end_check(f"offset-{size}", b, f64, f32)
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["d_dense"], b["d_dense"])


class _Ctx:
    """Stands in for autograd's context so that backward() can be handed None (autograd itself materialises zeros)."""
    def save_for_backward(self, *t):
        self.saved_tensors = t


@pytest.mark.gpu
def test_hip_backward_takes_none_for_either_gradient():
    """d_out is None: the regulariser's gradient alone; d_norm is None: the rays' alone -- each under its own group's rule."""
    dev = "cuda:0"
    case = make(C=65, size="down", N=6, S=11)
    f64, f32 = _reference(case)
    ctx = _Ctx()
    _ContrastiveFrontEnd.forward(ctx, case["rendered"].to(dev), case["gates"].to(dev), case["ray_yx"].to(dev), *case["hw"])
    d_r, d_g = _ContrastiveFrontEnd.backward(ctx, None, torch.tensor(case["gn"], device=dev))[:2]
    assert not d_g.any()
    er.front_end_check("d_out=None", {"d_dense": d_r.cpu()}, f64, f32)
    d_r, d_g = _ContrastiveFrontEnd.backward(ctx, case["up"].to(dev), None)[:2]
    er.front_end_check("d_norm=None", {"d_tap": d_r.cpu(), "d_gates": d_g.cpu()}, f64, f32)


@pytest.mark.gpu
def test_hip_determinism():
    """Forward: bit-identical.  Backward: bit-identical where at most two atomics meet on an address -- distinct rays under the
    identity resize share no tap (the upper taps carry weight 0) and S <= 8 is two workgroups; with shared taps (x3 up-sampling,
    every pixel a ray) two runs differ in the order of the float atomics and both meet the rule."""
    bits = lambda t: t.contiguous().view(torch.int32)
    case = make(C=70, size="ident", N=7, S=8)
    a, b = _gpu(case), _gpu(case)
    for k in ("out", "norm", "d_tap", "d_gates", "d_dense", "d_both"):
        assert torch.equal(bits(a[k]), bits(b[k])), k
    case = make(C=33, size="ident", N=7, S=300)           # 75 workgroups: the taps still meet no other ray's
    a, b = _gpu(case), _gpu(case)
    for k in ("out", "norm", "d_tap", "d_dense", "d_both"):
        assert torch.equal(bits(a[k]), bits(b[k])), k
    case = make(C=5, size="up3", N=2, rays="all")
    f64, f32 = _reference(case)
    a, b = _gpu(case), _gpu(case)
    assert torch.equal(bits(a["out"]), bits(b["out"])) and torch.equal(bits(a["norm"]), bits(b["norm"]))
    er.front_end_check("shared taps, run 1", a, f64, f32)
    er.front_end_check("shared taps, run 2", b, f64, f32)


_FULL = {}


def _full_case():
    """C = 32, N = 10, S = 1000 at 540p (1080p takes the float64 autograd of the CPU restatement past a few seconds; the kernels'
    tiling does not depend on the image size beyond the grid).  Computed once per test run."""
    if not _FULL:
        case = make(C=32, size="full", N=10, S=1000)
        _FULL["case"], (_FULL["f64"], _FULL["f32"]) = case, _reference(case)
    return _FULL["case"], _FULL["f64"], _FULL["f32"]


@pytest.mark.gpu
def test_hip_full_size_meets_the_rule():
    case, f64, f32 = _full_case()
    got = _gpu(case)
    er.front_end_check("full size 32 x 540p x 10 x 1000", got, f64, f32)
