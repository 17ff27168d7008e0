"""The argument checks the feature modules share (_args.py; the feature-table pieces in segmentation.py; the mask pieces are in
test_packed_masks_host.py), called directly: what each accepts and returns, and the exact text of each refusal.  CPU-only; a GPU tensor is
stood in for by a CPU tensor whose is_cuda and device say otherwise."""
import re

import pytest
import torch

from seganygaussians_amd import _args, segmentation


def on_gpu(t, device="cuda:0"):
    """t as a tensor that says it is on a GPU: what the checks read of a GPU tensor, without a GPU."""
    return t.as_subclass(type("OnGpu", (torch.Tensor,), {"is_cuda": True, "device": torch.device(device)}))


def refuses(text):
    return pytest.raises(ValueError, match="^" + re.escape(text) + "$")


def test_number_and_to_float():
    for v, want in ((2, 2.0), ("0.5", 0.5), (True, 1.0), (torch.tensor(3.0), 3.0), (float("inf"), float("inf"))):
        got = _args.number("f", "x", v)
        assert type(got) is float and got == want
        assert _args.to_float("f", "x", v) == want
    for v in (None, "a", [1], torch.zeros(2)):
        with refuses(f"f: x must be a number, got {v!r}"):
            _args.number("f", "x", v)
        with refuses(f"f: x must be a number, got {v!r}"):
            _args.to_float("f", "x", v)
    with refuses("f: x is NaN"):
        _args.number("f", "x", float("nan"))
    assert _args.to_float("f", "x", float("nan")) != _args.to_float("f", "x", float("nan"))   # to_float leaves NaN to its caller


def test_f32():
    t = torch.zeros(2)
    assert _args.f32("f", "x", t) is t and _args.f32("f", "x", t, optional=True) is t
    assert _args.f32("f", "x", None, optional=True) is None
    with refuses("f: x must be a float32 tensor, got <class 'NoneType'>"):
        _args.f32("f", "x", None)
    with refuses("f: x must be a float32 tensor, got torch.float64"):
        _args.f32("f", "x", t.double())
    with refuses("f: x must be a float32 tensor or None, got torch.int32"):
        _args.f32("f", "x", t.int(), optional=True)
    with refuses("f: x must be a float32 tensor or None, got <class 'list'>"):
        _args.f32("f", "x", [1.0], optional=True)


def test_size_hw():
    assert _args.size_hw("f", (3, 4)) == (3, 4) and _args.size_hw("f", [2.9, torch.tensor(5)]) == (2, 5)
    for v in (5, (1, 2, 3), ("a", "b"), None):
        with refuses(f"f: size must be (H, W), got {v!r}"):
            _args.size_hw("f", v)
    with refuses("f: size must be positive, got (0, 3)"):
        _args.size_hw("f", (0, 3))
    with refuses("f: size must be positive, got (3, -1)"):
        _args.size_hw("f", (3, -1))


def test_no_grad_one_gpu():
    a, b, other = on_gpu(torch.zeros(2)), on_gpu(torch.zeros(3)), on_gpu(torch.zeros(2), "cuda:1")
    assert _args.no_grad_one_gpu("f", [("a", a), ("b", b)]) == torch.device("cuda:0")
    assert _args.no_grad_one_gpu("f", [("a", other)], "features") == torch.device("cuda:1")
    # the two wordings of a tensor on another GPU than the first
    with refuses("f: b is on cuda:1, expected cuda:0"):
        _args.no_grad_one_gpu("f", [("a", a), ("b", other)])
    with refuses("f: b is on cuda:1, the features on cuda:0"):
        _args.no_grad_one_gpu("f", [("a", a), ("b", other)], "features")
    with refuses("f: a is on cuda:0, the features on cuda:1"):
        _args.no_grad_one_gpu("f", [("o", other), ("a", a)], "features")
    with refuses("f: c must be on a GPU, got cpu (there is no CPU fallback)"):
        _args.no_grad_one_gpu("f", [("a", a), ("c", torch.zeros(2))])
    # on the CPU comes before on another GPU, in the order of the list
    with refuses("f: c must be on a GPU, got cpu (there is no CPU fallback)"):
        _args.no_grad_one_gpu("f", [("a", a), ("c", torch.zeros(2)), ("b", other)])
    g = torch.zeros(2, requires_grad=True)
    # requires grad comes before everything else, whatever the position
    with refuses("f: g requires grad and there is no backward; call under torch.no_grad() or detach it"):
        _args.no_grad_one_gpu("f", [("c", torch.zeros(2)), ("g", g)])
    with torch.no_grad(), refuses("f: g must be on a GPU, got cpu (there is no CPU fallback)"):
        _args.no_grad_one_gpu("f", [("a", a), ("g", g)])


def test_check_out():
    dev = torch.device("cuda:0")
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32)
    assert _args.check_out("f", on_gpu(i32(4, 6)), (4, 6), torch.int32, dev) is None
    text = "f: out must be a contiguous int32 (4, 6) tensor on cuda:0"
    for bad in ([1], None, on_gpu(torch.zeros(4, 6)), on_gpu(i32(4, 7)), on_gpu(i32(6, 4)), on_gpu(i32(4, 6), "cuda:1"),
                on_gpu(i32(6, 4).t()), i32(4, 6)):
        with refuses(text):
            _args.check_out("f", bad, (4, 6), torch.int32, dev)
    with refuses("f: out must be a contiguous float32 (2, 4, 6) tensor on cuda:0"):
        _args.check_out("f", torch.zeros(2, 4, 6), (2, 4, 6), torch.float32, dev)
    # clip_tiles spells the dtype the way torch prints it
    with refuses("f: out must be a contiguous torch.float16 (3, 3, 8, 8) tensor on cuda:0"):
        _args.check_out("f", None, (3, 3, 8, 8), torch.float16, dev, dtype_name=str(torch.float16))
    out = torch.zeros(4, 2)
    assert _args.check_out("f", out, (4, 2), torch.float32, torch.device("cpu")) is None
    with refuses("f: out must be a contiguous float32 (2, 4) tensor on cpu"):
        _args.check_out("f", out.t(), (2, 4), torch.float32, torch.device("cpu"))   # the right shape, not contiguous


def test_feature_table():
    assert segmentation.feature_table("f", torch.zeros(5, 3, 4)) == (0, 5, 12, (3, 4))
    assert segmentation.feature_table("f", torch.zeros(7, 5)) == (1, 5, 7, (7,))
    with refuses("f: features must be a float32 tensor, got torch.float64"):
        segmentation.feature_table("f", torch.zeros(7, 5).double())
    for shape in ((4,), (1, 5, 3, 4)):
        with refuses(f"f: features must be (C, H, W) or (P, C), got {shape}"):
            segmentation.feature_table("f", torch.zeros(shape))
    with refuses("f: need 1 <= C <= 256 channels, got 257"):
        segmentation.feature_table("f", torch.zeros(257, 1, 1))
    with refuses("f: need 1 <= C <= 256 channels, got 0"):
        segmentation.feature_table("f", torch.zeros(3, 0))
    with refuses("f: need 1 <= N < 2^31 rows, got 0"):
        segmentation.feature_table("f", torch.zeros(5, 0, 4))
    with refuses("f: need 1 <= N < 2^31 rows, got 2147483648"):
        segmentation.feature_table("f", torch.zeros(1).expand(1, 1 << 16, 1 << 15))


def test_query_rows():
    q = torch.zeros(2, 5)
    got, Q = segmentation.query_rows("f", q, 5, 16)
    assert got is q and Q == 2
    got, Q = segmentation.query_rows("f", torch.zeros(5), 5, 16)
    assert tuple(got.shape) == (1, 5) and Q == 1
    with refuses("f: centers must be a float32 tensor, got <class 'NoneType'>"):
        segmentation.query_rows("f", None, 5, 16, "centers")
    for shape, shown in (((2, 6), (2, 6)), ((6,), (1, 6)), ((1, 2, 5), (1, 2, 5))):   # a 1-D tensor is shown as the row it became
        with refuses(f"f: queries must be (Q, 5) or (5,), got {shown}"):
            segmentation.query_rows("f", torch.zeros(shape), 5, 16)
    with refuses("f: need 1 <= queries <= 16, got 17"):
        segmentation.query_rows("f", torch.zeros(17, 5), 5, 16)
    with refuses("f: need 1 <= centers <= 4096, got 0"):
        segmentation.query_rows("f", torch.zeros(0, 5), 5, 4096, "centers")


def test_gate_row_and_check_pre():
    assert segmentation.gate_row("f", None, 5) is None
    for shape in ((5,), (1, 5), (5, 1)):
        assert tuple(segmentation.gate_row("f", torch.zeros(shape), 5).shape) == (5,)
    with refuses("f: gates must be a float32 tensor or None, got torch.int64"):
        segmentation.gate_row("f", torch.zeros(5, dtype=torch.int64), 5)
    for shape in ((6,), (1, 1, 5)):
        with refuses(f"f: gates must hold 5 values, got {shape}"):
            segmentation.gate_row("f", torch.zeros(shape), 5)
    for pre in segmentation.PRE_MODES:
        assert segmentation.check_pre("f", pre) is None
    with refuses("f: pre must be one of ['eps', 'l2', 'none'], got 'L2'"):
        segmentation.check_pre("f", "L2")
    with refuses("f: pre must be one of ['eps', 'l2', 'none'], got None"):
        segmentation.check_pre("f", None)
