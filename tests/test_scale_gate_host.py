"""CPU checks of scale conditioning (seganygaussians_amd/scale_gate.py): the restatement of
tests/scale_gate_ref.py against the fixture written from scikit-learn and, where scikit-learn is installed, against the library
itself, bit for bit; where the ABI lives; the argument checks before the library is loaded and the refusals of the C entry points
before any HIP call.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from seganygaussians_amd import _lib, build
from seganygaussians_amd import scale_gate as sg
from tests import scale_gate_ref as sr


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


@pytest.fixture(scope="module")
def cases():
    return sr.load_cases()


def bits(a):
    a = np.asarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def test_fixture_holds_what_the_issue_lists(cases):
    cases, versions = cases
    assert versions == {"sklearn": "1.7.2", "numpy": "2.2.6", "seed": 123} and os.path.getsize(sr.GOLDEN) < 300_000
    assert {k: c["data"].size for k, c in cases.items()} == {"gamma": 2500, "ties": 300, "constant": 64, "n1": 1, "n2": 2, "n3": 3,
                                                            "nan7": 500, "subsample": 10_001}
    assert {k: c["quantiles"].size for k, c in cases.items()} == {"gamma": 1000, "ties": 300, "constant": 64, "n1": 1, "n2": 2, "n3": 3,
                                                                 "nan7": 500, "subsample": 1000}
    assert int(np.count_nonzero(~np.isnan(cases["nan7"]["data"]))) == 428 and np.isnan(cases["nan7"]["data"][::7]).all()
    assert np.array_equal(cases["ties"]["data"] * 8, np.round(cases["ties"]["data"] * 8)) and len(set(cases["constant"]["data"])) == 1
    for name, c in cases.items():
        q, x, y = c["quantiles"], c["queries"], c["outputs"]
        assert c["data"].dtype == np.float32 and x.dtype == np.float32 and y.dtype == np.float32 and q.dtype == np.float64, name
        assert x.shape == y.shape and np.array_equal(x[:min(200, c["data"].size)], c["data"][:200], equal_nan=True), name
        q0, q1 = np.float32(q[0]), np.float32(q[-1])
        up, down = np.float32(np.inf), np.float32(-np.inf)
        tail = [0, -1, 1e9, q0, q1, np.nextafter(q0, up), np.nextafter(q0, down), np.nextafter(q1, up), np.nextafter(q1, down), np.nan, up, down]
        assert np.array_equal(x[-12:], np.asarray(tail, np.float32), equal_nan=True), name
        assert np.array_equal(np.isnan(y), np.isnan(x)) and np.nanmin(y) == 0 and np.nanmax(y) <= 1, name
        assert y[-2] == (1 if q.size > 1 else 0) and y[-1] == 0, name      # the infinities; one quantile has the single reference 0


def test_restatement_gives_the_fixtures_bits(cases):
    cases, versions = cases
    for name, c in cases.items():
        if name == "subsample":
            np.random.seed(versions["seed"])
        quantiles, references = sr.fit_quantiles(c["data"])
        assert np.array_equal(bits(quantiles), bits(c["quantiles"])), name
        assert np.array_equal(bits(references), bits(c["references"])), name
        assert np.array_equal(bits(sr.transform(c["queries"], c["quantiles"], c["references"])), bits(c["outputs"])), name
    # a column and a block of queries keep their shape
    c = cases["gamma"]
    assert sr.transform(c["queries"][:24].reshape(2, 3, 4), c["quantiles"], c["references"]).shape == (2, 3, 4)


@pytest.mark.parametrize("kind", ["random", "ties", "constant"])
def test_restatement_gives_scikit_learns_bits(kind):
    pytest.importorskip("sklearn")
    from sklearn.preprocessing import QuantileTransformer
    import warnings
    rng = np.random.default_rng(7)
    for n in sr.FIT_SIZES:
        x = rng.gamma(2.0, 0.5, n).astype(np.float32)
        x = {"random": x, "ties": (np.round(x * 4) / 4).astype(np.float32), "constant": np.full(n, x[0], np.float32)}[kind]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")      # n_quantiles is greater than the number of samples
            qt = QuantileTransformer(output_distribution="uniform").fit(x.reshape(-1, 1))
        quantiles, references = sr.fit_quantiles(x)
        assert np.array_equal(bits(quantiles), bits(qt.quantiles_[:, 0])) and np.array_equal(bits(references), bits(qt.references_)), n
        queries = np.concatenate([x[:100], rng.gamma(2.0, 0.5, 100).astype(np.float32), np.asarray([0, -1, 1e9, np.nan], np.float32)])
        assert np.array_equal(bits(sr.transform(queries, quantiles, references)), bits(qt.transform(queries.reshape(-1, 1))[:, 0])), n


@pytest.mark.parametrize("n", [10_001, 32_707])
def test_restatement_draws_scikit_learns_subsample(n):
    pytest.importorskip("sklearn")
    from sklearn.preprocessing import QuantileTransformer
    x = np.random.default_rng(n).gamma(2.0, 0.5, n).astype(np.float32)
    np.random.seed(123)
    qt = QuantileTransformer(output_distribution="uniform").fit(x.reshape(-1, 1))
    np.random.seed(123)
    quantiles, _ = sr.fit_quantiles(x)
    assert np.array_equal(bits(quantiles), bits(qt.quantiles_[:, 0]))
    state = np.random.get_state()[1].copy()
    sr.fit_quantiles(x, subsample=None)      # draws nothing
    assert np.array_equal(np.random.get_state()[1], state)


def test_the_abi_is_the_librarys_own_header(lib):
    names = ["mi_scale_quantile_fit", "mi_scale_gate_forward", "mi_scale_gate_backward"]
    # a public header like every other: _lib binds what it declares, and the module keeps no binder of its own
    assert _lib.DECLARED["mi_scale_gate.h"] == names and [n for n in _lib.ALL_EXPORTS if n.startswith("mi_scale_")] == names
    assert {n: v for n, v in _lib.CONSTANTS.items() if n.startswith("MI_SCALE_")} == {
        "MI_SCALE_MAX_QUANTILES": 1024, "MI_SCALE_MAX_CHANNELS": 256, "MI_SCALE_GATE_NONE": 0, "MI_SCALE_GATE_LEARNED": 1, "MI_SCALE_GATE_FIXED": 2}
    assert (sg.MAX_QUANTILES, sg.MAX_CHANNELS) == (1024, 256) and (sg._NONE, sg._LEARNED, sg._FIXED) == (0, 1, 2)
    header = [h for h in build.HEADERS if os.path.basename(h) == "mi_scale_gate.h"]
    assert len(header) == 1 and "mi_scale_gate.h" not in build.SOURCES and not [s for s in build.SOURCES if s.startswith("mi_") and s.endswith(".h")]
    assert not [n for n in ("load", "FUNCTIONS", "HEADER", "CONSTANTS", "_bound") if hasattr(sg, n)]
    for name in names:
        fn, (restype, argtypes) = getattr(lib, name), _lib.SIGNATURES[name]
        assert C.cast(fn, C.c_void_p).value and fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert lib.mi_scale_quantile_fit.argtypes == [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.mi_scale_gate_forward.argtypes == [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                  C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.mi_scale_gate_backward.argtypes == [C.c_int, C.c_int] + [C.c_void_p] * 7
    sources = {f: open(os.path.join(build.SRC_DIR, f)).read() for f in build.SOURCES}
    assert {"scale_gate.h", "mi_scale_gate.hip"} <= set(sources)
    assert [f for f, text in sources.items() if 'include/mi_scale_gate.h"' in text] == ["mi_scale_gate.hip"]
    assert [f for f, text in sources.items() if '"scale_gate.h"' in text] == ["mi_scale_gate.hip"]
    # what makes the arithmetic reproducible is a build flag, and the kernels say so
    assert "-ffp-contract=off" in build.HIPCC_FLAGS and "-ffp-contract=off" in sources["scale_gate.h"]
    assert "__expf" not in sources["scale_gate.h"] and "atomic" not in sources["scale_gate.h"].replace("no atomics", "")


def test_python_arguments_refused_before_the_library_is_loaded(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    x, w, b = torch.rand(10), torch.rand(32, 1), torch.rand(32)
    sq = object.__new__(sg.ScaleQuantile)      # a table needs a GPU; none of these calls gets as far as reading it
    with pytest.raises(ValueError, match="ScaleQuantile.fit: scales must be a float32 tensor, got torch.float64"):
        sg.ScaleQuantile.fit(x.double())
    with pytest.raises(ValueError, match=r"ScaleQuantile.fit: scales must be on a GPU, got cpu \(there is no CPU fallback\)"):
        sg.ScaleQuantile.fit(x)
    with pytest.raises(ValueError, match=r"ScaleQuantile.fit: n_quantiles must be 1 to 1024 \(MI_SCALE_MAX_QUANTILES\), got 1025"):
        sg.ScaleQuantile.fit(x, n_quantiles=1025)
    with pytest.raises(ValueError, match="ScaleQuantile.fit: n_quantiles must be 1 to 1024"):
        sg.ScaleQuantile.fit(x, n_quantiles=0)
    with pytest.raises(ValueError, match=r"ScaleQuantile.fit: n_quantiles \(1000\) is greater than subsample \(999\)"):
        sg.ScaleQuantile.fit(x, subsample=999)
    with pytest.raises(ValueError, match="ScaleQuantile.fit: scales is empty"):
        sg.ScaleQuantile.fit(x[:0])
    with pytest.raises(ValueError, match="ScaleQuantile.transform: scales must be a float32 tensor, got torch.float64"):
        sq.transform(x.double())
    with pytest.raises(ValueError, match="ScaleQuantile.transform: scales must be on a GPU, got cpu"):
        sq.transform(x)
    with pytest.raises(ValueError, match="ScaleQuantile: quantiles must be a float64"):
        sg.ScaleQuantile(torch.zeros(4), torch.zeros(4))
    with pytest.raises(ValueError, match="ScaleQuantile: quantiles must be on a GPU, got cpu"):
        sg.ScaleQuantile(torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64))
    for distribution in ("normal", None):
        with pytest.raises(ValueError, match='get_quantile_func: only output_distribution "uniform" is implemented'):
            sg.get_quantile_func(x) if distribution is None else sg.get_quantile_func(x, distribution)
    with pytest.raises(ValueError, match="get_quantile_func: scales must be a float32 tensor, got torch.float64"):
        sg.get_quantile_func(x.double(), "uniform")
    with pytest.raises(ValueError, match="scale_gates: scales must be a float32 tensor, got torch.float64"):
        sg.scale_gates(x.double(), sq, w, b)
    with pytest.raises(ValueError, match="scale_gates: scales must be on a GPU, got cpu"):
        sg.scale_gates(x, sq, w, b)
    with pytest.raises(ValueError, match="scale_gates: 257 channels, need 1 to 256"):
        sg.scale_gates(x, sq, torch.rand(257, 1), torch.rand(257))
    with pytest.raises(ValueError, match=r"scale_gates: weight must be \(C, 1\) or \(C,\) and bias \(C,\), got \(32, 2\) and \(32,\)"):
        sg.scale_gates(x, sq, torch.rand(32, 2), b)
    with pytest.raises(ValueError, match="scale_gates: bias must be a float32 tensor"):
        sg.scale_gates(x, sq, w, b.double())
    with pytest.raises(ValueError, match="scale_gates: sq must be a ScaleQuantile"):
        sg.scale_gates(x, None, w, b)
    for dim in (0, 32):
        with pytest.raises(ValueError, match=f"fixed_scale_gates: need 1 <= scale_aware_dim < channels = 32, got {dim}"):
            sg.fixed_scale_gates(x, sq, dim)
    with pytest.raises(ValueError, match="fixed_scale_gates: need 1 <= scale_aware_dim < channels = 8, got 8"):
        sg.fixed_scale_gates(x, sq, 8, channels=8)
    with pytest.raises(ValueError, match="fixed_scale_gates: 257 channels, need 1 to 256"):
        sg.fixed_scale_gates(x, sq, 10, channels=257)
    with pytest.raises(ValueError, match="fixed_scale_gates: scales must be a float32 tensor, got torch.float64"):
        sg.fixed_scale_gates(x.double(), sq, 10)
    with pytest.raises(ValueError, match="fixed_scale_gates: scales must be on a GPU, got cpu"):
        sg.fixed_scale_gates(x, sq, 10)


def test_entry_points_refuse_before_any_hip_call(lib):
    def refused(fn, args, msg):
        assert fn(*args.values()) != 0 and _lib.last_error() == "scale gate: " + msg, _lib.last_error()

    MB = 1 << 20
    fit = dict(n=100, s=1 * MB, nq=100, references=2 * MB, quantiles=3 * MB, stream=None)
    refused(lib.mi_scale_quantile_fit, dict(fit, n=0), "need 1 <= n < 2^30 scales")
    refused(lib.mi_scale_quantile_fit, dict(fit, n=1 << 30), "need 1 <= n < 2^30 scales")
    refused(lib.mi_scale_quantile_fit, dict(fit, nq=0), "need 1 <= nq <= 1024 quantiles")
    refused(lib.mi_scale_quantile_fit, dict(fit, nq=1025), "need 1 <= nq <= 1024 quantiles")
    for name in ("s", "references", "quantiles"):
        refused(lib.mi_scale_quantile_fit, dict(fit, **{name: None}), "null pointer")
    refused(lib.mi_scale_quantile_fit, dict(fit, quantiles=2 * MB + 8), "an output overlaps another tensor of the call")
    fwd = dict(n=100, scales=1 * MB, nq=100, quantiles=2 * MB, references=3 * MB, mode=_lib.MI_SCALE_GATE_LEARNED, channels=32,
               weight=4 * MB, bias=5 * MB, dim=0, u=6 * MB, gates=7 * MB, stream=None)
    refused(lib.mi_scale_gate_forward, dict(fwd, n=0), "need 1 <= n < 2^30 scales")
    refused(lib.mi_scale_gate_forward, dict(fwd, nq=1025), "need 1 <= nq <= 1024 quantiles")
    refused(lib.mi_scale_gate_forward, dict(fwd, mode=3), "unknown gate mode")
    refused(lib.mi_scale_gate_forward, dict(fwd, mode=-1), "unknown gate mode")
    refused(lib.mi_scale_gate_forward, dict(fwd, channels=0), "need 1 <= channels <= 256")
    refused(lib.mi_scale_gate_forward, dict(fwd, channels=257), "need 1 <= channels <= 256")
    for name in ("scales", "quantiles", "references", "weight", "bias", "gates"):
        refused(lib.mi_scale_gate_forward, dict(fwd, **{name: None}), "null pointer")
    refused(lib.mi_scale_gate_forward, dict(fwd, mode=0, u=None), "null pointer")      # the transform alone has u to write
    refused(lib.mi_scale_gate_forward, dict(fwd, gates=6 * MB + 4), "an output overlaps another tensor of the call")
    refused(lib.mi_scale_gate_forward, dict(fwd, u=1 * MB), "an output overlaps another tensor of the call")
    for dim in (0, 32):
        refused(lib.mi_scale_gate_forward, dict(fwd, mode=2, dim=dim), "need 1 <= scale_aware_dim < channels")
    bwd = dict(n=100, channels=32, u=1 * MB, weight=2 * MB, bias=3 * MB, d_gates=4 * MB, d_weight=5 * MB, d_bias=6 * MB, stream=None)
    refused(lib.mi_scale_gate_backward, dict(bwd, n=0), "need 1 <= n < 2^30 scales")
    refused(lib.mi_scale_gate_backward, dict(bwd, channels=257), "need 1 <= channels <= 256")
    for name in ("u", "weight", "bias", "d_gates", "d_weight", "d_bias"):
        refused(lib.mi_scale_gate_backward, dict(bwd, **{name: None}), "null pointer")
    refused(lib.mi_scale_gate_backward, dict(bwd, d_bias=5 * MB + 64), "an output overlaps another tensor of the call")
