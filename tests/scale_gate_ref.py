"""Scale conditioning (seganygaussians_amd/scale_gate.py) restated in elementwise numpy and Python: what
scikit-learn's QuantileTransformer(output_distribution="uniform") computes in fit and transform, operation by operation, the gates
in float64, and the loader of the golden fixture (tests/golden/scale_gate/scale_gate.npz, written by
tests/golden/make_scale_gate_golden.py from scikit-learn itself).  No call of np.nanpercentile or np.interp: those two are what is
being pinned, and the numpy of a machine that runs these tests need not be the one that wrote the fixture.  Runs anywhere."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scale_gate", "scale_gate.npz")
CASES = ("gamma", "ties", "constant", "n1", "n2", "n3", "nan7", "subsample")
SUBSAMPLE_SEED = 123
FIT_SIZES = (1, 2, 3, 7, 64, 999, 1000, 1001, 2500, 10_000)


def n_quantiles_of(N, n_quantiles=1000):
    return max(1, min(int(n_quantiles), int(N)))


def subsample_rows(N, subsample):
    """The rows scikit-learn fits on: None for all of them, else the first `subsample` of arange(N) shuffled by the GLOBAL numpy
    RandomState (sklearn.utils.resample(replace=False) with random_state=None)."""
    if subsample is None or subsample >= N:
        return None
    idx = np.arange(N)
    np.random.mtrand._rand.shuffle(idx)
    return idx[:subsample]


def fit_quantiles(data, n_quantiles=1000, subsample=10_000):
    """(quantiles float64 [nq], references float64 [nq]) of float32 data of any shape; NaNs are ignored as np.nanpercentile does."""
    data = np.asarray(data, np.float32).reshape(-1)
    N = data.size
    references = np.linspace(0, 1, n_quantiles_of(N, n_quantiles))
    rows = subsample_rows(N, subsample)
    if rows is not None:
        data = data[rows]
    s = np.sort(data)                               # NaN last
    m = int(np.count_nonzero(s == s))
    if m == 0:
        return np.full(references.shape, np.nan), references
    q = (references * 100.0) / 100.0                # fit passes references * 100, percentile divides by 100
    v = (m - 1) * q
    floor = np.floor(v)
    g = v - floor
    lo = floor.astype(np.int64)
    hi = np.minimum(lo + 1, m - 1)
    a, b = s[lo], s[hi]
    d = b - a                                       # float32: numpy's _lerp subtracts in the array's type
    assert d.dtype == np.float32
    a64, b64, d64 = a.astype(np.float64), b.astype(np.float64), d.astype(np.float64)
    with np.errstate(all="ignore"):
        out = np.where(g >= 0.5, b64 - d64 * (1 - g), a64 + d64 * g)
    out = np.where(d == 0, a64, out)
    for i in range(1, out.size):                    # np.maximum.accumulate
        if not out[i] >= out[i - 1] and out[i] == out[i]:
            out[i] = out[i - 1]
    return out, references


def _interp(x, xp, fp):
    """numpy's compiled interp for finite-or-infinite x (no NaN) on ascending xp, all float64; each operation rounds once."""
    n = xp.size
    j = np.clip(np.searchsorted(xp, x, side="right") - 1, 0, n - 1)       # the largest j with xp[j] <= x
    up = np.minimum(j + 1, n - 1)
    with np.errstate(all="ignore"):
        slope = (fp[up] - fp[j]) / (xp[up] - xp[j])
        y = slope * (x - xp[j]) + fp[j]
    y = np.where((j == n - 1) | (xp[j] == x), fp[j], y)
    y = np.where(x > xp[-1], fp[-1], y)
    return np.where(x < xp[0], fp[0], y)


def transform(x, quantiles, references):
    """float32 in, float32 out, the same shape."""
    x = np.asarray(x, np.float32)
    X = x.reshape(-1).astype(np.float64)
    Q, R = np.asarray(quantiles, np.float64), np.asarray(references, np.float64)
    ok = X == X
    out = np.full(X.shape, np.nan, np.float32)
    xf = X[ok]
    y = 0.5 * (_interp(xf, Q, R) - _interp(-xf, -Q[::-1], -R[::-1]))
    out[ok] = y.astype(np.float32)
    out[X == Q[-1]] = 1
    out[X == Q[0]] = 0
    return out.reshape(x.shape)


def gates_f64(u, weight, bias):
    """sigmoid(w u + b) in float64 from float32 operands: (n, C)."""
    z = np.asarray(u, np.float64).reshape(-1, 1) * np.asarray(weight, np.float64).reshape(1, -1) + np.asarray(bias, np.float64).reshape(1, -1)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-z))


def load_cases(path=GOLDEN):
    """{case: {"data" f32, "quantiles" f64, "references" f64, "queries" f32, "outputs" f32}}, and the versions that wrote them."""
    z = np.load(path)
    cases = {name: {k: z[f"{name}/{k}"] for k in ("data", "quantiles", "references", "queries", "outputs")} for name in CASES}
    return cases, {"sklearn": str(z["sklearn_version"]), "numpy": str(z["numpy_version"]), "seed": int(z["subsample_seed"])}
