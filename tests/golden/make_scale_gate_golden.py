"""Writes tests/golden/scale_gate/scale_gate.npz: what scikit-learn's QuantileTransformer(output_distribution="uniform") -- the
reference's q_trans (train_contrastive_feature.py:42-62) -- fits and returns on float32 mask scales, for
tests/test_scale_gate_host.py (the restatement of tests/scale_gate_ref.py) and tests/test_scale_gate.py (the kernels).

Run where scikit-learn is installed; not part of the tests:

    python tests/golden/make_scale_gate_golden.py [--out <file>]

Fit cases (float32 columns, as the reference passes them): gamma-distributed n = 2500; n = 300 rounded to 1/8 (ties, nq = 300);
constant n = 64; n = 1, 2, 3; n = 500 with every 7th value NaN (nq = 500, 428 values); n = 10 001 under np.random.seed(123), the
one case in which scikit-learn subsamples (10 000 rows drawn from the global RandomState).  Queries per case: the first 200 fit
points, 200 fresh draws, 0, -1, 1e9, Q[0], Q[-1], the float32 neighbours of both, NaN and the infinities.  Stored per case: the fit
data, quantiles_, references_, the queries and scikit-learn's float32 outputs; and the versions of scikit-learn and numpy.  The
outputs are those of the transformer's column routine, which transform() calls: transform() itself refuses an infinite input, and
is asserted to give the same bits on every other query.
Asserted here: tests/scale_gate_ref.py gives the same bits, tables and outputs."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import scale_gate_ref as sr  # noqa: E402


def fit_data(rng):
    nan7 = rng.gamma(2.0, 0.5, 500).astype(np.float32)
    nan7[::7] = np.nan
    return {"gamma": rng.gamma(2.0, 0.5, 2500).astype(np.float32),
            "ties": (np.round(rng.gamma(2.0, 0.5, 300) * 8) / 8).astype(np.float32),
            "constant": np.full(64, 0.75, np.float32),
            "n1": rng.gamma(2.0, 0.5, 1).astype(np.float32),
            "n2": rng.gamma(2.0, 0.5, 2).astype(np.float32),
            "n3": rng.gamma(2.0, 0.5, 3).astype(np.float32),
            "nan7": nan7,
            "subsample": rng.gamma(2.0, 0.5, 10_001).astype(np.float32)}


def queries_of(data, quantiles, rng):
    q0, q1 = np.float32(quantiles[0]), np.float32(quantiles[-1])
    assert q0 == quantiles[0] and q1 == quantiles[-1]      # the ends of the table are data values
    inf = np.float32(np.inf)
    return np.concatenate([data[:200], rng.gamma(2.0, 0.5, 200).astype(np.float32),
                           np.asarray([0, -1, 1e9, q0, q1, np.nextafter(q0, inf), np.nextafter(q0, -inf), np.nextafter(q1, inf),
                                       np.nextafter(q1, -inf), np.nan, inf, -inf], np.float32)])


def main():
    import sklearn
    from sklearn.preprocessing import QuantileTransformer
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=sr.GOLDEN)
    args = ap.parse_args()
    rng = np.random.default_rng(20271)
    out = {"sklearn_version": np.asarray(sklearn.__version__), "numpy_version": np.asarray(np.__version__),
           "subsample_seed": np.asarray(sr.SUBSAMPLE_SEED, np.int64)}
    data = fit_data(rng)
    assert tuple(data) == sr.CASES
    for name, x in data.items():
        if name == "subsample":
            np.random.seed(sr.SUBSAMPLE_SEED)
        qt = QuantileTransformer(output_distribution="uniform").fit(x.reshape(-1, 1))
        quantiles, references = qt.quantiles_[:, 0], qt.references_
        assert quantiles.dtype == np.float64 and references.dtype == np.float64 and qt.n_quantiles_ == sr.n_quantiles_of(x.size)
        queries = queries_of(x, quantiles, rng)
        # transform() refuses an infinite input at its door (check_array), so the whole set goes through the column routine behind
        # it -- scikit-learn's own arithmetic, which is what the rule for the infinities restates -- and the public call confirms
        # every other query
        outputs = qt._transform_col(queries.copy(), quantiles, False)
        finite = ~np.isinf(queries)
        public = qt.transform(queries[finite].reshape(-1, 1))[:, 0]
        assert outputs.dtype == np.float32 and public.dtype == np.float32
        assert np.array_equal(public.view(np.int32), outputs[finite].view(np.int32)), name
        assert np.array_equal(outputs[~finite], [references[-1], 0])      # 1 and 0; with one quantile the only reference is 0
        if name == "subsample":
            np.random.seed(sr.SUBSAMPLE_SEED)
        mine, refs = sr.fit_quantiles(x)
        assert np.array_equal(mine.view(np.int64), quantiles.view(np.int64)) and np.array_equal(refs.view(np.int64), references.view(np.int64)), name
        assert np.array_equal(sr.transform(queries, quantiles, references).view(np.int32), outputs.view(np.int32)), name
        for key, value in (("data", x), ("quantiles", quantiles), ("references", references), ("queries", queries), ("outputs", outputs)):
            out[f"{name}/{key}"] = value
        print(f"{name:10s} n {x.size:6d} nq {quantiles.size:5d} queries {queries.size}")
    assert out["ties/quantiles"].size == 300 and out["nan7/quantiles"].size == 500 and int(np.count_nonzero(~np.isnan(data["nan7"]))) == 428
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **out)
    cases, versions = sr.load_cases(args.out)
    assert set(cases) == set(sr.CASES) and versions["seed"] == sr.SUBSAMPLE_SEED
    print(args.out, os.path.getsize(args.out), "bytes;", versions)


if __name__ == "__main__":
    main()
