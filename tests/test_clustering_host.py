"""CPU checks of the HDBSCAN* clustering: the numpy restatement (tests/hdbscan_ref.py) against scikit-learn,
its invariance under the order of equal edges for exactly the inputs the GPU tests use, the product's host C++ (labels_from_mst)
against the restatement, the argument checks of seganygaussians_amd/clustering.py before any launch, install_dropin, the exports and
the workspace size.  No GPU.

Figures behind the scikit-learn comparison (scikit-learn 1.7.2, the 20 euclidean configurations x seeds below): the mutual-
reachability tree has many edges of equal weight (every edge from a point to a nearer neighbour weighs that point's core distance),
scikit-learn builds a BINARY merge tree in the order its sort leaves equal edges in, and a point that joins a cluster at the very
weight at which that cluster splits off is a member or noise depending on that order.  scikit-learn's own partition changed under
a permutation of the rows in 2 of 4 permutations tried on (300, 32, 4, 10, 0.01) seed 2.  The restatement and the product treat all
edges of one weight as one level, which does not depend on any order; against scikit-learn that leaves 0-3 points per case (in 15 of
the 20 cases at least one), every one of them a point the restatement marks as `border`, noise here and a member there.  So the
comparison below demands an equal partition everywhere else, and of every disagreement that it is such a point."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import seganygaussians_amd
from seganygaussians_amd import _lib, build
from seganygaussians_amd import clustering as cl
from tests import hdbscan_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 1, 2, 3)
EUCLID_IDS = [f"n{c[0]}-C{c[1]}-k{c[2]}-mcs{c[3]}-eps{c[4]}" for c in ref.EUCLID_CONFIGS]
JACCARD_IDS = [f"n{c[0]}-k{c[1]}-mcs{c[2]}-eps{c[3]}" for c in ref.JACCARD_CONFIGS]


def product_labels(n, a, b, w, mcs, eps=0.0, single=False):
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(dt)))
    return cl.labels_from_mst(t(a, np.int32), t(b, np.int32), t(w, np.float32), n, mcs, eps, single).numpy()


# ---- the restatement against scikit-learn ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ref.EUCLID_CONFIGS, ids=EUCLID_IDS)
def test_restatement_matches_sklearn(config):
    sk = pytest.importorskip("sklearn.cluster")
    n, C, k, mcs, eps = config
    for seed in SEEDS:
        pts, tree, lab = ref.planted_case("euclidean", config, seed)
        border = np.zeros(n, bool)
        again = ref.labels_from_mst(n, *tree[:3], mcs, eps, border=border)
        assert np.array_equal(again, lab)
        assert lab.max() + 1 == k and 0.10 <= (lab < 0).mean() <= 0.16
        theirs = [sk.HDBSCAN(min_cluster_size=mcs, cluster_selection_epsilon=eps, metric="precomputed",
                             allow_single_cluster=False).fit_predict(tree[4].copy()),
                  sk.HDBSCAN(min_cluster_size=mcs, cluster_selection_epsilon=eps, algorithm="brute",
                             allow_single_cluster=False).fit_predict(pts.astype(np.float64))]
        for other in theirs:
            differ = (lab < 0) != (other < 0)
            print(config, seed, "points that differ:", int(differ.sum()), "border points:", int(border.sum()))
            assert ref.same_partition(lab[~border], other[~border])      # equal partition wherever the order of equal edges has no say
            assert (border & (lab < 0))[differ].all()                    # the rest: noise here, a member there, and only at a split level
            assert differ.sum() <= 4 and other.max() + 1 == k


# ---- the order of equal edges does not matter ------------------------------------------------------------------------------------
def _tie_cases():
    return [("euclidean", c, s) for c in ref.EUCLID_CONFIGS for s in ref.GPU_SEEDS] + \
           [("jaccard", c, s) for c in ref.JACCARD_CONFIGS for s in ref.GPU_SEEDS]


@pytest.mark.parametrize("case", _tie_cases(), ids=lambda c: f"{c[0]}-{'-'.join(str(v) for v in c[1])}-s{c[2]}")
def test_restatement_is_tie_order_invariant(case):
    """For every (configuration, seed) of the GPU tests, both metrics: 8 random orders of the equal edges give the same partition.
    No seed had to be replaced (jaccard seeds 0-3 of both configurations pass)."""
    metric, config, seed = case
    pts, tree, lab = ref.planted_case(metric, config, seed)
    mcs, eps = config[-2], config[-1]
    assert lab.max() >= 1                                        # a structure to lose
    assert len(np.unique(tree[2])) < len(tree[2])                # and equal weights to shuffle
    for draw in range(8):
        got = ref.labels(pts, metric, mcs, epsilon=eps, tie_rng=np.random.default_rng(1000 + draw), tree=tree)
        assert ref.same_partition(got, lab), draw


# ---- the product's host C++ ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,config", [("euclidean", c) for c in ref.EUCLID_CONFIGS] + [("jaccard", c) for c in ref.JACCARD_CONFIGS],
                         ids=EUCLID_IDS + JACCARD_IDS)
def test_labels_from_mst_matches_restatement(metric, config):
    mcs, eps = config[-2], config[-1]
    for seed in SEEDS:
        pts, tree, lab = ref.planted_case(metric, config, seed)
        n = len(pts)
        a, b, w = tree[:3]
        got = product_labels(n, a, b, w, mcs, eps)
        assert ref.same_partition(got, lab)
        perm = np.random.default_rng(seed).permutation(n - 1)
        flip = np.random.default_rng(seed + 1).random(n - 1) < 0.5
        a2, b2 = np.where(flip, b, a)[perm], np.where(flip, a, b)[perm]
        assert np.array_equal(product_labels(n, a2, b2, w[perm], mcs, eps), got)     # edge order and direction: the same labels
        # numbered by smallest member
        firsts = [int(np.flatnonzero(got == c)[0]) for c in range(got.max() + 1)]
        assert firsts == sorted(firsts) and set(np.unique(got)) <= set(range(-1, got.max() + 1))


def test_labels_from_mst_small_and_degenerate():
    e = lambda *v: torch.tensor(v, dtype=torch.int32)
    w = lambda *v: torch.tensor(v, dtype=torch.float32)
    assert cl.labels_from_mst(e(), e(), w(), 1, 2).tolist() == [-1]
    assert cl.labels_from_mst(e(0), e(1), w(0.5), 2, 2).tolist() == [-1, -1]
    assert cl.labels_from_mst(e(0), e(1), w(0.5), 2, 2, allow_single_cluster=True).tolist() == ref.labels_from_mst(
        2, [0], [1], [0.5], 2, allow_single_cluster=True).tolist()
    # n < min_cluster_size: all noise, whatever else is asked
    a, b, ww = e(0, 1, 2), e(1, 2, 3), w(0.1, 0.2, 0.3)
    assert cl.labels_from_mst(a, b, ww, 4, 5).tolist() == [-1] * 4
    assert cl.labels_from_mst(a, b, ww, 4, 5, 0.0, True).tolist() == [-1] * 4
    # two tight groups of 3, mcs = 3; the cluster that holds point 0 is number 0 whichever way the edges come
    pts = np.array([[0.0], [10.0], [0.1], [10.1], [0.2], [10.2]], np.float32)
    a, b, ww, _, _ = ref.mst(pts, "euclidean", 2)
    want = ref.labels_from_mst(6, a, b, ww, 3)
    assert want.tolist() == [0, 1, 0, 1, 0, 1]
    assert product_labels(6, a, b, ww, 3).tolist() == want.tolist()
    assert product_labels(6, b[::-1], a[::-1], ww[::-1], 3).tolist() == want.tolist()


@pytest.mark.parametrize("seed", [0, 1])
def test_labels_from_mst_without_structure(seed):
    """Uniform random rows: all noise without allow_single_cluster, one cluster with it -- as the restatement says."""
    pts = np.random.default_rng(seed).random((400, 8)).astype(np.float32)
    a, b, w, _, _ = ref.mst(pts, "euclidean", 10)
    none, one = ref.labels_from_mst(400, a, b, w, 10), ref.labels_from_mst(400, a, b, w, 10, allow_single_cluster=True)
    assert (none == -1).all() and set(np.unique(one)) <= {-1, 0} and (one == 0).sum() >= 10
    assert np.array_equal(product_labels(400, a, b, w, 10), none)
    assert np.array_equal(product_labels(400, a, b, w, 10, single=True), one)
    one_eps = ref.labels_from_mst(400, a, b, w, 10, epsilon=0.3, allow_single_cluster=True)
    assert np.array_equal(product_labels(400, a, b, w, 10, eps=0.3, single=True), one_eps)
    assert set(np.unique(one_eps)) <= {-1, 0}


def test_labels_from_mst_epsilon_merges_upwards():
    """epsilon = 0 against an epsilon above every split below the root: the clusters below each child of the root become one."""
    pts, tree, lab = ref.planted_case("euclidean", ref.EUCLID_CONFIGS[1], 0)
    n = len(pts)
    a, b, w = tree[:3]
    fine, coarse = product_labels(n, a, b, w, 10, 0.0), product_labels(n, a, b, w, 10, 10.0)
    assert ref.same_partition(fine, ref.labels_from_mst(n, a, b, w, 10, 0.0))
    assert ref.same_partition(coarse, ref.labels_from_mst(n, a, b, w, 10, 10.0))
    assert 2 <= coarse.max() + 1 < fine.max() + 1
    for c in range(fine.max() + 1):                              # every fine cluster lies inside one coarse cluster
        assert len(set(coarse[fine == c].tolist())) == 1 and coarse[fine == c][0] >= 0
    assert ((coarse >= 0) | (fine < 0)).all()


def test_labels_from_mst_refuses_what_is_not_a_tree():
    e = lambda *v: torch.tensor(v, dtype=torch.int32)
    w = lambda *v: torch.tensor(v, dtype=torch.float32)
    with pytest.raises(ValueError, match="n - 1 edges"):
        cl.labels_from_mst(e(0, 1), e(1, 2), w(1, 1), 4, 2)                  # n - 2 edges
    with pytest.raises(ValueError, match="out of range"):
        cl.labels_from_mst(e(0, 1, 2), e(1, 2, 4), w(1, 1, 1), 4, 2)          # an index >= n
    with pytest.raises(ValueError, match="out of range"):
        cl.labels_from_mst(e(0, 1, -1), e(1, 2, 3), w(1, 1, 1), 4, 2)
    with pytest.raises(ValueError, match="cycle"):
        cl.labels_from_mst(e(0, 1, 2), e(1, 2, 0), w(1, 1, 1), 4, 2)          # a cycle (and point 3 left out)
    with pytest.raises(ValueError, match="cycle"):
        cl.labels_from_mst(e(0, 1, 1), e(1, 2, 1), w(1, 1, 1), 4, 2)          # a loop
    with pytest.raises(ValueError, match="finite"):
        cl.labels_from_mst(e(0, 1, 2), e(1, 2, 3), w(1, float("nan"), 1), 4, 2)
    with pytest.raises(ValueError, match="finite"):
        cl.labels_from_mst(e(0, 1, 2), e(1, 2, 3), w(1, -1, 1), 4, 2)


# ---- argument checks before any launch -------------------------------------------------------------------------------------------
def test_bad_inputs_refused_before_any_launch():
    p = torch.zeros(20, 8)
    bits = torch.zeros(20, 4, dtype=torch.int32)
    device_calls = (lambda x, k=2, **kw: cl.core_distances(x, k, **kw), lambda x, k=2, **kw: cl.mutual_reachability_mst(x, k, **kw),
                    lambda x, k=2, **kw: cl.hdbscan_labels(x, 5, core_k=k, **kw))
    for fn in device_calls:
        with pytest.raises(ValueError, match="GPU"):
            fn(p)                                                            # a CPU tensor
        with pytest.raises(ValueError, match="GPU"):
            fn(bits, metric="jaccard")
        with pytest.raises(ValueError, match="float32"):
            fn(p.double())
        with pytest.raises(ValueError, match="float32"):
            fn(p.numpy())
        with pytest.raises(ValueError, match="int32"):
            fn(p, metric="jaccard")
        with pytest.raises(ValueError, match=r"\(n, width\)"):
            fn(torch.zeros(20))
        with pytest.raises(ValueError, match="256"):
            fn(torch.zeros(20, 257))
        with pytest.raises(ValueError, match="1024"):
            fn(torch.zeros(20, 1025, dtype=torch.int32), metric="jaccard")
        with pytest.raises(ValueError, match="width"):
            fn(torch.zeros(20, 0))
        with pytest.raises(ValueError, match="points"):
            fn(torch.zeros(0, 8))
        with pytest.raises(ValueError, match="metric"):
            fn(p, metric="precomputed")
        with pytest.raises(ValueError, match="core_k"):
            fn(p, 0)
        with pytest.raises(ValueError, match="core_k"):
            fn(torch.zeros(100, 8), 65)
        with pytest.raises(ValueError, match="core_k"):
            fn(p, 2.0)
        with pytest.raises(ValueError, match="n >= core_k"):
            fn(p, 21)
        with pytest.raises(ValueError, match="requires grad"):
            fn(p.clone().requires_grad_())
        with torch.no_grad(), pytest.raises(ValueError, match="GPU"):
            fn(p.clone().requires_grad_())
    with pytest.raises(ValueError, match="min_cluster_size"):
        cl.hdbscan_labels(p, 1)
    with pytest.raises(ValueError, match="core_k"):
        cl.hdbscan_labels(p, 5, min_samples=0)
    e, w = torch.zeros(3, dtype=torch.int32), torch.zeros(3)
    with pytest.raises(ValueError, match="min_cluster_size"):
        cl.labels_from_mst(e, e, w, 4, 1)
    with pytest.raises(ValueError, match="epsilon"):
        cl.labels_from_mst(e, e, w, 4, 2, -0.1)
    with pytest.raises(ValueError, match="epsilon"):
        cl.labels_from_mst(e, e, w, 4, 2, float("nan"))
    with pytest.raises(ValueError, match="int32"):
        cl.labels_from_mst(e.long(), e, w, 4, 2)
    with pytest.raises(ValueError, match="float32"):
        cl.labels_from_mst(e, e, w.double(), 4, 2)
    with pytest.raises(ValueError, match="one entry per edge"):
        cl.labels_from_mst(e, e[:2], w, 4, 2)
    with pytest.raises(ValueError, match="points"):
        cl.labels_from_mst(e, e, w, 0, 2)
    with pytest.raises(ValueError, match="integer"):
        cl.labels_from_mst(e, e, w, 4.0, 2)
    with pytest.raises(ValueError, match="bool or integer"):
        cl.pack_bits(torch.zeros(3, 40))
    with pytest.raises(ValueError, match="bits"):
        cl.pack_bits(torch.zeros(3, 32 * 1024 + 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="labels"):
        cl.cluster_centers(p, torch.zeros(20, dtype=torch.int32))
    with pytest.raises(ValueError, match="features"):
        cl.cluster_centers(torch.zeros(20), torch.zeros(20, dtype=torch.int64))
    with pytest.raises(ValueError, match="hdbscan_labels"):
        cl.HDBSCAN(min_cluster_size=10, metric="precomputed")
    with pytest.raises(ValueError, match="jaccard"):
        cl.HDBSCAN(min_cluster_size=10, metric="jaccard")
    with pytest.raises(TypeError, match="unsupported"):
        cl.HDBSCAN(min_cluster_size=10, leaf_size=40)


def test_pack_bits_and_cluster_centers():
    rng = np.random.default_rng(5)
    for B in (1, 31, 32, 33, 70, 1024):
        bits = rng.random((9, B)) < 0.4
        got = cl.pack_bits(torch.from_numpy(bits)).numpy()
        assert got.dtype == np.int32 and got.shape == (9, (B + 31) // 32)
        assert np.array_equal(got.view(np.uint32), ref.pack_bits(bits))
        assert np.array_equal(ref.unpack_bits(got)[:, :B], bits.astype(np.uint8)) and not ref.unpack_bits(got)[:, B:].any()
    assert np.array_equal(cl.pack_bits(torch.from_numpy(bits.astype(np.int64))).numpy(), got)
    f = torch.tensor([[1.0, 0.0], [3.0, 0.0], [0.0, 2.0], [5.0, 5.0], [0.0, 4.0]])
    lab = torch.tensor([0, 0, 1, -1, 1])
    assert torch.allclose(cl.cluster_centers(f, lab), torch.tensor([[1.0, 0.0], [0.0, 1.0]]))
    assert cl.cluster_centers(f, torch.full((5,), -1)).shape == (0, 2)
    # the GUI's own centre 0 (saga_gui.py:539-540 loops over np.unique, noise first): the line of the docstring
    gui = torch.cat([torch.nn.functional.normalize(f[lab == -1].mean(0, keepdim=True), dim=-1), cl.cluster_centers(f, lab)])
    assert gui.shape == (3, 2) and torch.allclose(gui[0], torch.tensor([0.5, 0.5]).sqrt())


# ---- install_dropin --------------------------------------------------------------------------------------------------------------
def test_install_dropin_adds_hdbscan_only_on_request():
    saved_path, saved_mod = list(sys.path), sys.modules.pop("hdbscan", None)
    try:
        sys.path[:] = [p for p in sys.path if p != seganygaussians_amd.CLUSTERING_DROPIN_DIR]
        seganygaussians_amd.install_dropin()
        assert seganygaussians_amd.CLUSTERING_DROPIN_DIR not in sys.path
        assert not os.path.exists(os.path.join(seganygaussians_amd.DROPIN_DIR, "hdbscan"))
        try:
            import hdbscan
            assert not os.path.abspath(hdbscan.__file__).startswith(ROOT + os.sep)      # an installed package, not ours
            sys.modules.pop("hdbscan", None)
        except ImportError:
            pass
        assert seganygaussians_amd.install_dropin(fuse_clustering=True) == seganygaussians_amd.DROPIN_DIR
        assert sys.path[0] == seganygaussians_amd.CLUSTERING_DROPIN_DIR
        from hdbscan import HDBSCAN
        assert HDBSCAN is cl.HDBSCAN
        assert os.listdir(seganygaussians_amd.CLUSTERING_DROPIN_DIR) in (["hdbscan"], ["hdbscan", "__pycache__"], ["__pycache__", "hdbscan"])
        seganygaussians_amd.install_dropin(fuse_clustering=True)
        assert sys.path.count(seganygaussians_amd.CLUSTERING_DROPIN_DIR) == 1
        h = HDBSCAN(min_cluster_size=10, cluster_selection_epsilon=0.01, allow_single_cluster=False)
        assert (h.min_cluster_size, h.min_samples, h.cluster_selection_epsilon, h.allow_single_cluster, h.labels_) == (10, None, 0.01, False, None)
    finally:
        sys.path[:] = saved_path
        sys.modules.pop("hdbscan", None)
        if saved_mod is not None:
            sys.modules["hdbscan"] = saved_mod


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def test_abi_exported_and_checks_arguments(lib):
    hdr = open(os.path.join(ROOT, "include", "mi_cluster.h")).read()
    declared = set(re.findall(r"\b(mi_cluster_[a-z_0-9]+)\s*\(", hdr))
    assert declared == {"mi_cluster_workspace_bytes", "mi_cluster_core_distances", "mi_cluster_mst", "mi_cluster_mst_rounds",
                        "mi_cluster_labels_host"} <= set(_lib.ALL_EXPORTS)
    assert _lib.DECLARED["mi_cluster.h"] == ["mi_cluster_workspace_bytes", "mi_cluster_core_distances", "mi_cluster_mst", "mi_cluster_mst_rounds",
                                             "mi_cluster_labels_host"]
    for name in declared:
        assert ctypes.cast(getattr(lib, name), ctypes.c_void_p).value
    assert {"cluster.h", "cluster_tree.h", "mi_cluster.hip"} <= set(build.SOURCES)
    includers = [f for f in build.SOURCES if '"cluster.h"' in open(os.path.join(build.SRC_DIR, f)).read()]
    assert includers == ["mi_cluster.hip"]
    for name, value in (("MI_CLUSTER_EUCLIDEAN", 0), ("MI_CLUSTER_JACCARD", 1), ("MI_CLUSTER_MAX_POINTS", "(1 << 20)"),
                        ("MI_CLUSTER_MAX_CHANNELS", 256), ("MI_CLUSTER_MAX_WORDS", 1024), ("MI_CLUSTER_MAX_CORE_K", 64)):
        assert f"#define {name} {value}\n" in hdr
    assert (cl.MAX_POINTS, cl.MAX_CHANNELS, cl.MAX_WORDS, cl.MAX_CORE_K) == (1 << 20, 256, 1024, 64)
    assert (1 << 20, 256, 1024, 64) == tuple(getattr(_lib, "MI_CLUSTER_MAX_" + n) for n in ("POINTS", "CHANNELS", "WORDS", "CORE_K"))
    assert cl.METRICS == _lib.MI_CLUSTER_METRIC == {"euclidean": _lib.MI_CLUSTER_EUCLIDEAN, "jaccard": _lib.MI_CLUSTER_JACCARD}
    # refused for their arguments before any HIP call: the pointers are never read
    ws = lib.mi_cluster_workspace_bytes(0, 100, 32, 10)
    assert lib.mi_cluster_core_distances(2, 100, 32, 8, 10, 8, 8, ws, None) != 0 and "metric" in _lib.last_error()
    assert lib.mi_cluster_core_distances(0, 0, 32, 8, 10, 8, 8, ws, None) != 0 and "2^20" in _lib.last_error()
    assert lib.mi_cluster_core_distances(0, 100, 257, 8, 10, 8, 8, ws, None) != 0 and "256" in _lib.last_error()
    assert lib.mi_cluster_core_distances(1, 100, 1025, 8, 10, 8, 8, ws, None) != 0 and "1024" in _lib.last_error()
    assert lib.mi_cluster_core_distances(0, 100, 32, None, 10, 8, 8, ws, None) != 0 and "null" in _lib.last_error()
    assert lib.mi_cluster_core_distances(0, 100, 32, 8, 10, None, 8, ws, None) != 0 and "null" in _lib.last_error()
    assert lib.mi_cluster_core_distances(0, 100, 32, 8, 65, 8, 8, ws, None) != 0 and "core_k" in _lib.last_error()
    assert lib.mi_cluster_core_distances(0, 100, 32, 8, 101, 8, 8, ws, None) != 0 and "core_k" in _lib.last_error()
    assert lib.mi_cluster_core_distances(0, 100, 32, 8, 10, 8, 8, ws - 1, None) != 0 and "workspace" in _lib.last_error()
    assert lib.mi_cluster_core_distances(0, 100, 32, 6, 10, 8, 8, ws, None) != 0 and "aligned" in _lib.last_error()
    assert lib.mi_cluster_mst(0, 100, 32, 8, None, 8, 8, 8, 8, ws, None) != 0 and "null" in _lib.last_error()
    assert lib.mi_cluster_mst(0, 100, 32, 8, 8, 8, None, 8, 8, ws, None) != 0 and "null" in _lib.last_error()
    assert lib.mi_cluster_mst(0, 100, 32, 8, 8, 8, 8, 8, 8, ws - 1, None) != 0 and "workspace" in _lib.last_error()
    assert lib.mi_cluster_mst(0, 1, 32, 8, 8, None, None, None, 8, 1 << 20, None) == 0 and lib.mi_cluster_mst_rounds() == 0   # n = 1: no edges


def test_workspace_bytes(lib):
    f = lib.mi_cluster_workspace_bytes
    for bad in ((2, 100, 32, 10), (-1, 100, 32, 10), (0, 0, 32, 10), (0, (1 << 20) + 1, 32, 10), (0, 100, 0, 10), (0, 100, 257, 10),
                (1, 100, 1025, 10), (0, 100, 32, 0), (0, 100, 32, 65), (0, 100, 32, 101)):
        assert f(*bad) == 0, bad
    assert f(1, 100, 1024, 64) > 0 and f(0, 1, 1, 1) > 0 and f(0, 1 << 20, 256, 64) > 0
    sizes = [f(0, n, 32, 1) for n in (1, 2, 63, 64, 65, 1000, 51565, 1 << 19, 1 << 20)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    # the layout: ten arrays of n 4-byte words and one of n 8-byte words, plus a counter, each rounded up to 256 bytes -- linear in n
    # whatever the metric, the width and core_k; an n x n buffer of any element size would be 2^40 bytes or more at n = 2^20
    for metric, width, k in ((0, 1, 1), (0, 256, 64), (1, 1024, 64)):
        for n in (1, 1000, 51565, 1 << 20):
            assert 44 * n <= f(metric, n, width, min(k, n)) <= 48 * n + 12 * 256
    assert f(0, 1 << 20, 256, 64) <= 48 * (1 << 20) + 12 * 256 < 1 << 26


def test_module_exports():
    for name in ("core_distances", "mutual_reachability_mst", "labels_from_mst", "hdbscan_labels", "pack_bits", "cluster_centers", "HDBSCAN"):
        assert callable(getattr(cl, name))
    import inspect
    assert list(inspect.signature(cl.hdbscan_labels).parameters) == ["points", "min_cluster_size", "min_samples", "cluster_selection_epsilon",
                                                                      "allow_single_cluster", "metric", "core_k"]
    assert list(inspect.signature(seganygaussians_amd.install_dropin).parameters) == ["fuse_smoothing", "fuse_training_step", "fuse_clustering"]
    assert inspect.signature(seganygaussians_amd.install_dropin).parameters["fuse_clustering"].default is False
