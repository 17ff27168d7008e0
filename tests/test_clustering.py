"""GPU checks of the HDBSCAN* clustering against the numpy float64 restatement (tests/hdbscan_ref.py).

Tile sizes of csrc/cluster.h, which the shapes below straddle: a workgroup owns 64 rows; a column tile has 64 columns at a width of
up to 32 channels (and for jaccard), 32 columns above; a row is held 32 or 64 words at a time (widths 33, 65 and 256 take the chunked
path, 1024 jaccard words take 32 chunks); core_k runs the 16-, 32- or 64-entry list (2 and 10, 30, 64).

The euclidean bound, relative: (C / 2 + 2) 2^-24 -- the subtraction has relative error u = 2^-24, its square 2u (+ u when rounded on
its own), a sum of C terms in sequence adds at most (C - 1) u, the square root halves the total and adds u."""
import numpy as np
import pytest
import torch

from seganygaussians_amd import _lib
from seganygaussians_amd import clustering as cl
from seganygaussians_amd import segmentation as seg
from tests import hdbscan_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
N_LIST = (31, 32, 33, 63, 64, 65, 255, 256, 257, 700)
CORE_KS = (1, 2, 10, 30, 64)


def bound(C):
    return (C / 2 + 2) * U


def gpu(a):
    a = np.array(a, order="C")   # a copy: the shared cases are read-only
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def bits_of(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


def euclid_rows(n, C, seed):
    x = np.random.default_rng(seed).normal(size=(n, C)).astype(np.float32)
    if n >= 3:
        x[n // 2] = x[0]          # one pair of equal rows: distance exactly 0
    return x


def bit_rows(n, Wd, seed):
    rng = np.random.default_rng(seed)
    x = ref.pack_bits(rng.random((n, 32 * Wd)) < rng.random((n, 1)))   # every density from empty to full
    if n >= 6:
        x[1] = 0
        x[n - 1] = 0              # two empty sets: d = 1 between them
        x[n // 2] = x[0]          # identical rows
    return x


# ---- core distances --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 32, 33, 64, 65, 256])
def test_core_distances_euclidean(C):
    shapes = [(n, CORE_KS) for n in N_LIST] + [(k, (k,)) for k in CORE_KS] + [(k + 1, (k,)) for k in CORE_KS]
    for n, ks in shapes:
        x = euclid_rows(n, C, 100 * C + n)
        D = ref.euclidean_matrix(x)
        xg = gpu(x)
        for k in ks:
            if k > n:
                continue
            got = cl.core_distances(xg, k).cpu().numpy().astype(np.float64)
            want = ref.core_distances(D, k)
            err = np.abs(got - want)
            print(f"C={C} n={n} k={k} max rel err / bound = {(err / np.maximum(want, 1e-300)).max() / bound(C):.3f}")
            assert (err <= bound(C) * want).all(), (C, n, k)
            assert (got[want == 0] == 0).all()
        if n >= 3:
            assert cl.core_distances(xg, min(2, n))[0].item() == 0.0


def test_core_distances_unaligned_rows_give_equal_bits():
    for C, n, k in ((32, 257, 10), (65, 65, 2), (3, 700, 30)):
        x = torch.from_numpy(euclid_rows(n, C, 7)).to(DEV)
        store = torch.empty(n * C + 1, dtype=torch.float32, device=DEV)
        shifted = store[1:].view(n, C)
        shifted.copy_(x)
        assert shifted.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 0 and shifted.is_contiguous()
        assert torch.equal(cl.core_distances(shifted, k).view(torch.int32), cl.core_distances(x, k).view(torch.int32))
        a, b = cl.mutual_reachability_mst(shifted, k), cl.mutual_reachability_mst(x, k)
        assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))


@pytest.mark.parametrize("Wd", [1, 2, 7, 32, 33, 1024])
def test_core_distances_jaccard_bitwise(Wd):
    for n in ((64, 65, 257) if Wd == 1024 else (6, 63, 64, 65, 257, 700)):
        x = bit_rows(n, Wd, 10 * Wd + n)
        D = ref.jaccard_matrix(x)
        assert D[1, n - 1] == 1.0 and D[0, n // 2] == D[0, 0]
        xg = gpu(x)
        for k in CORE_KS:
            if k > n:
                continue
            got = cl.core_distances(xg, k, metric="jaccard").cpu().numpy()
            assert np.array_equal(bits_of(got), bits_of(ref.core_distances(D, k))), (Wd, n, k)


# ---- the spanning tree -----------------------------------------------------------------------------------------------------------
def mst_input(metric, kind, n, seed):
    rng = np.random.default_rng(seed)
    third = (n + 2) // 3
    if metric == "euclidean":
        if kind == "planted":
            x = ref.planted(n, 32, 3, seed)
        elif kind == "uniform":
            x = rng.random((n, 32)).astype(np.float32)
        elif kind == "triples":
            x = np.repeat(rng.normal(size=(third, 32)).astype(np.float32), 3, axis=0)[:n][rng.permutation(n)]
        elif kind == "identical":
            x = np.repeat(rng.normal(size=(1, 32)).astype(np.float32), n, axis=0)
        else:   # grid: channel 0 on a lattice of equal gaps, the rest zero
            x = np.zeros((n, 3), np.float32)
            x[:, 0] = 0.25 * rng.permutation(n)
        return np.ascontiguousarray(x)
    if kind == "planted":
        x = ref.planted_bits(n, 3, seed)
    elif kind == "uniform":
        x = ref.pack_bits(rng.random((n, 96)) < 0.5)
    elif kind == "triples":
        x = np.repeat(ref.pack_bits(rng.random((third, 96)) < 0.5), 3, axis=0)[:n][rng.permutation(n)]
    elif kind == "identical":
        x = np.repeat(ref.pack_bits(rng.random((1, 96)) < 0.5), n, axis=0)
    else:       # grid: row i is the window of 32 bits that starts at bit i
        b = np.zeros((n, n + 32), bool)
        for i in range(n):
            b[i, i:i + 32] = True
        x = ref.pack_bits(b)[rng.permutation(n)]
    return np.ascontiguousarray(x)


@pytest.mark.parametrize("kind", ["planted", "uniform", "triples", "identical", "grid"])
@pytest.mark.parametrize("metric", ["euclidean", "jaccard"])
def test_mst(metric, kind):
    for n in (1, 2, 3, 64, 65, 257, 1500):
        x = mst_input(metric, kind, n, seed=n)
        k = min(10, n)
        C = x.shape[1]
        xg = gpu(x)
        core = cl.core_distances(xg, k, metric=metric).cpu().numpy()
        ea, eb, ew = (t.cpu().numpy() for t in cl.mutual_reachability_mst(xg, k, metric=metric))
        assert ea.shape == eb.shape == ew.shape == (n - 1,)
        if n == 1:
            continue
        assert (0 <= ea).all() and (ea < eb).all() and (eb < n).all()
        up = list(range(n))

        def find(v):
            while up[v] != v:
                up[v] = up[up[v]]
                v = up[v]
            return v

        for a, b in zip(ea.tolist(), eb.tolist()):
            ra, rb = find(a), find(b)
            assert ra != rb, (metric, kind, n, "a cycle")
            up[ra] = rb
        assert len({find(v) for v in range(n)}) == 1
        ra, rb, rw, rcore, D = ref.mst(x, metric, k)
        if metric == "jaccard":
            assert np.array_equal(bits_of(core), bits_of(rcore))
            own = np.maximum(np.maximum(core[ea], core[eb]), D[ea, eb].astype(np.float32))
            assert np.array_equal(bits_of(ew), bits_of(own)), (kind, n)
            assert np.array_equal(bits_of(np.sort(ew)), bits_of(np.sort(rw))), (kind, n)
        else:
            own = np.maximum(np.maximum(core[ea].astype(np.float64), core[eb]), D[ea, eb])
            assert (np.abs(ew - own) <= bound(C) * own).all(), (kind, n)
            want = np.sort(rw)
            assert (np.abs(np.sort(ew).astype(np.float64) - want) <= bound(C) * want).all(), (kind, n)
        assert _lib.load().mi_cluster_mst_rounds() <= max(1, int(np.ceil(np.log2(n))))


# ---- labels end to end -----------------------------------------------------------------------------------------------------------
def _label_cases():
    return [("euclidean", c) for c in ref.EUCLID_CONFIGS] + [("jaccard", c) for c in ref.JACCARD_CONFIGS]


@pytest.mark.parametrize("metric,config", _label_cases(), ids=lambda v: v if isinstance(v, str) else "-".join(str(x) for x in v))
def test_hdbscan_labels_match_restatement(metric, config):
    """The GUI's parameters (10, 0.01) and the notebook's (30, 0.25), both metrics, seeds 0-1."""
    mcs, eps = config[-2], config[-1]
    for seed in ref.GPU_SEEDS:
        pts, tree, lab = ref.planted_case(metric, config, seed)
        got = cl.hdbscan_labels(gpu(pts), mcs, cluster_selection_epsilon=eps, allow_single_cluster=False, metric=metric)
        assert got.dtype == torch.int64 and got.device == DEV and got.shape == (len(pts),)
        got = got.cpu().numpy()
        print(metric, config, seed, "clusters", got.max() + 1, "noise", int((got < 0).sum()), "differ", int((got < 0).sum() - (lab < 0).sum()))
        assert ref.same_partition(got, lab), (metric, config, seed)
        firsts = [int(np.flatnonzero(got == c)[0]) for c in range(got.max() + 1)]
        assert firsts == sorted(firsts)


def test_hdbscan_class_gives_the_labels_of_hdbscan_labels():
    pts, _, lab = ref.planted_case("euclidean", ref.EUCLID_CONFIGS[0], 0)
    h = cl.HDBSCAN(min_cluster_size=10, cluster_selection_epsilon=0.01, allow_single_cluster=False)
    got = h.fit_predict(np.asarray(pts, np.float64))
    assert isinstance(got, np.ndarray) and got is h.labels_ and h.fit(pts) is h
    assert np.array_equal(got, cl.hdbscan_labels(gpu(pts), 10, cluster_selection_epsilon=0.01).cpu().numpy())
    assert ref.same_partition(got, lab)


# ---- determinism, streams, guard words -------------------------------------------------------------------------------------------
def _run_all(xg, metric, mcs):
    core = cl.core_distances(xg, mcs, metric=metric)
    edges = cl.mutual_reachability_mst(xg, mcs, metric=metric)
    return [core.view(torch.int32)] + [e.view(torch.int32) for e in edges] + [cl.hdbscan_labels(xg, mcs, metric=metric)]


@pytest.mark.parametrize("metric", ["euclidean", "jaccard"])
def test_two_runs_and_another_stream_give_equal_bits(metric):
    config = ref.EUCLID_CONFIGS[1] if metric == "euclidean" else ref.JACCARD_CONFIGS[1]
    xg = gpu(ref.planted_case(metric, config, 0)[0])
    first, second = _run_all(xg, metric, config[-2]), _run_all(xg, metric, config[-2])
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        third = _run_all(xg, metric, config[-2])
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, third))


@pytest.mark.parametrize("metric,width,n,k", [("euclidean", 32, 257, 10), ("euclidean", 65, 65, 30), ("jaccard", 7, 130, 64)])
def test_guard_words_stay_intact(metric, width, n, k):
    L = _lib.load()
    mid = cl.METRICS[metric]
    xg = gpu(euclid_rows(n, width, 3) if metric == "euclidean" else bit_rows(n, width, 3))
    nbytes = int(L.mi_cluster_workspace_bytes(mid, n, width, k))
    G, MARK = 64, 0x5A5A5A5A
    ws = torch.full((nbytes // 4 + G,), MARK, dtype=torch.int32, device=DEV)
    core = torch.full((n + G,), MARK, dtype=torch.int32, device=DEV)
    ea, eb, ew = (torch.full((n - 1 + G,), MARK, dtype=torch.int32, device=DEV) for _ in range(3))
    stream = torch.cuda.current_stream(DEV).cuda_stream
    assert L.mi_cluster_core_distances(mid, n, width, xg.data_ptr(), k, core.data_ptr(), ws.data_ptr(), nbytes, stream) == 0, _lib.last_error()
    assert L.mi_cluster_mst(mid, n, width, xg.data_ptr(), core.data_ptr(), ea.data_ptr(), eb.data_ptr(), ew.data_ptr(), ws.data_ptr(),
                            nbytes, stream) == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert (ws[(nbytes + 3) // 4:] == MARK).all() and (core[n:] == MARK).all()
    for t in (ea, eb, ew):
        assert (t[n - 1:] == MARK).all()
    assert torch.equal(core[:n], cl.core_distances(xg, k, metric=metric).view(torch.int32))
    assert (ea[:n - 1] < eb[:n - 1]).all() and (eb[:n - 1] < n).all() and (ea[:n - 1] >= 0).all()


# ---- the GUI's path, end to end --------------------------------------------------------------------------------------------------
def test_cluster_in_3d_end_to_end():
    """saga_gui.py:518-543 on a planted feature table: gate, normalise, a 2 % sample, hdbscan_labels, cluster_centers, assign_clusters.
    Every planted member must land on the centre of its own planted cluster: 0 misassigned."""
    P, C, K = 20000, 32, 6
    feats, truth = ref.planted(P, C, K, seed=11, with_truth=True)
    g = torch.Generator().manual_seed(3)
    gates = (0.75 + 0.5 * torch.rand(C, generator=g)).to(DEV)
    f = gpu(feats)
    pick = (torch.rand(P, generator=g) > 0.98).to(DEV)
    normed = torch.nn.functional.normalize(f, dim=-1)
    sample = torch.nn.functional.normalize(normed[pick] * gates, dim=-1).contiguous()
    labels = cl.hdbscan_labels(sample, min_cluster_size=10, cluster_selection_epsilon=0.01, allow_single_cluster=False)
    centers = cl.cluster_centers(sample, labels)
    assert centers.shape == (K, C) and torch.allclose(centers.norm(dim=-1), torch.ones(K, device=DEV), atol=1e-5)
    assigned, _ = seg.assign_clusters(f, centers, gates=gates, pre="l2")
    assigned, truth_s, lab_s = assigned.cpu().numpy(), truth[pick.cpu().numpy()], labels.cpu().numpy()
    own = {}
    for j in range(K):                                           # the centre of planted cluster j: where its sampled members went
        votes = lab_s[(truth_s == j) & (lab_s >= 0)]
        assert len(votes) >= 10 and len(set(votes.tolist())) == 1, j
        own[j] = int(votes[0])
    assert len(set(own.values())) == K
    misassigned = sum(int((assigned[truth == j] != own[j]).sum()) for j in range(K))
    print("misassigned planted members:", misassigned, "of", int((truth >= 0).sum()))
    assert misassigned == 0
