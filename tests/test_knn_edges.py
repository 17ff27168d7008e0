"""Edge tests of the exact HIP KNN (include/mi_knn.h, csrc/knn.h) against exhaustive search, judged in every row by the rule
of tests/knn_ref.py: indices and distances bit-equal to the binary32 exhaustive search ordered by (distance, index), every
distance within 6 * 2^-24 * d + 2^-125 of float64, distCUDA2 bit-equal to ((d0 + d1) + d2) / 3.  No row is excused.

Sizes sit on the structural seams of the index: 64 points per leaf, 4096 per super box, 1024 keys per sort tile in rounds of
256, the 1024-entry chunks of the histogram scan, 64 queries per workgroup, a compiled list size above K and above M.  The
classes of tests/knn_ref.py add exact ties, degenerate boxes, one Morton cell, underflow and overflow of the float32 distance.
"""
import functools

import pytest
import torch

from seganygaussians_amd import _lib, knn
from seganygaussians_amd import knn_smooth as ks
from tests import knn_ref as kr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SEAM_M = (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3072, 3073, 4095, 4096, 4097, 8193)
COMPILED_K, OTHER_K = (1, 3, 4, 8, 16, 32), (2, 5, 17, 31)
FREE_N = (1, 63, 64, 65, 257)


@functools.lru_cache(maxsize=None)
def _case(name, M):
    """the case's points on the device, its property asserted there once"""
    case = kr.make_case(name, M)
    case.check(DEV)
    return case.points.to(DEV)


@functools.lru_cache(maxsize=None)
def _self_ref(name, M, exclude_self):
    """((idx, d2) of the float32 exhaustive search, float64 distances) at the largest K the size allows; smaller K are prefixes"""
    x = _case(name, M)
    K = min(kr.MAX_K, M - int(exclude_self))
    return kr.exhaustive_f32(x, x, K, exclude_self), kr.exhaustive_f64(x, x, K, exclude_self)


def _check_self(name, M, index, K, exclude_self):
    x = _case(name, M)
    ref, d64 = _self_ref(name, M, exclude_self)
    idx, d2 = index.query(None, K, exclude_self=exclude_self)
    kr.assert_rule(x, x, K, idx, d2, exclude_self, ref=ref, d64=d64, what=f"{name} M={M} K={K} exclude_self={exclude_self}")
    return idx, d2


def _check_free(q, refs, index, ks_, what):
    M = refs.size(0)
    top = min(max(ks_), M)
    ref, d64 = kr.exhaustive_f32(q, refs, top), kr.exhaustive_f64(q, refs, top)
    out = {}
    for K in ks_:
        if K <= M:
            idx, d2 = index.query(q, K)
            kr.assert_rule(q, refs, K, idx, d2, ref=ref, d64=d64, what=f"{what} N={q.size(0)} M={M} K={K}")
            out[K] = (idx, d2)
    return out


# ---- seams, self queries -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", SEAM_M)
@pytest.mark.parametrize("name", ["uniform", "lattice"])
def test_seams_self_queries(name, M):
    index = knn.KnnIndex(_case(name, M))
    ran = 0
    for exclude_self in (False, True):
        for K in COMPILED_K + (OTHER_K if M in (65, 4097) else ()):
            if K <= M - int(exclude_self):
                _check_self(name, M, index, K, exclude_self)
                ran += 1
    assert ran >= (1 if M == 1 else 2)


@pytest.mark.parametrize("K", [1, 3, 4, 5, 8, 16, 17, 32])
@pytest.mark.parametrize("name", ["uniform", "lattice"])
def test_as_many_neighbours_as_candidates(name, K):
    """M == K (for K = 5, 17 the compiled list, 8 and 32 long, is longer than M) and M == K + 1 without the point itself"""
    _check_self(name, K, knn.KnnIndex(_case(name, K)), K, False)
    idx, _ = _check_self(name, K + 1, knn.KnnIndex(_case(name, K + 1)), K, True)
    assert torch.equal(idx.sort(1).values, torch.tensor([[j for j in range(K + 1) if j != i] for i in range(K + 1)], device=DEV))


# ---- every class of the table ------------------------------------------------------------------------------------------------

def _class_cases():
    return [(n, M) for n in sorted(kr.CLASSES) for M in (257, 4097)] + [("overflow", 10)]


@pytest.mark.parametrize("name,M", _class_cases())
def test_every_class_self_queries_and_dist_cuda2(name, M):
    x = _case(name, M)
    index = knn.KnnIndex(x)
    rows = torch.arange(M, device=DEV)[:, None]
    for K in (3, 8) if M == 10 else (3, 16):       # 10 points: two clusters of 5, K = 8 needs neighbours at distance +inf
        for exclude_self in (False, True):
            idx, d2 = _check_self(name, M, index, K, exclude_self)
            assert bool(((idx >= 0) & (idx < M)).all()), "an index outside [0, M)"
            if exclude_self:
                assert not bool((idx == rows).any())
            if name in ("coincident", "underflow"):       # every distance 0: the K lowest indices (other than the row's own)
                cols = torch.arange(K, device=DEV).expand(M, K)
                want = cols + (cols >= rows).long() if exclude_self else cols
                assert torch.equal(idx, want) and bool((d2 == 0).all())
    if name == "overflow":
        assert bool(torch.isinf(_self_ref(name, M, False)[0][1][:, :8]).any()), "no neighbour at distance +inf was needed"
    kr.assert_mean3(x, knn.distCUDA2(x), ref3=_self_ref(name, M, True)[0][1], what=f"{name} M={M}")


# ---- free queries ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["uniform", "lattice", "repeats"])
@pytest.mark.parametrize("M", FREE_N + (4097,))
def test_free_queries_equal_to_the_references_match_the_self_path(name, M):
    if name == "repeats" and M < 65:      # no leaf seam to straddle below 65 points
        name = "coincident"
    x = _case(name, M)
    index = knn.KnnIndex(x)
    got = _check_free(x.clone(), x, index, (1, 3, 16, 32), f"{name} clone")
    for K, (idx, d2) in got.items():
        si, sd = index.query(None, K)
        assert torch.equal(idx, si) and torch.equal(d2.view(torch.int32), sd.view(torch.int32))


def _rand(N, seed, lo=-2.0, hi=2.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(N, 3, generator=g) * (hi - lo) + lo).to(DEV)


@pytest.mark.parametrize("N", FREE_N)
def test_free_queries_at_lattice_cell_centres(N):
    """8 lattice points at the same distance from every query (where the lattice is filled): ties by index at every rank"""
    refs = _case("lattice", 4097)                       # 4097 of the 17^3 = 4913 lattice points
    q = torch.randint(0, 16, (N, 3), generator=torch.Generator().manual_seed(N)).float().to(DEV) + 0.5
    got = _check_free(q, refs, knn.KnnIndex(refs), (1, 3, 4, 8, 16, 32), "cell centres")
    d8 = got[8][1]
    assert float((d8[:, 0] == d8[:, 3]).float().mean()) >= 0.5 or N == 1, "the case lost its ties"


@pytest.mark.parametrize("N", FREE_N)
@pytest.mark.parametrize("name,M", [("uniform", 1025), ("lattice", 4097), ("planar_7.25", 257)])
def test_free_queries_outside_on_and_in_the_box(name, M, N):
    refs = _case(name, M)
    index = knn.KnnIndex(refs)
    lo, hi = refs.min(0).values, refs.max(0).values
    size = torch.clamp(hi - lo, min=1.0)
    corner = torch.tensor([[(c >> a) & 1 for a in range(3)] for c in range(8)], device=DEV, dtype=torch.float32)
    sign = corner[torch.arange(N, device=DEV) % 8] * 2 - 1
    # 10 box sizes outside, towards every corner (the Morton clamp, centre = min(lo, M - 1) at the far end of the order)
    jitter = 1 + 0.1 * torch.rand(N, 3, generator=torch.Generator().manual_seed(N)).to(DEV)
    _check_free((lo + hi) / 2 + sign * 10.5 * size * jitter, refs, index, (1, 3, 16), f"{name} outside")
    # exactly on the corners (first 8 rows), then on faces and edges: each coordinate lo, hi or inside, never all three inside
    g = torch.Generator().manual_seed(100 + N)
    pick = torch.randint(0, 3, (N, 3), generator=g).to(DEV)
    pick[torch.arange(N, device=DEV), torch.randint(0, 3, (N,), generator=g).to(DEV)] = torch.randint(0, 2, (N,), generator=g).to(DEV)
    pick[:min(N, 8)] = corner[:min(N, 8)].long()
    inside = lo + (hi - lo) * torch.rand(N, 3, generator=g).to(DEV)
    q = torch.where(pick == 0, lo.expand(N, 3), torch.where(pick == 1, hi.expand(N, 3), inside))
    assert bool(((q == lo) | (q == hi)).any(1).all())
    _check_free(q, refs, index, (1, 3, 16), f"{name} faces")
    _check_free(_rand(N, N + 7, float(lo.min()), float(hi.max())), refs, index, (1, 3, 16), f"{name} inside")


@pytest.mark.parametrize("N", FREE_N)
def test_free_queries_against_one_reference(N):
    refs = torch.tensor([[0.5, -1.25, 3.0]], device=DEV)
    index = knn.KnnIndex(refs)
    q = _rand(N, N)
    q[0] = refs[0]
    got = _check_free(q, refs, index, (1,), "one reference")
    assert bool((got[1][0] == 0).all()) and float(got[1][1][0, 0]) == 0.0
    with pytest.raises(RuntimeError, match="neighbours requested from 1 reference points"):
        index.query(q, 3)


@pytest.mark.parametrize("N", FREE_N)
@pytest.mark.parametrize("name", ["one_cell", "coincident", "collinear_0", "signed_zero", "underflow", "overflow"])
def test_free_queries_against_degenerate_references(name, N):
    refs = _case(name, 257)
    index = knn.KnnIndex(refs)
    scale = {"underflow": 1e-29, "overflow": 3e19}.get(name, 2.0)
    q = _rand(N, N + 1) * (scale / 2.0)
    q[::3] = refs[torch.arange(0, N, 3, device=DEV) % 257]           # some queries are reference points
    if name == "one_cell":
        q[1::3] = _rand(N, N + 2, 0.0, 1e-3)[1::3]                    # inside the dense cell
    got = _check_free(q, refs, index, (1, 3, 16), name)
    if name == "coincident":
        assert torch.equal(got[16][0], torch.arange(16, device=DEV).expand(N, 16))
    assert all(bool(((i >= 0) & (i < 257)).all()) for i, _ in got.values())


@pytest.mark.parametrize("N", FREE_N + (4097,))
def test_references_are_a_random_half_of_the_queries(N):
    """get_multi_resolution_smoothed_point_features (gaussian_model_ff.py:376-384)"""
    q = _case("uniform", N) if N < 4097 else _case("repeats", N)
    keep = torch.rand(N, generator=torch.Generator().manual_seed(N)) < 0.5
    keep[0] = True
    refs = q[keep.to(DEV)]
    got = _check_free(q, refs, knn.KnnIndex(refs), (1, 4, 16), "subset references")
    assert bool((got[1][1][keep.to(DEV)] == 0).all())
    if refs.size(0) >= 4:
        r = knn.knn_points(q.unsqueeze(0), refs.unsqueeze(0), K=4)
        assert torch.equal(r.idx[0], got[4][0]) and torch.equal(r.dists[0], got[4][1])


# ---- entry points and buffers --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [257, 4097])
def test_entry_points_on_a_lattice(M):
    x = _case("lattice", M)
    (ri, rd), _ = _self_ref("lattice", M, False)
    r = knn.knn_points(x.unsqueeze(0), x.unsqueeze(0), K=16)                      # same tensor: the self path
    assert torch.equal(r.idx[0], ri[:, :16]) and torch.equal(r.dists[0], rd[:, :16]) and r.knn is None
    r = knn.knn_points(x.clone().unsqueeze(0), x.unsqueeze(0), K=4, return_nn=True)   # different tensors: free queries
    assert torch.equal(r.idx[0], ri[:, :4]) and torch.equal(r.dists[0], rd[:, :4]) and torch.equal(r.knn[0], x[ri[:, :4]])
    nmap = ks.NeighbourMap.from_points(x, K=16)
    assert torch.equal(nmap.idx.long(), ri[:, :16])


def test_dist_cuda2_with_fewer_than_three_other_points():
    x = _case("uniform", 4)
    for P in (1, 2, 3):     # the list keeps initial distances, whose sum overflows: what simple-knn's FLT_MAX initialisation gives
        got = knn.distCUDA2(x[:P].contiguous())
        assert got.shape == (P,) and bool((got == float("inf")).all()), got
    kr.assert_mean3(x, knn.distCUDA2(x), what="P=4")
    assert bool(torch.isfinite(knn.distCUDA2(x)).all())
    assert knn.distCUDA2(x[:0]).shape == (0,)


def _raw(M_pts, q, K, exclude_self, pad=64):
    """mi_knn_build + mi_knn_query straight through the C ABI into buffers with a canary tail"""
    L = _lib.load()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    M = M_pts.size(0)
    nbytes = int(L.mi_knn_workspace_bytes(M))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    assert L.mi_knn_build(M, M_pts.data_ptr(), ws.data_ptr(), nbytes, stream) == 0, _lib.last_error()
    rows = M if q is None else q.size(0)
    idx = torch.full((rows * K + pad,), -7, dtype=torch.int64, device=DEV)
    d2 = torch.full((rows * K + pad,), -123.0, dtype=torch.float32, device=DEV)
    rc = L.mi_knn_query(rows, None if q is None else q.data_ptr(), M, ws.data_ptr(), K, int(exclude_self), idx.data_ptr(), d2.data_ptr(), stream)
    torch.cuda.synchronize()
    return rc, idx, d2, rows


@pytest.mark.parametrize("rows", [1, 65])
def test_rows_past_the_last_are_untouched(rows):
    for self_query in (True, False):
        refs = _case("lattice", rows if self_query else 257)
        q = None if self_query else _rand(rows, rows, 0.0, 6.0)
        for K in (1, 3, 16):
            excl = self_query and K < rows
            if K > refs.size(0) - int(excl):
                continue
            rc, idx, d2, n = _raw(refs, q, K, excl)
            assert rc == 0 and n == rows
            assert bool((idx[rows * K:] == -7).all()) and bool((d2[rows * K:] == -123.0).all()), "wrote past the last row"
            kr.assert_rule(refs if q is None else q, refs, K, idx[:rows * K].view(rows, K), d2[:rows * K].view(rows, K), excl,
                           what=f"raw rows={rows} K={K} self={self_query}")


def test_more_neighbours_than_references_through_the_c_abi():
    refs = _case("uniform", 3)
    rc, idx, d2, _ = _raw(refs, None, 4, False)
    assert rc == 0
    idx, d2 = idx[:12].view(3, 4), d2[:12].view(3, 4)
    kr.assert_rule(refs, refs, 3, idx[:, :3].contiguous(), d2[:, :3].contiguous(), what="K=4 from M=3")
    assert bool((idx[:, 3] == -1).all()) and bool((d2[:, 3] == float("inf")).all())     # the documented padding
    rc, idx, d2, _ = _raw(refs, None, 5, False)
    assert rc != 0 and "knn: K must be one of 1, 3, 4, 8, 16, 32" in _lib.last_error()
    assert bool((idx == -7).all()) and bool((d2 == -123.0).all())


# ---- determinism ---------------------------------------------------------------------------------------------------------------

def test_build_and_query_twice_bit_identical():
    x = _case("repeats", 4097)
    q = _rand(257, 5)

    def run():
        index = knn.KnnIndex(x)
        out = list(index.query(None, 16)) + list(index.query(None, 3, exclude_self=True)) + list(index.query(q, 8))
        return out + [knn.distCUDA2(x)]
    for u, v in zip(run(), run()):
        assert torch.equal(u.view(torch.int32) if u.dtype == torch.float32 else u, v.view(torch.int32) if v.dtype == torch.float32 else v)
