"""References, rule and edge-case generators for the exact KNN search (include/mi_knn.h, csrc/knn.h).  Nothing here imports the
search under test.

The promise: the K smallest squared distances `(dx*dx + dy*dy) + dz*dz`, `d = reference - query`, every operation rounded to
binary32 on its own, ascending, ties by reference index.  `exhaustive_f32` restates it with eager elementwise torch ops (which
do not contract) and a stable sort over the index-ordered columns; `exhaustive_f32_numpy` with NumPy and `lexsort` (host test,
small M).  `exhaustive_f64` gives the sorted float64 distances of the same float32 inputs.

The rule (`assert_rule`, `assert_mean3`), no row excused:
  1. idx and d2 are equal, bit for bit, to `exhaustive_f32` in every row and column, ties included;
  2. |d2[r] - d64[r]| <= 6 * 2^-24 * d64[r] + 2^-125 for every row and rank r.  Three subtractions, three squares and two sums
     of non-negative terms put at most 5 roundings of relative size 2^-24 on any term, 6 covers the second-order terms; the
     absolute term covers products that underflow (denormals kept or flushed).  Order statistics move by no more than the
     largest perturbation, so the bound holds rank by rank without matching neighbours.  Where d64[r] exceeds the largest
     float32 the value must be +inf;
  3. distCUDA2 is bit-equal to `((d0 + d1) + d2) / 3` in binary32 of `exhaustive_f32(x, x, 3, exclude_self=True)`.

Inputs are finite.  NaN and infinite coordinates are out of scope: the search makes no promise for them.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional

import numpy as np
import torch

F32_MAX = float(np.finfo(np.float32).max)
REL, ABS = 6.0 * 2.0 ** -24, 2.0 ** -125
LEAF, SUPER, MAX_K = 64, 4096, 32      # points per leaf box / per super box (csrc/knn.h), restated


# ---- references --------------------------------------------------------------------------------------------------------------

def _dist_f32(q: torch.Tensor, refs: torch.Tensor) -> torch.Tensor:
    d = refs[None, :, :] - q[:, None, :]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def _drop_self(idx, val, first_row, K):
    """from K + 1 sorted columns: drop the row's own index where it is among them, keep the order, return K columns"""
    rows = torch.arange(first_row, first_row + idx.size(0), device=idx.device)[:, None]
    order = torch.sort((idx == rows).to(torch.int8), dim=1, stable=True).indices[:, :K]
    return idx.gather(1, order), val.gather(1, order)


def exhaustive_f32(queries: torch.Tensor, refs: torch.Tensor, K: int, exclude_self: bool = False, chunk: int = 1024):
    """(idx int64 [N, K], d2 float32 [N, K]): every pairwise binary32 distance, each row ordered by (distance, index)."""
    q, r = queries.to(torch.float32), refs.to(torch.float32)
    N, M = q.size(0), r.size(0)
    assert 1 <= K <= M - (1 if exclude_self else 0)
    if exclude_self:
        assert N == M, "exclude_self: the queries are the references"
    idx = torch.empty((N, K), dtype=torch.int64, device=q.device)
    d2 = torch.empty((N, K), dtype=torch.float32, device=q.device)
    take = K + 1 if exclude_self else K
    for s in range(0, N, chunk):
        v, i = torch.sort(_dist_f32(q[s:s + chunk], r), dim=1, stable=True)   # stable over index-ordered columns: ties by index
        v, i = v[:, :take], i[:, :take]
        if exclude_self:
            i, v = _drop_self(i, v, s, K)
        idx[s:s + chunk], d2[s:s + chunk] = i, v
    return idx, d2


def exhaustive_f64(queries: torch.Tensor, refs: torch.Tensor, K: int, exclude_self: bool = False, chunk: int = 1024) -> torch.Tensor:
    """sorted float64 squared distances [N, K] of the float32 inputs"""
    q, r = queries.to(torch.float32).double(), refs.to(torch.float32).double()
    N = q.size(0)
    out = torch.empty((N, K), dtype=torch.float64, device=q.device)
    for s in range(0, N, chunk):
        d = r[None, :, :] - q[s:s + chunk, None, :]
        d = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        if exclude_self:   # float64 distances of float32 points are finite, so +inf marks the row's own column safely
            n = d.size(0)
            d[torch.arange(n, device=d.device), torch.arange(s, s + n, device=d.device)] = float("inf")
        out[s:s + chunk] = torch.sort(d, dim=1).values[:, :K]
    return out


def exhaustive_f32_numpy(queries, refs, K: int, exclude_self: bool = False):
    """the same promise with NumPy: float32 operations one by one, `lexsort` by (distance, index).  Small M only."""
    q, r = np.asarray(queries, np.float32), np.asarray(refs, np.float32)
    N, M = q.shape[0], r.shape[0]
    idx, d2 = np.empty((N, K), np.int64), np.empty((N, K), np.float32)
    cols = np.arange(M)
    for n in range(N):
        d = r - q[n]
        with np.errstate(over="ignore", under="ignore"):
            dist = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert dist.dtype == np.float32
        order = np.lexsort((cols, dist))
        if exclude_self:
            order = order[order != n]
        idx[n], d2[n] = order[:K], dist[order[:K]]
    return idx, d2


def mean3_f32(d2: torch.Tensor) -> torch.Tensor:
    s3 = (d2[:, 0] + d2[:, 1]) + d2[:, 2]
    return torch.div(s3, torch.full_like(s3, 3.0))     # a tensor divisor: true division (a scalar one becomes x * (1/3))


# ---- the rule ------------------------------------------------------------------------------------------------------------------

def value_bound_violations(d2: torch.Tensor, d64: torch.Tensor) -> torch.Tensor:
    """part 2 of the rule: boolean [N, K], True where a value breaks the bound"""
    over = d64 > F32_MAX
    err = (d2.double() - d64).abs()
    bad = ~(err <= REL * d64 + ABS)           # NaN and inf - finite count as violations
    return torch.where(over, ~(torch.isinf(d2) & (d2 > 0)), bad)


def assert_rule(queries, refs, K, idx, d2, exclude_self=False, ref=None, d64=None, what=""):
    """parts 1 and 2; `ref` = (idx, d2) of exhaustive_f32 and `d64` of exhaustive_f64 with at least K columns, when shared"""
    N = queries.size(0)
    assert idx.shape == (N, K) and d2.shape == (N, K) and idx.dtype == torch.int64 and d2.dtype == torch.float32, what
    ri, rd = ref if ref is not None else exhaustive_f32(queries, refs, K, exclude_self)
    ri, rd = ri[:, :K], rd[:, :K]
    if not torch.equal(idx, ri):
        rows = (idx != ri).any(1).nonzero().flatten()
        r = int(rows[0])
        raise AssertionError(f"{what}: indices differ from exhaustive search in {rows.numel()} of {N} rows, first row {r}: "
                             f"got {idx[r].tolist()} {d2[r].tolist()}, want {ri[r].tolist()} {rd[r].tolist()}")
    # bit for bit: compare the words, so that -0.0 / +0.0 or a NaN cannot slip through
    assert torch.equal(d2.view(torch.int32), rd.view(torch.int32)), f"{what}: distances differ from exhaustive search"
    d64 = d64[:, :K] if d64 is not None else exhaustive_f64(queries, refs, K, exclude_self)
    bad = value_bound_violations(d2, d64)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} distances outside 6 * 2^-24 * d + 2^-125 of float64"


def assert_mean3(points, got, ref3=None, what=""):
    """part 3; `ref3` = the distances of exhaustive_f32(points, points, 3, exclude_self=True), when shared"""
    d = ref3 if ref3 is not None else exhaustive_f32(points, points, 3, exclude_self=True)[1]
    want = mean3_f32(d[:, :3])
    assert got.shape == want.shape and got.dtype == torch.float32, what
    bad = got.view(torch.int32) != want.view(torch.int32)
    assert not bool(bad.any()), f"{what}: distCUDA2 differs from ((d0 + d1) + d2) / 3 in {int(bad.sum())} of {got.numel()} rows"


# ---- the index's Morton arithmetic, restated (csrc/knn.h: f2ord, ord2f, prep_morton, morton_of) ---------------------------------

def _ordered(a: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _unordered(o: np.ndarray) -> np.ndarray:
    o = np.asarray(o, np.uint32)
    return np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32).view(np.float32)


def box_of(refs: np.ndarray):
    """(lo, hi, ordered lo, ordered hi) as the index takes them: min / max over the ordered-int image of the floats"""
    o = _ordered(refs)
    olo, ohi = o.min(0), o.max(0)
    return _unordered(olo), _unordered(ohi), olo, ohi


def _spread(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint32)
    x = (x | (x << np.uint32(16))) & np.uint32(0x030000FF)
    x = (x | (x << np.uint32(8))) & np.uint32(0x0300F00F)
    x = (x | (x << np.uint32(4))) & np.uint32(0x030C30C3)
    x = (x | (x << np.uint32(2))) & np.uint32(0x09249249)
    return x


def morton_codes(points: np.ndarray, refs: Optional[np.ndarray] = None) -> np.ndarray:
    """30-bit codes of `points` in the box of `refs` (default: their own), float32 operation by operation"""
    p = np.ascontiguousarray(points, np.float32)
    lo, hi, _, _ = box_of(p if refs is None else np.ascontiguousarray(refs, np.float32))
    code = np.zeros(p.shape[0], np.uint32)
    with np.errstate(all="ignore"):
        for a in range(3):
            ext = np.float32(hi[a] - lo[a])
            t = ((p[:, a] - lo[a]) / ext).astype(np.float32) if ext > 0 else np.zeros(p.shape[0], np.float32)
            t = np.minimum(np.maximum(t, np.float32(0)), np.float32(1))
            code |= _spread((t * np.float32(1023.0)).astype(np.float32).astype(np.uint32)) << np.uint32(a)
    return code


def morton_order(points: np.ndarray) -> np.ndarray:
    """reference indices in the order the index stores them: stable sort of (code, index)"""
    return np.argsort(morton_codes(points), kind="stable")


# ---- case generators -------------------------------------------------------------------------------------------------------------

class Case(NamedTuple):
    name: str
    points: torch.Tensor                    # float32 [M, 3], CPU, index order shuffled
    check: Callable[..., None]              # check(device="cpu"): asserts the property that makes the case bite


def _shuffled(rng, pts) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(pts)[rng.permutation(len(pts))])


def _not_morton_ordered(p: np.ndarray):
    if len(p) >= 63 and len(np.unique(p, axis=0)) > 8:
        assert not np.array_equal(morton_order(p), np.arange(len(p))), "index order is Morton order"


def _tie_shares(x: torch.Tensor, ks, exclude_self: bool, chunk: int = 1024) -> dict:
    """K -> share of rows whose K-th and (K+1)-th float32 distances are equal"""
    M, top = x.size(0), max(ks) + 1
    eq = torch.zeros(top - 1, dtype=torch.float64, device=x.device)
    for s in range(0, M, chunk):
        d = _dist_f32(x[s:s + chunk], x)
        if exclude_self:       # only used on inputs whose distances are finite
            n = d.size(0)
            d[torch.arange(n, device=d.device), torch.arange(s, s + n, device=d.device)] = float("inf")
        v = torch.topk(d, top, dim=1, largest=False).values
        eq += (v[:, :-1] == v[:, 1:]).double().sum(0)
    return {K: float(eq[K - 1]) / M for K in ks}


def tied_lists(M: int, K: int):
    """which of the two self-query lists of a lattice are tied between rank K and K + 1 in at least half the rows: with the
    point itself (distance 0, then shells of 6, 12, 8, 6, 24 ... equal distances) every K >= 2, without it every K"""
    return [e for e in (False, True) if K + 1 <= M - int(e) and (e or K >= 2)]


def uniform(M, seed=0) -> Case:
    rng = np.random.default_rng([seed, M, 1])
    p = (rng.random((M, 3)) * 4 - 2).astype(np.float32)

    def check(device="cpu"):
        x = torch.from_numpy(p).to(device)
        i, d = exhaustive_f32(x, x, min(2, M))
        assert torch.equal(i[:, 0], torch.arange(M, device=x.device)) and bool((d[:, 0] == 0).all())
        assert M == 1 or bool((d[:, 1] > 0).all()), "a second zero distance: the self distance is not unique"
        _not_morton_ordered(p)
    return Case("uniform", torch.from_numpy(p), check)


LATTICE_MIN_M = 63      # below this a lattice has too few shells for the tie property


def lattice(M, seed=0, ks=(1, 2, 3, 4, 5, 8, 16, 17, 31, 32)) -> Case:
    """the first M points of a shuffled g x g x g integer lattice, g the smallest side with g^3 > M (21 at M = 8193): never the
    full cube, whose few distinct distances leave some ranks untied in most rows"""
    g = 1
    while g ** 3 <= M:
        g += 1
    rng = np.random.default_rng([seed, M, 2])
    grid = np.stack(np.meshgrid(np.arange(g), np.arange(g), np.arange(g), indexing="ij"), -1).reshape(-1, 3)
    p = _shuffled(rng, grid)[:M].astype(np.float32)

    def check(device="cpu"):
        if M < LATTICE_MIN_M:
            return
        x = torch.from_numpy(p).to(device)
        for e in (False, True):
            use = [K for K in ks if e in tied_lists(M, K)]
            for K, share in _tie_shares(x, use, e).items():
                assert share >= 0.5, f"lattice M={M} K={K} exclude_self={e}: ranks K and K+1 tie in only {share:.3f} of the rows"
        _not_morton_ordered(p)
    return Case("lattice", torch.from_numpy(p), check)


def coincident(M, seed=0) -> Case:
    p = np.tile(np.array([[0.75, -1.5, 3.25]], np.float32), (M, 1))

    def check(device="cpu"):
        assert (p == p[0]).all()
    return Case("coincident", torch.from_numpy(p), check)


def _flat(M, seed, axes, value, name, signed_zero=False) -> Case:
    rng = np.random.default_rng([seed, M, 3, len(axes)])
    p = (rng.random((M, 3)) * 4 - 2).astype(np.float32)
    for a in axes:
        p[:, a] = value
    if signed_zero:
        assert value == 0 and M >= 2
        neg = rng.random(M) < 0.5
        neg[0], neg[1] = True, False
        p[neg, axes[0]] = -0.0
    p = _shuffled(rng, p)

    def check(device="cpu"):
        lo, hi, olo, ohi = box_of(p)
        for a in axes:
            assert np.float32(hi[a] - lo[a]) == 0, "extent not exactly 0"
            assert (olo[a] != ohi[a]) == signed_zero, "ordered-int min and max"
        free = [a for a in range(3) if a not in axes]
        assert all(hi[a] - lo[a] > 0 for a in free) or M == 1
        _not_morton_ordered(p)
    return Case(name, torch.from_numpy(p), check)


def planar(M, seed=0, value=0.0) -> Case:
    return _flat(M, seed, (2,), np.float32(value), "planar")


def collinear(M, seed=0, value=0.0) -> Case:
    return _flat(M, seed, (0, 2), np.float32(value), "collinear")


def signed_zero(M, seed=0) -> Case:
    return _flat(M, seed, (1,), np.float32(0.0), "signed_zero", signed_zero=True)


def one_cell(M, seed=0) -> Case:
    assert M >= 3
    rng = np.random.default_rng([seed, M, 4])
    p = (rng.random((M, 3)) * 1e-3).astype(np.float32)
    out = rng.choice(M, 2, replace=False)
    p[out[0]], p[out[1]] = 1e3, -1e3

    def check(device="cpu"):
        dense = np.ones(M, bool)
        dense[out] = False
        codes = morton_codes(p)
        assert len(np.unique(codes[dense])) == 1, "the dense points do not share one Morton code"
        assert codes[out[0]] != codes[dense][0] and codes[out[1]] != codes[dense][0]
        assert len(np.unique(p[dense], axis=0)) > 0.9 * (M - 2)
    return Case("one_cell", torch.from_numpy(p), check)


def repeats(M, seed=0) -> Case:
    """every distinct point 2 to 40 times; the sub-seed is advanced until a run straddles a leaf and (M > 4096) a super-box seam"""
    def build(sub):
        rng = np.random.default_rng([seed, M, 5, sub])
        counts = []
        while sum(counts) < M:
            counts.append(int(rng.integers(2, 41)))
        counts[-1] -= sum(counts) - M
        if counts[-1] < 2:                      # fold a remainder of 0 or 1 into the run before
            last = counts.pop()
            counts[-1] += last
        base = (rng.random((len(counts), 3)) * 4 - 2).astype(np.float32)
        return _shuffled(rng, np.repeat(base, counts, axis=0)), counts

    def seams(p):
        s = p[morton_order(p)]
        return [b for b in range(LEAF, M, LEAF) if (s[b - 1] == s[b]).all()]

    for sub in range(64):
        p, counts = build(sub)
        cross = seams(p)
        if cross and (M <= SUPER or any(b % SUPER == 0 for b in cross)):
            break

    def check(device="cpu"):
        assert len(p) == M and min(counts) >= 2 and max(counts) <= 41
        cross = seams(p)
        assert cross, "no run of repeats crosses a multiple of 64 in Morton order"
        assert M <= SUPER or any(b % SUPER == 0 for b in cross), "no run of repeats crosses a multiple of 4096"
        _not_morton_ordered(p)
    return Case("repeats", torch.from_numpy(p), check)


def offset(M, seed=0) -> Case:
    """a cloud of typical spacing 1e-3 at 1e4, where a float32 step is 9.8e-4"""
    rng = np.random.default_rng([seed, M, 6])
    p64 = 1e4 + rng.random((M, 3)) * (1e-3 * M ** (1.0 / 3.0))
    p = p64.astype(np.float32)

    def check(device="cpu"):
        assert len(np.unique(p64, axis=0)) == M
        assert len(np.unique(p, axis=0)) < M, "no two distinct points share their float32 coordinates"
        if M > 4:
            x = torch.from_numpy(p).to(device)
            assert _tie_shares(x, [3], True)[3] > 0, "no equal float32 distances"
    return Case("offset", torch.from_numpy(p), check)


def underflow(M, seed=0) -> Case:
    rng = np.random.default_rng([seed, M, 7])
    g = 1
    while g ** 3 < M:
        g += 1
    grid = np.stack(np.meshgrid(np.arange(g), np.arange(g), np.arange(g), indexing="ij"), -1).reshape(-1, 3)
    p = (_shuffled(rng, grid)[:M] * 1e-30).astype(np.float32)

    def check(device="cpu"):
        assert len(np.unique(p, axis=0)) == M
        x = torch.from_numpy(p).to(device)
        assert bool((_dist_f32(x[:1024], x) == 0).all()), "a float32 distance inside the cluster is not 0"
        if M > 1:
            assert bool((exhaustive_f64(x, x, 1, exclude_self=True) > 0).all())
    return Case("underflow", torch.from_numpy(p), check)


OVERFLOW_SMALL = 5      # points in the first cluster: every K above it needs neighbours at distance +inf


def overflow(M, seed=0) -> Case:
    """two clusters 4e19 apart along x, 5 points in the first and M - 5 in the second (M = 10: 5 and 5)"""
    assert M >= 2 * OVERFLOW_SMALL
    rng = np.random.default_rng([seed, M, 8])
    p = (rng.integers(-64, 65, (M, 3)) * 1e15).astype(np.float32)
    first = np.zeros(M, bool)
    first[rng.choice(M, OVERFLOW_SMALL, replace=False)] = True
    p[:, 0] += np.where(first, np.float32(-2e19), np.float32(2e19)).astype(np.float32)

    def check(device="cpu"):
        assert np.isfinite(p).all()
        x = torch.from_numpy(p).to(device)
        d = _dist_f32(x[torch.from_numpy(first).to(device)], x)
        other = torch.from_numpy(~first).to(device)
        assert bool(torch.isinf(d[:, other]).all()) and bool(torch.isfinite(d[:, ~other]).all())
        i, v = exhaustive_f32(x, x, 8)
        assert bool(((i >= 0) & (i < M)).all())
        rows = torch.from_numpy(first).to(device)
        assert bool(torch.isinf(v[rows][:, OVERFLOW_SMALL:]).all()) and bool(torch.isfinite(v[rows][:, :OVERFLOW_SMALL]).all())
        far = torch.from_numpy(np.flatnonzero(~first)[:8 - OVERFLOW_SMALL]).to(device)
        assert torch.equal(i[rows][:, OVERFLOW_SMALL:], far.expand(OVERFLOW_SMALL, -1)), "infinite distances are ordered by index"
    return Case("overflow", torch.from_numpy(p), check)


CLASSES = {
    "uniform": uniform,
    "lattice": lattice,
    "coincident": coincident,
    "planar_0": lambda M, seed=0: planar(M, seed, 0.0),
    "planar_7.25": lambda M, seed=0: planar(M, seed, 7.25),
    "collinear_0": lambda M, seed=0: collinear(M, seed, 0.0),
    "collinear_7.25": lambda M, seed=0: collinear(M, seed, 7.25),
    "one_cell": one_cell,
    "repeats": repeats,
    "offset": offset,
    "underflow": underflow,
    "overflow": overflow,
    "signed_zero": signed_zero,
}


def make_case(name: str, M: int, seed: int = 0) -> Case:
    return CLASSES[name](M, seed)
