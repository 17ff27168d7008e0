"""HDBSCAN* restated in numpy float64 (the always-present yardstick of tests/test_clustering*.py) and the planted generators.

One definition, always from the float32 / packed inputs:
  euclidean  d(i, j) = sqrt(sum_c (x_ic - x_jc)^2), evaluated in float64.
  jaccard    d(i, j) = float32(1 - I / (|a| + |b| - I + 1e-6)) with integer counts, the expression in float64, rounded once.
  core_i     the core_k-th smallest d(i, j) over all j, j = i included.
  w(i, j)    max(core_i, core_j, d(i, j)); the tree is Prim's over the dense matrix.
  labels     edges sorted by weight (ties in the given order, or shuffled by `tie_rng`), the single-linkage hierarchy with ONE node
             per component and distinct weight (all edges of a weight join at once), condensed with min_cluster_size, stabilities,
             excess of mass, cluster_selection_epsilon, allow_single_cluster; noise -1, clusters numbered by ascending smallest member.
             A binary merge tree (scikit-learn's) is the same hierarchy when no two weights are equal; with equal weights its result
             depends on the order of the equal edges -- at the points that join a cluster at the very weight at which it splits off --
             and scikit-learn's own partition changes when the rows are permuted (tests/test_clustering_host.py).
Written from the algorithm (Campello et al.; behaviour checked against scikit-learn in tests/test_clustering_host.py)."""
import functools

import numpy as np


# ---- distances ------------------------------------------------------------------------------------------------------------------
def euclidean_matrix(points):
    x = np.asarray(points, np.float32).astype(np.float64)
    n, C = x.shape
    d2 = np.zeros((n, n))
    for c in range(C):   # channel by channel: n x n at a time, and exactly 0 for equal rows
        d2 += np.subtract.outer(x[:, c], x[:, c]) ** 2
    return np.sqrt(d2)


def unpack_bits(words):
    """(n, Wd) uint32 / int32 -> (n, 32 Wd) uint8, bit k of word w at column 32 w + k."""
    w = np.ascontiguousarray(np.asarray(words).astype(np.uint32, copy=False)).astype("<u4")
    return np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")


def pack_bits(bits):
    b = np.asarray(bits).astype(np.uint8)
    n, B = b.shape
    pad = (-B) % 32
    b = np.concatenate([b, np.zeros((n, pad), np.uint8)], axis=1)
    return np.packbits(b, axis=1, bitorder="little").view("<u4").astype(np.uint32)


def jaccard_matrix(words):
    bits = unpack_bits(words).astype(np.float32)     # counts stay below 2^24: exact
    inter = (bits @ bits.T).astype(np.float64)
    cnt = bits.sum(1).astype(np.float64)
    d = 1.0 - inter / (cnt[:, None] + cnt[None, :] - inter + 1e-6)
    return d.astype(np.float32).astype(np.float64)


def distance_matrix(points, metric):
    return euclidean_matrix(points) if metric == "euclidean" else jaccard_matrix(points)


def core_distances(D, core_k):
    return np.partition(D, core_k - 1, axis=1)[:, core_k - 1]


def mutual_reachability(D, core):
    return np.maximum(np.maximum(core[:, None], core[None, :]), D)


def prim_mst(W):
    """Prim's algorithm over a dense symmetric matrix: (a, b, w), n - 1 edges."""
    n = W.shape[0]
    a, b, w = np.zeros(n - 1, np.int64), np.zeros(n - 1, np.int64), np.zeros(n - 1)
    inside = np.zeros(n, bool)
    inside[0] = True
    best, src = W[0].copy(), np.zeros(n, np.int64)
    best[0] = np.inf
    for k in range(n - 1):
        j = int(np.argmin(best))
        a[k], b[k], w[k] = src[j], j, best[j]
        inside[j] = True
        best[j] = np.inf
        closer = (W[j] < best) & ~inside
        best[closer], src[closer] = W[j][closer], j
    return a, b, w


# ---- from the tree to labels ----------------------------------------------------------------------------------------------------
def labels_from_mst(n, ea, eb, ew, min_cluster_size, epsilon=0.0, allow_single_cluster=False, tie_rng=None, border=None):
    """`border` (bool array, optional) receives the points that left a cluster at the very weight at which it split."""
    ea, eb, ew = np.asarray(ea), np.asarray(eb), np.asarray(ew, np.float64)
    out = np.full(n, -1, np.int64)
    if n < min_cluster_size or n < 2:
        return out
    idx = np.arange(n - 1) if tie_rng is None else tie_rng.permutation(n - 1)
    idx = idx[np.argsort(ew[idx], kind="stable")]
    # single-linkage hierarchy by levels: all edges of one weight are one level; a node is one component at one level and has every
    # component that level joins as a child, so the order of equal edges (and which minimum spanning tree came in) cannot matter
    up, node_of = list(range(n)), list(range(n))
    kids, size, dist = [[] for _ in range(n)], [1] * n, [0.0] * n

    def find(x):
        r = x
        while up[r] != r:
            r = up[r]
        while up[x] != r:
            up[x], x = r, up[x]
        return r

    k = 0
    while k < n - 1:
        k2 = k
        while k2 < n - 1 and ew[idx[k2]] == ew[idx[k]]:
            k2 += 1
        merged = {}                       # new root -> the nodes it swallows at this level
        for e in idx[k:k2]:
            ra, rb = find(int(ea[e])), find(int(eb[e]))
            assert ra != rb, "not a tree"
            group = merged.pop(ra, [node_of[ra]]) + merged.pop(rb, [node_of[rb]])
            up[ra] = rb
            merged[rb] = group
        for r, group in merged.items():
            node_of[r] = len(kids)
            kids.append(group)
            size.append(sum(size[g] for g in group))
            dist.append(float(ew[idx[k]]))
        k = k2
    # condensed tree: clusters as dicts, points remember where and when they fell out
    cl = [dict(parent=-1, birth=0.0, stab=0.0, kids=[])]
    p_cluster, p_lambda, p_border = np.zeros(n, np.int64), np.zeros(n), np.zeros(n, bool)

    def leaves(top):
        todo, pts = [top], []
        while todo:
            v = todo.pop()
            if v < n:
                pts.append(v)
            else:
                todo += kids[v]
        return pts

    todo = [(node_of[find(0)], 0)]
    while todo:
        node, c = todo.pop()
        lam = 1.0 / dist[node] if dist[node] > 0 else np.inf
        big = [s for s in kids[node] if size[s] >= min_cluster_size]
        for s in kids[node]:
            if size[s] < min_cluster_size:
                pts = leaves(s)
                p_cluster[pts], p_lambda[pts], p_border[pts] = c, lam, len(big) >= 2
                cl[c]["stab"] += (lam - cl[c]["birth"]) * len(pts)
            elif len(big) == 1:
                todo.append((s, c))
            else:
                cl[c]["stab"] += (lam - cl[c]["birth"]) * size[s]
                cl[c]["kids"].append(len(cl))
                cl.append(dict(parent=c, birth=lam, stab=0.0, kids=[]))
                todo.append((s, len(cl) - 1))
    if border is not None:
        border[:] = p_border
    # excess of mass
    nc = len(cl)
    chosen = [False] * nc
    with np.errstate(invalid="ignore"):
        for c in range(nc - 1, -1, -1):
            if c == 0 and not allow_single_cluster:
                break
            below = sum(cl[k]["stab"] for k in cl[c]["kids"])
            if below > cl[c]["stab"]:
                cl[c]["stab"] = below
            else:
                chosen[c] = True

    def keep_topmost(flags):
        covered = [False] * nc
        for c in range(1, nc):
            covered[c] = covered[cl[c]["parent"]] or flags[cl[c]["parent"]]
            if covered[c]:
                flags[c] = False

    keep_topmost(chosen)
    if epsilon != 0.0 and nc > 1 and not chosen[0]:
        with np.errstate(divide="ignore"):
            eps_of = [np.inf if c == 0 else 1.0 / np.float64(cl[c]["birth"]) for c in range(nc)]
        nxt = [False] * nc
        for c in range(1, nc):
            if not chosen[c]:
                continue
            cur = c
            if eps_of[c] < epsilon:
                while True:
                    p = cl[cur]["parent"]
                    if p == 0:
                        cur = 0 if allow_single_cluster else cur
                        break
                    cur = p
                    if eps_of[p] > epsilon:
                        break
            nxt[cur] = True
        chosen = nxt
        keep_topmost(chosen)
    if chosen[0]:
        if epsilon != 0.0:
            thr = 1.0 / epsilon
        else:
            thr = max([p_lambda[i] for i in range(n) if p_cluster[i] == 0] + [cl[k]["birth"] for k in cl[0]["kids"]] + [0.0])
        out[p_lambda >= thr] = 0
        return out
    number = {}
    for i in range(n):
        c = int(p_cluster[i])
        while c >= 0 and not chosen[c]:
            c = cl[c]["parent"]
        if c >= 0:
            out[i] = number.setdefault(c, len(number))
    return out


def mst(points, metric, core_k):
    """(a, b, w, core, D) of the restatement."""
    D = distance_matrix(points, metric)
    core = core_distances(D, core_k)
    a, b, w = prim_mst(mutual_reachability(D, core)) if len(D) > 1 else (np.zeros(0, np.int64),) * 2 + (np.zeros(0),)
    return a, b, w, core, D


def labels(points, metric, min_cluster_size, core_k=None, epsilon=0.0, allow_single_cluster=False, tie_rng=None, tree=None):
    a, b, w = (tree or mst(points, metric, core_k or min_cluster_size))[:3]
    return labels_from_mst(len(points), a, b, w, min_cluster_size, epsilon, allow_single_cluster, tie_rng)


def same_partition(x, y):
    """Equal noise sets and a one-to-one renaming of the cluster numbers."""
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != y.shape or not np.array_equal(x < 0, y < 0):
        return False
    pairs = set(zip(x[x >= 0].tolist(), y[y >= 0].tolist()))
    return len(pairs) == len({p[0] for p in pairs}) == len({p[1] for p in pairs})


# ---- planted data ---------------------------------------------------------------------------------------------------------------
def planted(n, C, k, seed, with_truth=False):
    """k centres on the unit sphere, (n - int(0.15 n)) // k members each at centre + 0.05 N(0, I), the rest N(0, I) background; all
    rows normalised, permuted, float32."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(k, C))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    per = (n - int(0.15 * n)) // k
    rows = [centres[j] + 0.05 * rng.normal(size=(per, C)) for j in range(k)]
    rows.append(rng.normal(size=(n - per * k, C)))
    truth = np.concatenate([np.full(per, j) for j in range(k)] + [np.full(n - per * k, -1)])
    x = np.concatenate(rows)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    perm = rng.permutation(n)
    x, truth = x[perm].astype(np.float32), truth[perm]
    return (x, truth) if with_truth else x


def planted_bits(n, k, seed, bits=1024, on=200, flip=0.05):
    """k prototypes with `on` of `bits` bits set, members with 5 % of the bits flipped, 15 % uniformly random rows; packed uint32."""
    rng = np.random.default_rng(seed)
    protos = np.zeros((k, bits), bool)
    for j in range(k):
        protos[j, rng.choice(bits, on, replace=False)] = True
    per = (n - int(0.15 * n)) // k
    rows = [protos[j][None] ^ (rng.random((per, bits)) < flip) for j in range(k)]
    rows.append(rng.random((n - per * k, bits)) < 0.5)
    x = np.concatenate(rows)[rng.permutation(n)]
    return pack_bits(x)


# (n, C, k, min_cluster_size, epsilon): the configurations the planted checks run on, each with seeds 0..3
EUCLID_CONFIGS = [(300, 32, 4, 10, 0.01), (700, 32, 6, 10, 0.01), (1500, 32, 8, 10, 0.01), (700, 5, 5, 10, 0.0), (700, 32, 6, 30, 0.25)]
# (n, k, min_cluster_size, epsilon) on 1024 bits: the GUI's parameters and the notebook's
JACCARD_CONFIGS = [(300, 4, 10, 0.01), (700, 6, 30, 0.25)]
GPU_SEEDS = (0, 1)


@functools.lru_cache(maxsize=None)
def planted_case(metric, config, seed):
    """(points, tree of the restatement, labels of the restatement) -- computed once, shared by the tests, never modified."""
    if metric == "euclidean":
        n, C, k, mcs, eps = config
        pts = planted(n, C, k, seed)
    else:
        n, k, mcs, eps = config
        pts = planted_bits(n, k, seed)
    tree = mst(pts, metric, mcs)
    lab = labels_from_mst(n, *tree[:3], mcs, eps)
    for arr in (pts, lab) + tree:
        arr.setflags(write=False)
    return pts, tree, lab
