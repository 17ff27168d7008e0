"""Exact HDBSCAN* on the MI355X: where the centres of segmentation.assign_clusters come from
(saga_gui.py:518-543 `cluster_in_3D`, the notebook's "Cluster in 3D / 2D" and its Jaccard cell).

Core distances and the minimum spanning tree of the mutual-reachability graph run on the device (all pairs, the n x n matrix is
never formed); the tree work -- single linkage, condensed tree, excess of mass, cluster_selection_epsilon -- runs on the host in C++.

  metric="euclidean": points float32 (n, C), 1 <= C <= 256; d = sqrt(sum_c (x_c - y_c)^2) in binary32, difference form.
  metric="jaccard":   points int32 (n, Wd) from pack_bits(), 1 <= Wd <= 1024 words of 32 bits;
                      d = float32(1 - I / (|a| + |b| - I + 1e-6)) with exact integer counts.
  core_i = the core_k-th smallest d(i, j) over all j, j = i INCLUDED (scikit-learn's min_samples).  The `hdbscan` package is not a
  dependency and its own convention was not checked against: a caller who needs "self not counted" passes core_k = min_samples + 1.
  edge weight max(core_i, core_j, d(i, j)); labels: noise -1, clusters 0 .. K-1 by ascending smallest member index.

Not provided: membership probabilities, outlier scores, leaf selection, approximate prediction, metric="precomputed".  No autograd;
there is no CPU fallback for the device parts."""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._args import no_grad_one_gpu, to_float
from ._ffi import check, stream_ptr

METRICS = _lib.MI_CLUSTER_METRIC
MAX_POINTS = _lib.MI_CLUSTER_MAX_POINTS
MAX_CHANNELS = _lib.MI_CLUSTER_MAX_CHANNELS
MAX_WORDS = _lib.MI_CLUSTER_MAX_WORDS
MAX_CORE_K = _lib.MI_CLUSTER_MAX_CORE_K


def pack_bits(bool_matrix: torch.Tensor) -> torch.Tensor:
    """(n, B) bool / 0-1 integer matrix -> int32 (n, ceil(B / 32)): bit k of word w is column 32 w + k, bits past B are zero.
    Plain torch, on the matrix's device."""
    if not isinstance(bool_matrix, torch.Tensor) or bool_matrix.dim() != 2 or bool_matrix.is_floating_point() or bool_matrix.is_complex():
        raise ValueError(f"pack_bits: need an (n, B) bool or integer tensor, got {getattr(bool_matrix, 'dtype', type(bool_matrix))} "
                         f"{tuple(getattr(bool_matrix, 'shape', ()))}")
    n, B = int(bool_matrix.shape[0]), int(bool_matrix.shape[1])
    if B < 1 or B > 32 * MAX_WORDS:
        raise ValueError(f"pack_bits: need 1 <= B <= {32 * MAX_WORDS} bits, got {B}")
    words = (B + 31) // 32
    bits = torch.zeros((n, words * 32), dtype=torch.int64, device=bool_matrix.device)
    bits[:, :B] = (bool_matrix != 0).to(torch.int64)
    weights = torch.ones(32, dtype=torch.int64, device=bool_matrix.device) << torch.arange(32, device=bool_matrix.device)
    return (bits.reshape(n, words, 32) * weights).sum(-1).to(torch.int32)   # the cast keeps the low 32 bits


def _check_params(who, min_cluster_size, cluster_selection_epsilon, n=1):
    if not isinstance(min_cluster_size, int) or isinstance(min_cluster_size, bool) or min_cluster_size < 2:
        raise ValueError(f"{who}: min_cluster_size must be an integer >= 2, got {min_cluster_size!r}")
    eps = to_float(who, "cluster_selection_epsilon", cluster_selection_epsilon)
    if not eps >= 0.0 or eps == float("inf"):
        raise ValueError(f"{who}: cluster_selection_epsilon must be finite and >= 0, got {cluster_selection_epsilon!r}")
    if not 1 <= n <= MAX_POINTS:
        raise ValueError(f"{who}: need 1 <= n <= {MAX_POINTS} points, got {n}")
    return eps


def _prepare(who: str, points, core_k, metric):
    """Everything that can be checked without a device; returns (points contiguous, metric id, n, width)."""
    if metric not in METRICS:
        raise ValueError(f"{who}: metric must be one of {sorted(METRICS)}, got {metric!r} "
                         "('precomputed' is the n x n matrix this module avoids)")
    want = torch.float32 if metric == "euclidean" else torch.int32
    if not isinstance(points, torch.Tensor) or points.dtype != want:
        raise ValueError(f"{who}: points must be a {str(want).replace('torch.', '')} tensor for metric={metric!r}"
                         f"{' (see pack_bits)' if metric == 'jaccard' else ''}, got {getattr(points, 'dtype', type(points))}")
    if points.dim() != 2:
        raise ValueError(f"{who}: points must be (n, width), got {tuple(points.shape)}")
    n, width = int(points.shape[0]), int(points.shape[1])
    limit, unit = (MAX_CHANNELS, "channels") if metric == "euclidean" else (MAX_WORDS, "words")
    if not 1 <= width <= limit:
        raise ValueError(f"{who}: need 1 <= width <= {limit} {unit}, got {width}")
    if not 1 <= n <= MAX_POINTS:
        raise ValueError(f"{who}: need 1 <= n <= {MAX_POINTS} points, got {n}")
    if not isinstance(core_k, int) or isinstance(core_k, bool) or not 1 <= core_k <= MAX_CORE_K:
        raise ValueError(f"{who}: core_k must be an integer in 1..{MAX_CORE_K}, got {core_k!r}")
    if core_k > n:
        raise ValueError(f"{who}: need n >= core_k, got n = {n}, core_k = {core_k}")
    no_grad_one_gpu(who, [("points", points)])
    return points.detach().contiguous(), METRICS[metric], n, width


def _workspace(L, mid, n, width, core_k, dev):
    nbytes = int(L.mi_cluster_workspace_bytes(mid, n, width, core_k))
    if nbytes == 0:
        raise RuntimeError("clustering: the library refuses these sizes")
    return torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=dev), nbytes


def _core(L, points, mid, n, width, core_k, ws, nbytes):
    core = torch.empty(n, dtype=torch.float32, device=points.device)
    check(L.mi_cluster_core_distances(mid, n, width, points.data_ptr(), core_k, core.data_ptr(), ws.data_ptr(), nbytes,
                                      stream_ptr(points.device)))
    return core


def _mst(L, points, mid, n, width, core, ws, nbytes):
    dev = points.device
    ea = torch.empty(n - 1, dtype=torch.int32, device=dev)
    eb = torch.empty(n - 1, dtype=torch.int32, device=dev)
    ew = torch.empty(n - 1, dtype=torch.float32, device=dev)
    if n > 1:
        check(L.mi_cluster_mst(mid, n, width, points.data_ptr(), core.data_ptr(), ea.data_ptr(), eb.data_ptr(), ew.data_ptr(),
                               ws.data_ptr(), nbytes, stream_ptr(dev)))
    return ea, eb, ew


def core_distances(points: torch.Tensor, core_k: int, metric: str = "euclidean") -> torch.Tensor:
    """float32 (n,): the core_k-th smallest distance from every row to all rows, itself included."""
    points, mid, n, width = _prepare("core_distances", points, core_k, metric)
    L = _lib.load()
    with torch.cuda.device(points.device):
        ws, nbytes = _workspace(L, mid, n, width, core_k, points.device)
        return _core(L, points, mid, n, width, core_k, ws, nbytes)


def mutual_reachability_mst(points: torch.Tensor, core_k: int, metric: str = "euclidean"):
    """(edge_a int32, edge_b int32, edge_w float32), each (n - 1,), on the device: a minimum spanning tree of the complete graph under
    max(core_a, core_b, d(a, b)), a < b.  The same input gives the same edges in the same order."""
    points, mid, n, width = _prepare("mutual_reachability_mst", points, core_k, metric)
    L = _lib.load()
    with torch.cuda.device(points.device):
        ws, nbytes = _workspace(L, mid, n, width, core_k, points.device)
        core = _core(L, points, mid, n, width, core_k, ws, nbytes)
        return _mst(L, points, mid, n, width, core, ws, nbytes)


def labels_from_mst(edge_a: torch.Tensor, edge_b: torch.Tensor, edge_w: torch.Tensor, n: int, min_cluster_size: int,
                    cluster_selection_epsilon: float = 0.0, allow_single_cluster: bool = False) -> torch.Tensor:
    """The host half: CPU tensors in (int32, int32, float32, one entry per edge, in any order), int64 labels (n,) out on the CPU.
    Refuses edges that are not a spanning tree of n points.  Needs no GPU."""
    if not isinstance(n, int) or isinstance(n, bool):
        raise ValueError(f"labels_from_mst: n must be an integer, got {n!r}")
    eps = _check_params("labels_from_mst", min_cluster_size, cluster_selection_epsilon, n)
    for name, t, dtype in (("edge_a", edge_a, torch.int32), ("edge_b", edge_b, torch.int32), ("edge_w", edge_w, torch.float32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 1:
            raise ValueError(f"labels_from_mst: {name} must be a 1-D {str(dtype).replace('torch.', '')} tensor, "
                             f"got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
        if t.is_cuda:
            raise ValueError(f"labels_from_mst: {name} must be a CPU tensor, got {t.device}")
    if not edge_a.numel() == edge_b.numel() == edge_w.numel():
        raise ValueError("labels_from_mst: edge_a, edge_b and edge_w must have one entry per edge each")
    edge_a, edge_b, edge_w = edge_a.contiguous(), edge_b.contiguous(), edge_w.detach().contiguous()
    labels = torch.empty(n, dtype=torch.int32)
    count = ctypes.c_int(0)
    m = int(edge_a.numel())
    rc = _lib.load().mi_cluster_labels_host(n, m, edge_a.data_ptr() if m else None, edge_b.data_ptr() if m else None,
                                            edge_w.data_ptr() if m else None, min_cluster_size, eps, 1 if allow_single_cluster else 0,
                                            labels.data_ptr(), ctypes.byref(count))
    if rc != 0:
        raise ValueError("labels_from_mst: " + _lib.last_error())
    return labels.to(torch.int64)


def hdbscan_labels(points: torch.Tensor, min_cluster_size: int = 10, min_samples: int = None, cluster_selection_epsilon: float = 0.0,
                   allow_single_cluster: bool = False, metric: str = "euclidean", core_k: int = None) -> torch.Tensor:
    """int64 labels (n,) on points.device: -1 for noise, clusters 0 .. K-1 by ascending smallest member index.

    core_k defaults to min_samples, which defaults to min_cluster_size (scikit-learn's convention: the point itself is counted).
    cluster_in_3D (saga_gui.py:529-531) is hdbscan_labels(sample, 10, cluster_selection_epsilon=0.01).  One download of the
    12 (n - 1) bytes of the tree and one upload of the labels; the rest of the device work is asynchronous apart from one 4-byte read
    per Boruvka round."""
    _check_params("hdbscan_labels", min_cluster_size, cluster_selection_epsilon)
    if core_k is None:
        core_k = min_cluster_size if min_samples is None else min_samples
    points, mid, n, width = _prepare("hdbscan_labels", points, core_k, metric)
    L = _lib.load()
    dev = points.device
    with torch.cuda.device(dev):
        ws, nbytes = _workspace(L, mid, n, width, core_k, dev)
        core = _core(L, points, mid, n, width, core_k, ws, nbytes)
        ea, eb, ew = _mst(L, points, mid, n, width, core, ws, nbytes)
        packed = torch.cat([ea.view(torch.uint8), eb.view(torch.uint8), ew.view(torch.uint8)]).cpu()   # the one download
    m = 4 * (n - 1)
    labels = labels_from_mst(packed[:m].view(torch.int32), packed[m:2 * m].view(torch.int32), packed[2 * m:].view(torch.float32), n,
                             min_cluster_size, cluster_selection_epsilon, allow_single_cluster)
    return labels.to(dev)


def cluster_centers(features: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """(K, C): the L2-normalised mean feature of every cluster 0 .. K-1, noise (-1) left out.  Plain torch: the sample is small.

    The GUI's own loop (saga_gui.py:539-540) runs over np.unique(labels), noise included, so its row 0 is the mean of the noise
    points whenever there are any; torch.cat([F.normalize(features[labels == -1].mean(0, keepdim=True), dim=-1), centers]) adds it."""
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or not features.is_floating_point():
        raise ValueError(f"cluster_centers: features must be a floating (n, C) tensor, got {getattr(features, 'dtype', type(features))} "
                         f"{tuple(getattr(features, 'shape', ()))}")
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or labels.shape != features.shape[:1]:
        raise ValueError(f"cluster_centers: labels must be int64 ({features.shape[0]},), got {getattr(labels, 'dtype', type(labels))} "
                         f"{tuple(getattr(labels, 'shape', ()))}")
    if labels.device != features.device:
        raise ValueError(f"cluster_centers: labels are on {labels.device}, the features on {features.device}")
    K = int(labels.max().item()) + 1 if labels.numel() else 0
    if K <= 0:
        return features.new_zeros((0, features.shape[1]))
    member = labels >= 0
    sums = features.new_zeros((K, features.shape[1])).index_add_(0, labels[member], features.detach()[member])
    counts = torch.bincount(labels[member], minlength=K).clamp_(min=1).to(features.dtype)
    return torch.nn.functional.normalize(sums / counts[:, None], dim=-1)


class HDBSCAN:
    """Stand-in for `hdbscan.HDBSCAN` as the reference uses it: numpy in, numpy out; the work runs on the current GPU.

    Only metric='euclidean'.  min_samples follows scikit-learn: the point itself is counted (see the module text)."""

    def __init__(self, min_cluster_size=5, min_samples=None, cluster_selection_epsilon=0.0, allow_single_cluster=False,
                 metric="euclidean", **unsupported):
        if unsupported:
            raise TypeError(f"HDBSCAN: unsupported arguments {sorted(unsupported)}")
        if metric != "euclidean":
            raise ValueError(f"HDBSCAN: only metric='euclidean' is supported here, got {metric!r}; for bit sets use "
                             "seganygaussians_amd.clustering.hdbscan_labels(pack_bits(...), metric=\"jaccard\") -- 'precomputed' is the "
                             "n x n matrix this implementation avoids")
        self.min_cluster_size, self.min_samples = min_cluster_size, min_samples
        self.cluster_selection_epsilon, self.allow_single_cluster, self.metric = cluster_selection_epsilon, allow_single_cluster, metric
        self.labels_ = None

    def fit(self, X, y=None):
        import numpy as np
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2:
            raise ValueError(f"HDBSCAN: X must be (n_samples, n_features), got {X.shape}")
        pts = torch.from_numpy(X).to(torch.device("cuda", torch.cuda.current_device()))
        self.labels_ = hdbscan_labels(pts, int(self.min_cluster_size), None if self.min_samples is None else int(self.min_samples),
                                      self.cluster_selection_epsilon, bool(self.allow_single_cluster)).cpu().numpy()
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_
