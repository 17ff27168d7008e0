"""Scale-gated segmentation queries on the MI355X: similarity scores, selection, cluster assignment.

What a user does with trained affinity features, as three fused device operations over a rendered feature image (C, H, W) or the
per-Gaussian feature table (P, C).  For a feature row f, optional gates g (the scale gate of saga_gui.py:596) and `pre`:

    u = f                       pre="none"   (saga_gui.py:674)
    u = f / max(|f|, 1e-12)     pre="l2"     (F.normalize; cluster_in_3D :526)
    u = f / (|f| + 1e-6)        pre="eps"    (the GUI's image path, :592)
    v = u * g                   (v = u without gates)
    w = v / max(|v|, 1e-12)     F.normalize; skipped with post=False (the PCA image, :593)
    s_k = <w, q_k>              q_k as given, never normalised here

  * similarity_scores()    -- s as (Q, ...) float32.
  * select_by_similarity() -- the GUI's decision (:648-652, :678-679): t = (s + 1) / 2 (half_shift) or s, selected where any
                              t_k > threshold, score = max_k (selected_k ? t_k : 0).  (Q, N) is never written.
  * assign_clusters()      -- arg-max over up to 4096 centres and its value; (N, K) is never formed.

The layout follows features.dim(): 3 -> image (C, H, W), outputs (..., H, W); 2 -> points (P, C), outputs (..., P).  float32 tensors
on one GPU.  No autograd (every use in the reference is under no_grad or detached): inputs that require grad are refused while grad
mode is on.  Non-finite inputs are outside the contract.  There is no CPU fallback."""
from __future__ import annotations

import torch

from . import _lib
from ._args import f32, no_grad_one_gpu, number
from ._ffi import check, ptr, stream_ptr

MAX_CHANNELS = _lib.MI_SEGMENT_MAX_CHANNELS
MAX_QUERIES = _lib.MI_SEGMENT_MAX_QUERIES
MAX_CENTERS = _lib.MI_SEGMENT_MAX_CENTERS
PRE_MODES = _lib.MI_SEGMENT_PRE


def feature_table(who: str, features):
    """(layout, C, N, shape) of a float32 feature image (C, H, W), layout 0, or feature table (P, C), layout 1, within the limits."""
    f32(who, "features", features)
    if features.dim() == 3:
        layout, C, shape = 0, int(features.shape[0]), tuple(int(v) for v in features.shape[1:])
        N = shape[0] * shape[1]
    elif features.dim() == 2:
        layout, C, shape = 1, int(features.shape[1]), (int(features.shape[0]),)
        N = shape[0]
    else:
        raise ValueError(f"{who}: features must be (C, H, W) or (P, C), got {tuple(features.shape)}")
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError(f"{who}: need 1 <= C <= {MAX_CHANNELS} channels, got {C}")
    if not 1 <= N < 1 << 31:
        raise ValueError(f"{who}: need 1 <= N < 2^31 rows, got {N}")
    return layout, C, N, shape


def query_rows(who: str, queries, C: int, max_q: int, qname: str = "queries"):
    """(queries as (Q, C), Q) of float32 (Q, C) or (C,) with 1 <= Q <= max_q."""
    f32(who, qname, queries)
    if queries.dim() == 1:
        queries = queries[None]
    if queries.dim() != 2 or queries.shape[1] != C:
        raise ValueError(f"{who}: {qname} must be (Q, {C}) or ({C},), got {tuple(queries.shape)}")
    Q = int(queries.shape[0])
    if not 1 <= Q <= max_q:
        raise ValueError(f"{who}: need 1 <= {qname} <= {max_q}, got {Q}")
    return queries, Q


def gate_row(who: str, gates, C: int):
    """gates as (C,): float32 with C values in at most two dimensions, or None."""
    if f32(who, "gates", gates, optional=True) is None:
        return None
    if gates.numel() != C or gates.dim() > 2:
        raise ValueError(f"{who}: gates must hold {C} values, got {tuple(gates.shape)}")
    return gates.reshape(C)


def check_pre(who: str, pre) -> None:
    if pre not in PRE_MODES:
        raise ValueError(f"{who}: pre must be one of {sorted(PRE_MODES)}, got {pre!r}")


def _prepare(who: str, features, queries, gates, pre, max_q: int, qname: str):
    """Checks everything that can be checked without a device, then returns (features, queries, gates, layout, N, C, Q, shape) with
    contiguous tensors.  Raises ValueError before any pointer reaches the library."""
    layout, C, N, shape = feature_table(who, features)
    queries, Q = query_rows(who, queries, C, max_q, qname)
    gates = gate_row(who, gates, C)
    check_pre(who, pre)
    no_grad_one_gpu(who, [("features", features), (qname, queries)] + ([("gates", gates)] if gates is not None else []), "features")
    # a non-contiguous input (e.g. a transposed view) is copied once here
    features, queries = features.detach().contiguous(), queries.detach().contiguous()
    gates = None if gates is None else gates.detach().contiguous()
    return features, queries, gates, layout, N, C, Q, shape


def similarity_scores(features: torch.Tensor, queries: torch.Tensor, gates: torch.Tensor = None, pre: str = "none",
                      post: bool = True) -> torch.Tensor:
    """s_k of every row for 1 <= Q <= 16 queries: (Q, H, W) for a (C, H, W) image, (Q, P) for (P, C) points.

    saga_gui.py:592-599 + :645 is similarity_scores(rendered, chosen.T, gates, pre="eps"); :593, the PCA image, is
    similarity_scores(rendered, proj_mat.T, pre="eps", post=False); viewer.viewer_frame() applies clip(x * 0.5 + 0.5, 0, 1) of :594
    to the same chain and composes the display buffer in the one read of the image.
    features: float32 (C, H, W) or (P, C); a non-contiguous tensor is copied.  queries: float32 (Q, C) or (C,), used as given.
    gates: float32, C values, or None."""
    features, queries, gates, layout, N, C, Q, shape = _prepare("similarity_scores", features, queries, gates, pre, MAX_QUERIES, "queries")
    L = _lib.load()
    dev = features.device
    out = torch.empty((Q,) + shape, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        check(L.mi_segment_scores(layout, N, C, Q, features.data_ptr(), queries.data_ptr(), ptr(gates), PRE_MODES[pre],
                                  1 if post else 0, out.data_ptr(), stream_ptr(dev)))
    return out


def select_by_similarity(features: torch.Tensor, queries: torch.Tensor, threshold: float, gates: torch.Tensor = None,
                         pre: str = "none", half_shift: bool = True):
    """The GUI's selection (saga_gui.py:648-652 on the image, :678-679 on the Gaussians) for 1 <= Q <= 16 queries.

    t_k = (s_k + 1) / 2 with half_shift (the GUI), t_k = s_k without (the notebook's `similarities > 0.75`).  Returns
    (mask, score): mask bool = any_k t_k > threshold, score float32 = max_k (t_k > threshold ? t_k : 0), shaped (H, W) or (P,)."""
    features, queries, gates, layout, N, C, Q, shape = _prepare("select_by_similarity", features, queries, gates, pre, MAX_QUERIES, "queries")
    threshold = number("select_by_similarity", "threshold", threshold)
    L = _lib.load()
    dev = features.device
    mask = torch.empty(shape, device=dev, dtype=torch.bool)
    score = torch.empty(shape, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        check(L.mi_segment_select(layout, N, C, Q, features.data_ptr(), queries.data_ptr(), ptr(gates), PRE_MODES[pre],
                                  1 if half_shift else 0, threshold, mask.data_ptr(), score.data_ptr(), stream_ptr(dev)))
    return mask, score


def assign_clusters(features: torch.Tensor, centers: torch.Tensor, gates: torch.Tensor = None, pre: str = "l2"):
    """cluster_in_3D's assignment (saga_gui.py:542-543) and the notebook's "Cluster in 2D / 3D" arg-max for 1 <= K <= 4096 centres.

    Returns (labels, best): labels int32 = argmax_k s_k (the lowest index among equal maxima, as torch.argmax on the CPU), best
    float32 = max_k s_k, shaped (H, W) or (P,).  centers: float32 (K, C), used as given."""
    features, centers, gates, layout, N, C, K, shape = _prepare("assign_clusters", features, centers, gates, pre, MAX_CENTERS, "centers")
    L = _lib.load()
    dev = features.device
    labels = torch.empty(shape, device=dev, dtype=torch.int32)
    best = torch.empty(shape, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        check(L.mi_segment_assign(layout, N, C, K, features.data_ptr(), centers.data_ptr(), ptr(gates), PRE_MODES[pre],
                                  labels.data_ptr(), best.data_ptr(), stream_ptr(dev)))
    return labels, best
