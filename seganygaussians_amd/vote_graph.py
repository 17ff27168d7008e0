"""The language-segmentation vote graph on the MI355X: prompt_segmenting.ipynb's "Language-driven
Segmentation" between the feature render and the Jaccard clustering, and from the clusters to the 3-D query.

  * sam_mask_features() -- per SAM mask, the normalised mean of the scale-gated, normalised rendered features over the mask at the
                           working resolution.  The (M, C, h, w) tensor of the notebook is never formed.
  * anchor_bits()       -- which anchor Gaussians each mask's feature selects (> threshold), written as the pack_bits words that
                           clustering.hdbscan_labels(metric="jaccard") reads.  The (M, A, C) tensor is never formed.
  * clip_relevancy()    -- the template relevancy of CLIP embeddings against positive and negative prompt embeddings.
  * cluster_scores(), cluster_queries() -- plain torch over a few thousand numbers: the mean score per cluster and the notebook's
                           choice of query features and scales.

The CLIP and SAM networks and the tokenizer stay with the caller; `gates` is scale_gate(q_trans(scales)), which
scale_gate.scale_gates(scales, sq, weight, bias) gives in one launch.
No autograd: inputs that require grad are refused while grad mode is on.  There is no CPU fallback for the device parts."""
from __future__ import annotations

import torch

from . import _lib
from ._args import f32, no_grad_one_gpu, number, size_hw
from ._ffi import check, stream_ptr
from .clustering import MAX_POINTS
from .mask_scales import erode
from .packed_masks import as_packed, mask_dims, row_words

MAX_CHANNELS = 256
MAX_ANCHORS = _lib.MI_VOTE_MAX_ANCHORS     # 32 MI_CLUSTER_MAX_WORDS
MAX_EMBED_DIM = _lib.MI_VOTE_MAX_EMBED_DIM
MAX_PROMPTS = _lib.MI_VOTE_MAX_PROMPTS


def _f32_matrix(who: str, name: str, t, rows=None, cols=None) -> None:
    f32(who, name, t)
    if t.dim() != 2 or (rows is not None and t.shape[0] != rows) or (cols is not None and t.shape[1] != cols):
        want = f"({'rows' if rows is None else rows}, {'cols' if cols is None else cols})"
        raise ValueError(f"{who}: {name} must be {want}, got {tuple(t.shape)}")


def sam_mask_features(rendered: torch.Tensor, masks, gates: torch.Tensor, size=None, min_sum: float = 2.0, return_counts: bool = False):
    """The notebook's per-view mask descriptors.

    rendered: float32 (C, H, W) on a GPU, as render_contrastive_feature(..., norm_point_features=True) returns it, 1 <= C <= 256.
    masks: bool (M, hm, wm) on the CPU or that GPU, or a PackedSamMasks on it.  gates: float32 (M, C), scale_gate(q_trans(scales))
    (scale_gate.scale_gates).  size: the working resolution (h, w), default (H // 4, W // 4).  With f_p the bilinear sample (align_corners=False) of rendered
    at working pixel p and b_m the masks resampled to (h, w) and eroded (erode_sam_masks(masks, size, min_sum)):

        s_m = sum_{p in b_m} (g_m * f_p) / max(|g_m * f_p|, 1e-12) / (n_m + 1e-9),      row m = s_m / max(|s_m|, 1e-12)

    Returns float32 (M, C); an empty mask gives a zero row.  With return_counts, also n_m as int64 (M,).  The same inputs give the
    same bits on any stream."""
    who = "sam_mask_features"
    f32(who, "rendered", rendered)
    if rendered.dim() != 3:
        raise ValueError(f"{who}: rendered must be (C, H, W), got {tuple(rendered.shape)}")
    C, H, W = (int(v) for v in rendered.shape)
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError(f"{who}: need 1 <= C <= {MAX_CHANNELS} channels, got {C}")
    if H < 1 or W < 1 or C * H * W >= 1 << 31:
        raise ValueError(f"{who}: need a non-empty render of fewer than 2^31 values, got {(C, H, W)}")
    h, w = size_hw(who, (H // 4, W // 4) if size is None else size)
    if C * h * w >= 1 << 31:
        raise ValueError(f"{who}: more than 2^31 values at the working resolution {(h, w)}")
    min_sum = number(who, "min_sum", min_sum)
    M = mask_dims(who, masks)[0]   # not check_shape: the masks' own size has no pixel limit here
    _f32_matrix(who, "gates", gates, M, C)
    dev = no_grad_one_gpu(who, [("rendered", rendered), ("gates", gates)])
    packed = as_packed(who, masks, dev)
    if M * h * row_words(w) >= 1 << 31:
        raise ValueError(f"{who}: more than 2^31 mask words")
    L = _lib.load()
    rendered, gates = rendered.detach().contiguous(), gates.detach().contiguous()
    with torch.cuda.device(dev):
        eroded = erode(packed, h, w, min_sum)
        nbytes = int(L.mi_vote_mask_features_workspace_bytes(M, C, h, w))
        ws = torch.empty(nbytes // 8 + 1, device=dev, dtype=torch.int64)
        out = torch.empty((M, C), device=dev, dtype=torch.float32)
        counts = torch.empty((M,), device=dev, dtype=torch.int64)
        check(L.mi_vote_mask_features(M, C, H, W, rendered.data_ptr(), h, w, eroded.words.data_ptr(), gates.data_ptr(), ws.data_ptr(),
                                      nbytes, out.data_ptr(), counts.data_ptr(), stream_ptr(dev)))
    return (out, counts) if return_counts else out


def anchor_bits(mask_features: torch.Tensor, gates: torch.Tensor, anchor_features: torch.Tensor, threshold: float = 0.5,
                out: torch.Tensor = None, row_offset: int = 0, return_counts: bool = False):
    """Which anchors each mask selects: bit a of row m = <normalize(g_m * a_a), phi_m> > threshold (strict; a NaN is not greater).

    mask_features (phi), gates: float32 (M, C).  anchor_features: float32 (A, C), raw point features, 1 <= A <= 32768.
    Returns int32 (M, ceil(A / 32)) in the pack_bits layout (bit k of word w = anchor 32 w + k, bits past A zero), the input of
    hdbscan_labels(metric="jaccard").  out: a contiguous int32 (M_total, ceil(A / 32)) tensor to fill instead, rows
    row_offset .. row_offset + M - 1 (the view of those rows is returned), so that a scene is filled view by view.
    With return_counts, also the set bits per row as int32 (M,)."""
    who = "anchor_bits"
    _f32_matrix(who, "mask_features", mask_features)
    M, C = int(mask_features.shape[0]), int(mask_features.shape[1])
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError(f"{who}: need 1 <= C <= {MAX_CHANNELS} channels, got {C}")
    if not 1 <= M <= MAX_POINTS:
        raise ValueError(f"{who}: need 1 <= M <= {MAX_POINTS} rows, got {M}")
    _f32_matrix(who, "gates", gates, M, C)
    _f32_matrix(who, "anchor_features", anchor_features, None, C)
    A = int(anchor_features.shape[0])
    if not 1 <= A <= MAX_ANCHORS:
        raise ValueError(f"{who}: need 1 <= A <= {MAX_ANCHORS} anchors, got {A}")
    threshold = number(who, "threshold", threshold)
    words = (A + 31) // 32
    if not isinstance(row_offset, int) or isinstance(row_offset, bool):
        raise ValueError(f"{who}: row_offset must be an integer, got {row_offset!r}")
    tensors = [("mask_features", mask_features), ("gates", gates), ("anchor_features", anchor_features)]
    if out is None:
        if row_offset != 0:
            raise ValueError(f"{who}: row_offset without out")
    else:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or out.dim() != 2 or out.shape[1] != words:
            raise ValueError(f"{who}: out must be int32 (M_total, {words}), got {getattr(out, 'dtype', type(out))} "
                             f"{tuple(getattr(out, 'shape', ()))}")
        if not out.is_contiguous():
            raise ValueError(f"{who}: out must be contiguous")
        if out.shape[0] > MAX_POINTS:
            raise ValueError(f"{who}: out has more than {MAX_POINTS} rows")
        if not 0 <= row_offset <= out.shape[0] - M:
            raise ValueError(f"{who}: rows {row_offset} .. {row_offset + M - 1} do not lie in out's {out.shape[0]} rows")
        tensors.append(("out", out))
    dev = no_grad_one_gpu(who, tensors)
    L = _lib.load()
    phi, gates, anchors = mask_features.detach().contiguous(), gates.detach().contiguous(), anchor_features.detach().contiguous()
    with torch.cuda.device(dev):
        rows = torch.empty((M, words), device=dev, dtype=torch.int32) if out is None else out[row_offset:row_offset + M]
        counts = torch.empty((M,), device=dev, dtype=torch.int32) if return_counts else None
        check(L.mi_vote_anchor_bits(M, A, C, phi.data_ptr(), gates.data_ptr(), anchors.data_ptr(), threshold, rows.data_ptr(),
                                    None if counts is None else counts.data_ptr(), stream_ptr(dev)))
    return (rows, counts) if return_counts else rows


def clip_relevancy(embeds: torch.Tensor, pos_embeds: torch.Tensor, neg_embeds: torch.Tensor, normalize: bool = True) -> torch.Tensor:
    """The notebook's template relevancy: out[n, p] = min_q softmax(10 [e_n . pos_p, e_n . neg_q])[0]
    = 1 / (1 + exp(10 (max_q e_n . neg_q - e_n . pos_p))).

    embeds: float32 or float16 (N, D), 1 <= D <= 1024; with normalize, e_n = row.float() / max(|row|, 1e-12).  pos_embeds float32
    (P, D), neg_embeds float32 (Q, D), used as given, 1 <= P, Q <= 16.  Returns float32 (N, P)."""
    who = "clip_relevancy"
    if not isinstance(embeds, torch.Tensor) or embeds.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"{who}: embeds must be a float32 or float16 tensor, got {getattr(embeds, 'dtype', type(embeds))}")
    if embeds.dim() != 2:
        raise ValueError(f"{who}: embeds must be (N, D), got {tuple(embeds.shape)}")
    N, D = int(embeds.shape[0]), int(embeds.shape[1])
    if not 1 <= D <= MAX_EMBED_DIM:
        raise ValueError(f"{who}: need 1 <= D <= {MAX_EMBED_DIM}, got {D}")
    if not 1 <= N < 1 << 31:
        raise ValueError(f"{who}: need 1 <= N < 2^31 rows, got {N}")
    _f32_matrix(who, "pos_embeds", pos_embeds, None, D)
    _f32_matrix(who, "neg_embeds", neg_embeds, None, D)
    P, Q = int(pos_embeds.shape[0]), int(neg_embeds.shape[0])
    if not (1 <= P <= MAX_PROMPTS and 1 <= Q <= MAX_PROMPTS):
        raise ValueError(f"{who}: need 1 <= P, Q <= {MAX_PROMPTS} prompt embeddings, got P = {P}, Q = {Q}")
    dev = no_grad_one_gpu(who, [("embeds", embeds), ("pos_embeds", pos_embeds), ("neg_embeds", neg_embeds)])
    L = _lib.load()
    embeds, pos, neg = embeds.detach().contiguous(), pos_embeds.detach().contiguous(), neg_embeds.detach().contiguous()
    out = torch.empty((N, P), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        check(L.mi_vote_relevancy(N, D, P, Q, embeds.data_ptr(), 1 if embeds.dtype == torch.float16 else 0, pos.data_ptr(),
                                  neg.data_ptr(), 1 if normalize else 0, out.data_ptr(), stream_ptr(dev)))
    return out


def _scores_and_labels(who: str, scores, labels):
    if not isinstance(scores, torch.Tensor) or not scores.is_floating_point() or scores.dim() != 1:
        raise ValueError(f"{who}: scores must be a floating (n,) tensor, got {getattr(scores, 'dtype', type(scores))} "
                         f"{tuple(getattr(scores, 'shape', ()))}")
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or labels.shape != scores.shape:
        raise ValueError(f"{who}: labels must be int64 ({scores.shape[0]},), got {getattr(labels, 'dtype', type(labels))} "
                         f"{tuple(getattr(labels, 'shape', ()))}")
    if labels.device != scores.device:
        raise ValueError(f"{who}: labels are on {labels.device}, the scores on {scores.device}")
    if labels.numel() and int(labels.min().item()) < -1:
        raise ValueError(f"{who}: labels must be >= -1")


def _group_means(scores, labels):
    K = int(labels.max().item()) + 1 if labels.numel() else 0
    sums = scores.new_zeros(K + 1).index_add_(0, labels + 1, scores.detach())
    sizes = torch.bincount(labels + 1, minlength=K + 1)
    return sums / sizes.to(scores.dtype), sizes   # 0 / 0 = NaN for a group without members


def cluster_scores(scores: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """The mean score per label of hdbscan_labels, noise first: entry 0 is the mean over the noise rows (label -1), entry k + 1 that
    of cluster k; K + 1 entries.  The noise entry is NaN when no row is noise.  Plain torch, on the scores' device."""
    _scores_and_labels("cluster_scores", scores, labels)
    return _group_means(scores, labels)[0]


def cluster_queries(scores: torch.Tensor, labels: torch.Tensor, mask_features: torch.Tensor, mask_scales: torch.Tensor,
                    min_score: float = 0.45):
    """The notebook's selection of 3-D queries.  The groups are the clusters and, as in the notebook, the noise rows (id -1): those
    whose mean score exceeds min_score are taken, or the single best one if none does.  Of each, the member with the highest score
    (the first among equals) gives the query feature, re-normalised, and the scale.

    scores (n,), labels int64 (n,), mask_features (n, C), mask_scales (n,) or (n, 1), on one device.
    Returns (queries (G, C), scales (G,), cluster_ids int64 (G,), cluster_means (G,)) in ascending id."""
    who = "cluster_queries"
    _scores_and_labels(who, scores, labels)
    n = int(scores.shape[0])
    if n < 1:
        raise ValueError(f"{who}: no rows")
    if not isinstance(mask_features, torch.Tensor) or not mask_features.is_floating_point() or mask_features.dim() != 2 \
            or mask_features.shape[0] != n:
        raise ValueError(f"{who}: mask_features must be a floating ({n}, C) tensor, got {getattr(mask_features, 'dtype', type(mask_features))} "
                         f"{tuple(getattr(mask_features, 'shape', ()))}")
    if not isinstance(mask_scales, torch.Tensor) or mask_scales.numel() != n or mask_scales.dim() > 2:
        raise ValueError(f"{who}: mask_scales must hold {n} values, got {tuple(getattr(mask_scales, 'shape', ()))}")
    if mask_features.device != scores.device or mask_scales.device != scores.device:
        raise ValueError(f"{who}: all tensors must be on {scores.device}")
    means, sizes = _group_means(scores, labels)
    ranked = torch.where(sizes > 0, means, torch.full_like(means, float("-inf")))
    good = torch.nonzero(ranked > float(min_score)).flatten()
    if good.numel() == 0:
        good = ranked.argmax().reshape(1)
    ids = good - 1
    rows = []
    for g in ids.tolist():
        members = torch.nonzero(labels == g).flatten()
        best = scores[members].max()
        rows.append(members[scores[members] == best][0])   # the first among equal maxima
    rows = torch.stack(rows)
    queries = torch.nn.functional.normalize(mask_features.detach()[rows], dim=-1)
    return queries, mask_scales.detach().reshape(n)[rows], ids, means[good]
