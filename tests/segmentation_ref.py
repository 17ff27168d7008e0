"""CPU restatement of the segmentation queries (include/mi_segment.h) in float64, and the reference's own float32
lines transcribed one for one (literal32_*).  The float64 form is the yardstick of tests/test_segmentation.py; the literal form shows
that the reference itself stays inside the yardstick's band (tests/test_segmentation_host.py).

    u = f | f / max(|f|, 1e-12) | f / (|f| + 1e-6)      pre = "none" | "l2" | "eps"
    v = u * g,  w = v / max(|v|, 1e-12) (post),  s_k = <w, q_k>

Inputs are float32 tensors, converted exactly.  Rows are processed in chunks so that (N, K) never exceeds a few hundred MB."""
import torch

CHUNK_ELEMS = 1 << 24


def rows_of(features):
    """(C, H, W) or (P, C) -> (N, C) view-or-copy and the output shape."""
    if features.dim() == 3:
        C, H, W = features.shape
        return features.reshape(C, H * W).t(), (H, W)
    return features, (features.shape[0],)


def _unit_rows64(rows, gates, pre, post):
    f = rows.double()
    if pre == "l2":
        f = f / f.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    elif pre == "eps":
        f = f / (f.norm(dim=-1, keepdim=True) + 1e-6)
    elif pre != "none":
        raise ValueError(pre)
    if gates is not None:
        f = f * gates.double().reshape(1, -1)
    if post:
        f = f / f.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return f


def _chunks(N, width):
    step = max(1, CHUNK_ELEMS // max(1, width))
    for i in range(0, N, step):
        yield i, min(N, i + step)


def scores64(features, queries, gates=None, pre="none", post=True):
    """float64 (Q,) + shape."""
    rows, shape = rows_of(features)
    q = queries.double().reshape(-1, rows.shape[1])
    out = torch.empty((q.shape[0], rows.shape[0]), dtype=torch.float64)
    for i, j in _chunks(rows.shape[0], rows.shape[1] + q.shape[0]):
        out[:, i:j] = (_unit_rows64(rows[i:j], gates, pre, post) @ q.t()).t()
    return out.reshape((q.shape[0],) + shape)


def value_bound(C, queries):
    """(2 C + 16) 2^-24 max(1, |q_k|) per query, float64 (Q,): a C-term float32 dot product of a unit row errs by at most about
    C 2^-24 |q| in any summation order, the two norms add about C / 2 2^-24 relative each, the rest is slack for the divide, the
    square root and the (s + 1) / 2."""
    q = queries.double().reshape(-1, C)
    return (2 * C + 16) * 2.0 ** -24 * q.norm(dim=-1).clamp_min(1.0)


def select64(features, queries, threshold, gates=None, pre="none", half_shift=True):
    """(mask bool, score float64, t float64 (Q,) + shape)."""
    s = scores64(features, queries, gates, pre, True)
    t = (s + 1.0) / 2 if half_shift else s
    b = t > threshold
    score = torch.where(b, t, torch.zeros_like(t)).max(dim=0).values
    return b.any(dim=0), score, t


def assign64(features, centers, gates=None, pre="l2"):
    """(labels int64, best float64, gap float64 = best minus the second largest s_k (inf for K = 1), second int64), each of the
    output shape.  torch.argmax on the CPU returns the lowest index among equal maxima."""
    rows, shape = rows_of(features)
    q = centers.double().reshape(-1, rows.shape[1])
    N, K = rows.shape[0], q.shape[0]
    labels = torch.empty(N, dtype=torch.int64)
    second = torch.zeros(N, dtype=torch.int64)
    best = torch.empty(N, dtype=torch.float64)
    gap = torch.full((N,), float("inf"), dtype=torch.float64)
    for i, j in _chunks(N, rows.shape[1] + K):
        s = _unit_rows64(rows[i:j], gates, pre, True) @ q.t()
        labels[i:j] = s.argmax(dim=-1)
        best[i:j] = s.gather(1, labels[i:j, None])[:, 0]
        if K > 1:
            s.scatter_(1, labels[i:j, None], float("-inf"))
            second[i:j] = s.argmax(dim=-1)
            gap[i:j] = best[i:j] - s.gather(1, second[i:j, None])[:, 0]
    return labels.reshape(shape), best.reshape(shape), gap.reshape(shape), second.reshape(shape)


# ---- the reference's float32 lines ----------------------------------------------------------------------------------------------

def literal32_gui_frame(rendered, gates, chosen_feature, score_thres, proj_mat=None):
    """saga_gui.py:590-599, 633, 645-652 (and :593 with proj_mat).  rendered (C, H, W), gates (C,), chosen_feature (C, Q) as :637-641
    build it.  Returns (score_binary.any(-1) as :656 reduces it, score_map after :652, sem_transed or None)."""
    sems = rendered.clone().permute(1, 2, 0)                                                  # :590
    H, W, C = sems.shape                                                                      # :591
    sems /= (torch.norm(sems, dim=-1, keepdim=True) + 1e-6)                                   # :592
    sem_transed = None if proj_mat is None else sems @ proj_mat                               # :593
    scale_gated_feat = sems * gates.unsqueeze(0).unsqueeze(0)                                 # :598
    scale_gated_feat = torch.nn.functional.normalize(scale_gated_feat, dim=-1, p=2)           # :599
    featmap = scale_gated_feat.reshape(H, W, -1)                                              # :633
    score_map = featmap @ chosen_feature                                                      # :645
    score_map = (score_map + 1.0) / 2                                                         # :648
    score_binary = score_map > score_thres                                                    # :649
    score_map[~score_binary] = 0.0                                                            # :651
    score_map = torch.max(score_map, dim=-1).values                                           # :652
    return torch.max(score_binary, dim=-1).values, score_map, sem_transed


def literal32_segment3d(feat_pts, gates, chosen_feature, score_thres):
    """saga_gui.py:674-679.  Returns (score_pts_binary, score_pts after :678)."""
    scale_gated_feat_pts = feat_pts * gates.unsqueeze(0)                                      # :674
    scale_gated_feat_pts = torch.nn.functional.normalize(scale_gated_feat_pts, dim=-1, p=2)   # :675
    score_pts = scale_gated_feat_pts @ chosen_feature                                         # :677
    score_pts = (score_pts + 1.0) / 2                                                         # :678
    return (score_pts > score_thres).sum(1) > 0, score_pts                                    # :679


def literal32_cluster_in_3d(point_features, gates, cluster_centers):
    """saga_gui.py:526-528, 542-543 (the notebook's "Cluster in 3D").  Returns (seg_score (P, K), seg_score.argmax(-1))."""
    scale_conditioned_point_features = torch.nn.functional.normalize(point_features, dim=-1, p=2) * gates.unsqueeze(0)   # :526
    normed_point_features = torch.nn.functional.normalize(scale_conditioned_point_features, dim=-1, p=2)                # :528
    seg_score = torch.einsum('nc,bc->bn', cluster_centers.cpu(), normed_point_features.cpu())                           # :542
    return seg_score, seg_score.argmax(dim=-1)                                                                          # :543


def literal32_get_similarity_map(point_features, gates, query_feature):
    """prompt_segmenting.ipynb, get_similarity_map (and "Segmentation in 3D"): gate, normalise, einsum('C,NC->N')."""
    scale_conditioned_point_features = point_features * gates.unsqueeze(0)
    normed_scale_conditioned_point_features = torch.nn.functional.normalize(scale_conditioned_point_features, dim=-1, p=2)
    return torch.einsum('C,NC->N', query_feature, normed_scale_conditioned_point_features)


def literal32_point_prompt_2d(rendered, gates, query_feature):
    """prompt_segmenting.ipynb "Point Prompt": gate the (C, H, W) render, normalise over C, einsum('C,HWC->HW')."""
    feature_with_scale = rendered * gates.unsqueeze(-1).unsqueeze(-1)
    scale_conditioned_feature = feature_with_scale.permute([1, 2, 0])
    normed_features = torch.nn.functional.normalize(scale_conditioned_feature, dim=-1, p=2)
    return torch.einsum('C,HWC->HW', query_feature, normed_features)


def literal32_cluster_2d(rendered, gates, cluster_centers):
    """prompt_segmenting.ipynb "Cluster in 2D": einsum('nc,hwc->hwn') on the gated, normalised render and its argmax."""
    normed_features = torch.nn.functional.normalize((rendered * gates.unsqueeze(-1).unsqueeze(-1)).permute([1, 2, 0]), dim=-1, p=2)
    segmentation_res = torch.einsum('nc,hwc->hwn', cluster_centers, normed_features)
    return segmentation_res, segmentation_res.argmax(dim=-1)


# ---- the cases the GPU test and the host test share: seeds and shapes -----------------------------------------------------------

def make_case(layout, shape, C, Q, seed, gated=True):
    """i.i.d. normal rows, queries and gates in (0, 1) as a sigmoid scale gate gives them (float32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn((C,) + tuple(shape), generator=g) if layout == "image" else torch.randn(tuple(shape) + (C,), generator=g)
    queries = torch.randn(Q, C, generator=g)
    gates = torch.rand(C, generator=g) * 0.9 + 0.05 if gated else None
    return feats, queries, gates


# (layout, shape, C, Q or K, seed): the decision cases whose excused share is capped at 1 %
CAP_CASES = [
    ("image", (6, 65), 32, 4, 1), ("image", (3, 1920), 32, 1, 2), ("points", (257,), 32, 16, 3), ("points", (4099,), 256, 4, 4),
    ("image", (5, 63), 100, 2, 5), ("points", (5000,), 64, 3, 6), ("points", (3001,), 33, 16, 7), ("image", (7, 64), 31, 5, 8),
]
ASSIGN_CASES = [
    ("points", (4099,), 32, 38, 11), ("points", (2500,), 64, 130, 12), ("image", (9, 65), 32, 17, 13), ("points", (1500,), 256, 512, 14),
    ("image", (16, 64), 100, 33, 15), ("points", (3000,), 3, 40, 16),
]


def unit_centers(centers):
    return torch.nn.functional.normalize(centers, dim=-1)
