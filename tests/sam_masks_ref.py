"""Plain numpy / torch restatement of seganygaussians_amd/sam_masks.py, for the tests.  Runs anywhere.

mask_nms_ref is the decision of clip_utils/sam_utils.py:138-187 in float32, one IEEE operation per step (numpy float32 arrays round
each elementwise operation separately), with the fallbacks of :173-181 as they are meant (the first min(3, M) masks of the sorted
order); tests/test_sam_masks_host.py holds it against the reference's own selections (tests/golden/sam_masks/sam_masks.npz)."""
import os

import numpy as np
import torch

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sam_masks", "sam_masks.npz")


def load_cases(path=GOLDEN):
    """The fixture of tests/golden/make_sam_masks_golden.py as a list of (masks bool (M, h, w), scores f32 (M,),
    (iou_thr, score_thr, inner_thr), the reference's selected_idx int64)."""
    z = np.load(path)
    cases, b0, s0, k0 = [], 0, 0, 0
    for (M, h, w), thr, n in zip(z["shapes"], z["thresholds"], z["selected_len"]):
        nbytes = (int(M) * int(h) * int(w) + 7) // 8
        masks = np.unpackbits(z["mask_bits"][b0:b0 + nbytes])[: M * h * w].reshape(M, h, w).astype(bool)
        cases.append((masks, z["scores"][s0:s0 + M], tuple(float(t) for t in thr), z["selected"][k0:k0 + n].astype(np.int64)))
        b0, s0, k0 = b0 + nbytes, s0 + M, k0 + n
    return cases


def overlaps_ref(masks, order=None):
    """masks bool (M, h, w) -> (inter (M, M) int32, areas (M,) int64), read through `order`."""
    m = np.asarray(masks, dtype=bool)
    if order is not None:
        m = m[np.asarray(order)]
    flat = m.reshape(m.shape[0], -1).astype(np.int64)
    inter = flat @ flat.T
    return inter.astype(np.int32), np.diagonal(inter).astype(np.int64).copy()


def boxes_ref(masks):
    """(M, 4) float32 (x_min, y_min, x_max, y_max), inclusive; NaN rows for empty masks."""
    m = np.asarray(masks, dtype=bool)
    out = np.full((m.shape[0], 4), np.nan, np.float32)
    for i, mk in enumerate(m):
        ys, xs = np.nonzero(mk)
        if ys.size:
            out[i] = (xs.min(), ys.min(), xs.max(), ys.max())
    return out


def _nanmax0(values):
    """max(0, values...) as torch.max over a column that also holds zeros: NaN if any value is NaN."""
    v = np.asarray(values, F32)
    if v.size and np.isnan(v).any():
        return F32(np.nan)
    return max(F32(0), v.max()) if v.size else F32(0)


def nms_tests_ref(inter, areas, s, iou_thr=0.7, score_thr=0.1, inner_thr=0.2):
    """The four tests (iou, score, upper inner, lower inner), each (M,) bool, fallbacks applied, from the intersections, areas and
    scores in descending-score order; a mask is kept where all four hold."""
    M = len(s)
    I = np.asarray(inter, np.int64)
    ia = np.asarray(areas, np.int64)
    a = ia.astype(F32)
    s = np.asarray(s, F32)
    iou_max, in_u, in_l = np.zeros(M, F32), np.zeros(M, F32), np.zeros(M, F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        fi = I.astype(F32)
        r_row = fi / a[:, None]     # [i, j] = I_ij / a_i
        r_col = fi / a[None, :]     # [i, j] = I_ij / a_j
        v = F32(1) - r_col * r_row  # symmetric
        iou = fi / (ia[:, None] + ia[None, :] - I).astype(F32)
    for j in range(M):
        iou_max[j] = _nanmax0(iou[:j, j])
        up = [v[i, j] for i in range(j) if r_row[i, j] < F32(0.5) and r_col[i, j] >= F32(0.85)]
        in_u[j] = _nanmax0(up)
        lo = [v[j, k] for k in range(j + 1, M) if r_row[j, k] >= F32(0.85) and r_col[j, k] < F32(0.5)]
        if j >= 1 and r_row[j - 1, j] < F32(0.5) and r_col[j - 1, j] >= F32(0.85):
            lo.append(v[j - 1, j])   # torch.tril(..., diagonal=1) keeps the first superdiagonal
        in_l[j] = _nanmax0(lo)
    t = F32(1.0 - float(inner_thr))
    k_iou = iou_max <= F32(iou_thr)
    k_conf = s > F32(score_thr)
    k_u = in_u <= t
    k_l = in_l <= t
    top = np.arange(M) < 3
    if not k_conf.any():
        k_conf = top
    if not k_u.any():
        k_u = top
    if not k_l.any():
        k_l = top
    return k_iou, k_conf, k_u, k_l


def nms_decision_ref(inter, areas, s, iou_thr=0.7, score_thr=0.1, inner_thr=0.2):
    """keep (M,) bool in descending-score order."""
    k_iou, k_conf, k_u, k_l = nms_tests_ref(inter, areas, s, iou_thr, score_thr, inner_thr)
    return k_iou & k_conf & k_u & k_l


def mask_nms_ref(masks, scores, iou_thr=0.7, score_thr=0.1, inner_thr=0.2):
    """selected_idx (int64 numpy), in descending-score order; ties by a stable sort."""
    scores = torch.as_tensor(np.asarray(scores, F32))
    s, idx = torch.sort(scores, descending=True, stable=True)
    idx = idx.numpy()
    inter, areas = overlaps_ref(masks, idx)
    keep = nms_decision_ref(inter, areas, s.numpy(), iou_thr, score_thr, inner_thr)
    return idx[keep]


def masks_update_ref(*levels, **kwargs):
    out = ()
    for lvl in levels:
        if not lvl:
            out += ([],)
            continue
        seg = np.stack([m["segmentation"] for m in lvl])
        sc = (np.stack([m["stability_score"] for m in lvl]) * np.stack([m["predicted_iou"] for m in lvl])).astype(F32)
        kept = set(mask_nms_ref(seg, sc, **kwargs).tolist())
        out += ([m for i, m in enumerate(lvl) if i in kept],)
    return out


def score_images_ref(scores, masks):
    """float64 (K, h, w) sum / mean / max, the covering count (h, w) int64 and sum_m |scores[m, k]| bit_m (K, h, w) float64."""
    m = np.asarray(masks, dtype=bool)
    s = np.asarray(scores, np.float64)
    if s.ndim == 1:
        s = s[:, None]
    mf = m.astype(np.float64)
    total = np.einsum("mk,mhw->khw", s, mf)
    mag = np.einsum("mk,mhw->khw", np.abs(s), mf)
    count = m.sum(axis=0).astype(np.int64)
    mean = np.where(count > 0, total / np.maximum(count, 1), 0.0)
    mx = (s[:, :, None, None] * mf[:, None]).max(axis=0)
    return {"sum": total, "mean": mean, "max": mx}, count, mag
