"""CPU restatement of the viewer frame (include/mi_viewer.h) in float64, and the reference's
own float32 lines transcribed one for one (literal32_*).  The float64 form is the yardstick of tests/test_viewer.py; the literal form
shows that the reference itself stays inside the yardstick's band (tests/test_viewer_host.py).

Bounds, with vb(q) = segmentation_ref.value_bound(C, q) = (2 C + 16) 2^-24 max(1, |q|):

  rgb, cluster   exact (a copy, or a product with 0 / 1)
  pca            0.5 vb(proj_j) per channel j: the dot product of a unit row errs by vb, the frame takes half of it
  similarity     4 * 0.5 vb(q) + 2^-22: t = (s + 1) / 2 errs by 0.5 vb, Jet's steepest slope is 0.5 per 1/8, i.e. 4, and the map itself
                 is a handful of float32 operations on values in [0, 8]
  frame          (the sum of the enabled components' bounds) / count + 2^-23 max|value|, where value runs over the partial sums of the
                 pixel's components: k - 1 <= 3 additions and one division, each within 2^-24 of a value no larger than that, divided
                 by k, is at most 4 * 2^-24 / k * max|value| <= 2^-23 max|value| for every k >= 2, and nothing for k = 1.

A pixel with some |t_k - threshold| <= 2 * 0.5 vb(q_k) may take the other decision in float32; it is excused where the decision shows:
in the "similarity" component and under preview.  The share of such pixels is capped at 1 % per case.

Covariance (B = mi_view_moments_block() rows per float32 chain): |u| <= 1 with float32 errors of about (C / 2 + 4) 2^-24, so
|d mean_i| <= (C / 2 + 4) 2^-24 (the product adds sum u in float64) and |d cov_ij| <= (B + 2 C + 32) 2^-24."""
from types import SimpleNamespace

import numpy as np
import torch

from tests import segmentation_ref as ref

MODES = ("rgb", "pca", "cluster", "similarity")
JET = torch.tensor([[0, 0, 0.5], [0, 0, 1], [0, 0.5, 1], [0, 1, 1], [0.5, 1, 0.5], [1, 1, 0], [1, 0.5, 0], [1, 0, 0], [0.5, 0, 0]],
                   dtype=torch.float64)


def jet64(score):
    """saga_gui.py:266-292 in float64: linear interpolation between 9 knots at k / 8, constant outside [0, 1].  (...,) -> (..., 3)."""
    x = score.double().clamp(0.0, 1.0) * 8
    i = x.floor().clamp(max=7).long()
    fr = (x - i).unsqueeze(-1)
    return JET[i] * (1 - fr) + JET[i + 1] * fr


def mode_set(modes):
    modes = (modes,) if isinstance(modes, str) else tuple(modes)
    return [m for m in MODES if m in modes] or ["rgb"]


def frame64(features, rgb, proj=None, queries=None, gates=None, threshold=0.0, cluster_rgb=None, modes=("rgb",), preview=False):
    """The frame in float64 with its per-value bound.  Returns a namespace: frame (H, W, 3), bound (H, W, 3), excused (H, W) bool,
    mask, score, t (None without queries), comps {name: (H, W, 3)}."""
    C, H, W = features.shape
    enabled = mode_set(modes)
    img = rgb.double().permute(1, 2, 0)
    mask = score = t = None
    band = torch.zeros(H, W, dtype=torch.bool)
    if queries is not None:
        queries = queries.reshape(-1, C)
        mask, score, t = ref.select64(features, queries, threshold, gates, pre="eps", half_shift=True)
        vbq = ref.value_bound(C, queries)
        band = ((t - threshold).abs() <= 2 * 0.5 * vbq[:, None, None]).any(0)
    rgb_score = img * mask.unsqueeze(-1) if (preview and queries is not None) else img
    zero = torch.zeros(3, dtype=torch.float64)
    comps, bounds = {}, {}
    for m in enabled:
        if m == "rgb":
            comps[m], bounds[m] = rgb_score, zero
        elif m == "pca":
            p = ref.scores64(features, proj.t().contiguous(), None, pre="eps", post=False).permute(1, 2, 0)
            comps[m], bounds[m] = (p * 0.5 + 0.5).clamp(0.0, 1.0), 0.5 * ref.value_bound(C, proj.t().contiguous())
        elif m == "cluster":
            comps[m], bounds[m] = (rgb_score if cluster_rgb is None else cluster_rgb.double().permute(1, 2, 0)), zero
        elif queries is not None:
            comps[m], bounds[m] = jet64(score), (4 * 0.5 * vbq.max() + 2.0 ** -22) * torch.ones(3, dtype=torch.float64)
        else:
            comps[m], bounds[m] = rgb_score, zero
    total = torch.zeros(H, W, 3, dtype=torch.float64)
    largest = torch.zeros(H, W, 3, dtype=torch.float64)
    for m in enabled:
        total = total + comps[m]
        largest = torch.maximum(largest, total.abs())
    k = len(enabled)
    bound = sum(bounds[m] for m in enabled).reshape(1, 1, 3) / k + (2.0 ** -23 * largest if k > 1 else 0.0)
    shows = queries is not None and ("similarity" in enabled or preview)
    return SimpleNamespace(frame=total / k, bound=bound.expand(H, W, 3), excused=band if shows else torch.zeros_like(band),
                           band=band, mask=mask, score=score, t=t, comps=comps)


def frame_errors(got, want):
    """(worst |got - want| / bound over the pixels not excused, with an exact match where the bound is zero; excused share)."""
    err = (got.double() - want.frame).abs()
    keep = ~want.excused.unsqueeze(-1).expand_as(err)
    ratio = torch.where(want.bound > 0, err / want.bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    worst = ratio[keep].max().item() if keep.any() else 0.0
    return worst, want.excused.double().mean().item()


# ---- the reference's float32 lines ----------------------------------------------------------------------------------------------

def literal32_grayscale_to_colormap(gray):
    """saga_gui.py:266-292."""
    jet_colormap = np.array([[0, 0, 0.5], [0, 0, 1], [0, 0.5, 1], [0, 1, 1], [0.5, 1, 0.5], [1, 1, 0], [1, 0.5, 0], [1, 0, 0], [0.5, 0, 0]])
    positions = np.linspace(0, 1, jet_colormap.shape[0])
    r = np.interp(gray, positions, jet_colormap[:, 0])
    g = np.interp(gray, positions, jet_colormap[:, 1])
    b = np.interp(gray, positions, jet_colormap[:, 2])
    return np.stack((r, g, b), axis=-1)


def literal32_fetch_data(rendered, scene_render, proj_mat, gates, chosen_feature, score_thres, rendered_cluster, modes, preview):
    """saga_gui.py:584-599, 630-659, 701-724.  rendered (C, H, W), scene_render (3, H, W), proj_mat (C, 3), chosen_feature (C, Q) or
    None (no click), rendered_cluster (H, W, 3) or None, modes: the four render_mode_* flags by name.  Returns the render buffer
    reshaped (H, W, 3)."""
    render_mode_rgb, render_mode_pca, render_mode_cluster, render_mode_similarity = (m in modes for m in MODES)
    img = scene_render.permute(1, 2, 0)                                                       # :584
    rgb_score = img.clone()                                                                   # :586
    sems = rendered.clone().permute(1, 2, 0)                                                  # :590
    H, W, C = sems.shape                                                                      # :591
    score_map = None                                                                          # :630
    if chosen_feature is not None:
        score_binary, score_map, sem_transed = ref.literal32_gui_frame(rendered, gates, chosen_feature, score_thres, proj_mat)   # :592-652
        if preview:                                                                           # :655
            rgb_score = img * score_binary.unsqueeze(-1)                                      # :656 (max over the queries, keepdim)
        else:
            rgb_score = img                                                                   # :658
    else:
        sems /= (torch.norm(sems, dim=-1, keepdim=True) + 1e-6)                               # :592
        sem_transed = sems @ proj_mat                                                         # :593
    sem_transed_rgb = torch.clip(sem_transed * 0.5 + 0.5, 0, 1)                               # :594
    render_buffer = None                                                                      # :701
    render_num = 0
    if render_mode_rgb or (not render_mode_pca and not render_mode_cluster and not render_mode_similarity):   # :703
        render_buffer = rgb_score.cpu().numpy().reshape(-1)
        render_num += 1
    if render_mode_pca:                                                                       # :707
        render_buffer = sem_transed_rgb.cpu().numpy().reshape(-1) if render_buffer is None else render_buffer + sem_transed_rgb.cpu().numpy().reshape(-1)
        render_num += 1
    if render_mode_cluster:                                                                   # :710
        if rendered_cluster is None:
            render_buffer = rgb_score.cpu().numpy().reshape(-1) if render_buffer is None else render_buffer + rgb_score.cpu().numpy().reshape(-1)
        else:
            render_buffer = rendered_cluster.cpu().numpy().reshape(-1) if render_buffer is None else render_buffer + rendered_cluster.cpu().numpy().reshape(-1)
        render_num += 1
    if render_mode_similarity:                                                                # :717
        if score_map is not None:
            jet = literal32_grayscale_to_colormap(score_map.squeeze().cpu().numpy()).reshape(-1).astype(np.float32)
            render_buffer = jet if render_buffer is None else render_buffer + jet
        else:
            render_buffer = rgb_score.cpu().numpy().reshape(-1) if render_buffer is None else render_buffer + rgb_score.cpu().numpy().reshape(-1)
        render_num += 1
    render_buffer = render_buffer / render_num                                                # :724
    assert render_buffer.dtype == np.float32
    return torch.from_numpy(np.ascontiguousarray(render_buffer)).reshape(H, W, 3)


def literal32_pca(X, n_components=3):
    """saga_gui.py:547-558 with torch.linalg.eigh in place of the removed torch.eig."""
    n = X.shape[0]
    mean = torch.mean(X, dim=0)
    X = X - mean
    covariance_matrix = (1 / n) * torch.matmul(X.T, X).float()
    eigenvalues, eigenvectors = torch.linalg.eigh(covariance_matrix)
    eigenvalues = eigenvalues.abs()                     # :553 is the norm of (re, im)
    idx = torch.argsort(-eigenvalues)
    eigenvectors = eigenvectors[:, idx]
    return eigenvectors[:, 0:n_components]


def literal32_do_pca(point_features, n=200_000):
    """saga_gui.py:561-568.  The reference seeds the global generator; here its state is put back afterwards."""
    sems = point_features.clone().squeeze()
    N, C = sems.shape
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        randint = torch.randint(0, N, [n])
    sems /= (torch.norm(sems, dim=1, keepdim=True) + 1e-6)
    sem_chosen = sems[randint, :]
    return literal32_pca(sem_chosen, n_components=3), randint


# ---- float64 moments and basis ----------------------------------------------------------------------------------------------------

def moments64(features, index=None, pre="eps"):
    """(mean (C,), cov (C, C), n) in float64: cov = sum u u^T / n - mean mean^T."""
    rows, _ = ref.rows_of(features)
    if index is not None:
        rows = rows[index]
    u = ref._unit_rows64(rows, None, pre, False)
    n = u.shape[0]
    mean = u.sum(0) / n
    return mean, u.t() @ u / n - torch.outer(mean, mean), n


def basis64(cov, n_components=3):
    """Eigenpairs by descending eigenvalue, the largest-magnitude component of each vector (lowest index on ties) positive."""
    w, v = torch.linalg.eigh(cov.double())
    w, v = w.flip(0), v.flip(1)
    k = v.abs().argmax(dim=0)
    sign = torch.where(v.gather(0, k[None])[0] < 0, -1.0, 1.0).double()
    return (v * sign[None])[:, :n_components], w[:n_components], w


def moment_bounds(C, B):
    """(|d mean_i|, |d cov_ij|) allowed."""
    return (C / 2 + 4) * 2.0 ** -24, (B + 2 * C + 32) * 2.0 ** -24


def eigen_gaps(w_all, n_components):
    """gap_j = the distance from eigenvalue j to the nearest other one."""
    d = (w_all[:, None] - w_all[None, :]).abs() + torch.diag(torch.full((w_all.numel(),), float("inf"), dtype=torch.float64))
    return d.min(dim=1).values[:n_components]


def planted_features(P, C, seed, scales=(64.0, 16.0, 4.0, 1.0), offset=4.0, noise=0.02):
    """Rows offset * e_4 + sum_k scales[k] z_k e_k + noise in an orthonormal frame e: after the row normalisation the leading
    eigenvalues stay apart (the host test asserts gaps of at least 20 % of the eigenvalue for the first three)."""
    g = torch.Generator().manual_seed(seed)
    frame, _ = torch.linalg.qr(torch.randn(C, C, generator=g, dtype=torch.float64))
    z = torch.randn(P, len(scales), generator=g, dtype=torch.float64) * torch.tensor(scales, dtype=torch.float64)
    rows = z @ frame[:, :len(scales)].t() + offset * frame[:, len(scales)] + noise * torch.randn(P, C, generator=g, dtype=torch.float64)
    return rows.float()


PLANTED = dict(P=6000, C=32, seed=77)


# ---- the cases the GPU test and the host test share: seeds and shapes -----------------------------------------------------------

def make_view_case(shape, C, Q, seed):
    """features, unit-norm queries (None for Q = 0), gates, rgb, cluster_rgb, proj (C, 3) with unit columns (float32, CPU)."""
    feats, queries, gates = ref.make_case("image", shape, C, max(Q, 1), seed)
    g = torch.Generator().manual_seed(seed + 10_000)
    rgb = torch.rand((3,) + tuple(shape), generator=g)
    cluster = torch.rand((3,) + tuple(shape), generator=g)
    proj = torch.randn(C, 3, generator=g, dtype=torch.float64)
    if C >= 3:
        proj, _ = torch.linalg.qr(proj)
    proj = (proj / proj.norm(dim=0, keepdim=True)).float()
    queries = torch.nn.functional.normalize(queries, dim=-1) if Q else None
    return SimpleNamespace(features=feats, queries=queries, gates=gates, rgb=rgb, cluster_rgb=cluster, proj=proj)


# ((H, W), C, Q, seed, threshold): every N mod 4, the vector seams, more than one workgroup (256 lanes of 4 pixels = 1024 pixels)
FRAME_CASES = [
    ((1, 1), 1, 1, 1, 0.5), ((3, 5), 3, 0, 2, 0.5), ((3, 5), 3, 1, 3, 0.55), ((2, 6), 31, 4, 4, 0.5), ((7, 9), 32, 4, 5, 0.55),
    ((8, 8), 32, 16, 6, 0.7), ((5, 13), 33, 5, 7, 0.5), ((6, 65), 33, 5, 8, 0.55), ((4, 256), 64, 1, 9, 0.7), ((5, 64), 64, 16, 10, 0.5),
    ((2, 130), 256, 3, 11, 0.55), ((4, 256), 32, 0, 12, 0.5), ((8, 8), 256, 1, 13, 0.7), ((5, 413), 32, 4, 14, 0.55),
    ((6, 342), 1, 5, 15, 0.5),
]
MODE_CASE = ((7, 9), 32, 4, 5, 0.55)      # all 16 mode subsets x preview x cluster_rgb
ALL_MODE_SUBSETS = [tuple(m for i, m in enumerate(MODES) if bits >> i & 1) for bits in range(16)]
