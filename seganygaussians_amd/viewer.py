"""The viewer frame on the MI355X: the PCA basis of the features and the GUI's display buffer.

What a user of saga_gui.py looks at, as device operations:

  * feature_covariance() -- mean and covariance (the reference's 1/n form, saga_gui.py:549-551) of the normalised rows of a feature
                            table (P, C) or feature image (C, H, W), optionally of the rows an index picks; float64, on the device.
  * feature_pca_basis()  -- GaussianSplattingGUI.pca (:547-558) on top of it: the eigenvectors of the largest eigenvalues, by
                            torch.linalg.eigh on the (C, C) float64 matrix on the host (torch.eig no longer exists).  The sign of an
                            eigenvector is fixed: its largest-magnitude component, the lowest index on ties, is positive.
  * gui_pca_sample()     -- the row draw of do_pca (:564-565) from a private generator.
  * viewer_frame()       -- the per-frame body of fetch_data (:590-599, 645-659, 701-724) in one kernel that reads the feature image
                            once: selection mask and score (bit for bit those of select_by_similarity(..., pre="eps",
                            half_shift=True)), the PCA image, the Jet colour map and the average of the enabled views, stored
                            interleaved (H, W, 3) as dpg.set_value("_texture", ...) takes it.
  * prompt_features()    -- the gated, normalised features at clicked pixels (:637), a few torch ops on Q x C values.

float32 tensors on one GPU.  No autograd: inputs that require grad are refused while grad mode is on.  Non-finite inputs are outside
the contract.  There is no CPU fallback."""
from __future__ import annotations

from collections import namedtuple

import torch

from ._args import f32, no_grad_one_gpu, number
from ._ffi import check, ptr, stream_ptr
from ._lib import MI_VIEW_MODES as VIEW_MODES   # mode name -> MI_VIEW_* bit, in the order the components are added
from .segmentation import MAX_QUERIES, PRE_MODES, check_pre, feature_table, gate_row, query_rows

ViewerFrame = namedtuple("ViewerFrame", ["frame", "mask", "score"])


def _index_range(who, index, N):
    lo, hi = int(index.min()), int(index.max())   # the one host read when the index lives on the device
    if lo < 0 or hi >= N:
        raise ValueError(f"{who}: index out of range: values in [{lo}, {hi}], rows in [0, {N})")


def gui_pca_sample(P: int, n: int = 200_000, seed: int = 0) -> torch.Tensor:
    """The rows do_pca samples (saga_gui.py:564-565): the draws of torch.manual_seed(seed); torch.randint(0, P, [n]), taken from a
    private generator so that the global one stays where it is.  int64 (n,), on the host, repeats included."""
    P, n = int(P), int(n)
    if P < 1 or n < 1:
        raise ValueError(f"gui_pca_sample: need P >= 1 and n >= 1, got {P} and {n}")
    g = torch.Generator()
    g.manual_seed(int(seed))
    return torch.randint(0, P, [n], generator=g)


def feature_covariance(features: torch.Tensor, index: torch.Tensor = None, pre: str = "eps"):
    """(mean (C,) float64, cov (C, C) float64, n) of the rows u = pre(f): mean = sum u / n, cov = sum u u^T / n - mean mean^T.

    features: float32 (P, C) or (C, H, W), 1 <= C <= 256.  index: int64 row numbers (pixels in row-major order for an image), repeats
    allowed, checked against the row count before any launch; None takes every row.  pre as in segmentation.py; the GUI uses "eps".
    Two launches, no atomics, bit-identical from run to run; the workspace is a torch allocation of this call."""
    from . import _lib
    who = "feature_covariance"
    layout, C, N, _ = feature_table(who, features)
    check_pre(who, pre)
    n = N
    if index is not None:
        if not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.dim() != 1:
            raise ValueError(f"{who}: index must be a 1-D int64 tensor or None, got {getattr(index, 'dtype', type(index))}")
        n = int(index.numel())
        if not 1 <= n < 1 << 31:
            raise ValueError(f"{who}: need 1 <= len(index) < 2^31, got {n}")
        if not index.is_cuda:
            _index_range(who, index, N)
    dev = no_grad_one_gpu(who, [("features", features)])
    if index is not None:
        if index.is_cuda:
            if index.device != dev:
                raise ValueError(f"{who}: index is on {index.device}, the features on {dev}")
            _index_range(who, index, N)
        index = index.to(dev).contiguous()
    features = features.detach().contiguous()
    L = _lib.load()
    nbytes = int(L.mi_view_moments_workspace_bytes(n, C))
    workspace = torch.empty(nbytes // 8, device=dev, dtype=torch.float64)
    mean = torch.empty(C, device=dev, dtype=torch.float64)
    cov = torch.empty((C, C), device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        check(L.mi_view_moments(layout, N, C, features.data_ptr(), ptr(index), n, PRE_MODES[pre], workspace.data_ptr(), nbytes,
                                mean.data_ptr(), cov.data_ptr(), stream_ptr(dev)))
    return mean, cov, n


def basis_from_covariance(cov: torch.Tensor, n_components: int = 3):
    """(proj (C, n_components) float64, eigenvalues (n_components,) float64) of a symmetric (C, C) matrix, on the host: eigenpairs by
    descending eigenvalue (saga_gui.py:553-556 sorts by |lambda|, the same for a covariance), each eigenvector with its
    largest-magnitude component, the lowest index on ties, made positive."""
    w, v = torch.linalg.eigh(cov.detach().double().cpu())
    w, v = w.flip(0)[:n_components], v.flip(1)[:, :n_components]
    k = v.abs().argmax(dim=0)
    sign = torch.where(v.gather(0, k[None])[0] < 0, -1.0, 1.0).double()
    return v * sign[None], w


def feature_pca_basis(features: torch.Tensor, n_components: int = 3, index: torch.Tensor = None, pre: str = "eps"):
    """GaussianSplattingGUI.pca (saga_gui.py:547-558) of the rows feature_covariance() takes: (proj (C, n_components) float32 on the
    features' device, eigenvalues (n_components,) float64 on the host), by descending eigenvalue.  do_pca is
    feature_pca_basis(point_features, 3, gui_pca_sample(P))."""
    who = "feature_pca_basis"
    f32(who, "features", features)
    if features.dim() in (2, 3):
        C = int(features.shape[0] if features.dim() == 3 else features.shape[1])
        if not 1 <= int(n_components) <= C:
            raise ValueError(f"{who}: need 1 <= n_components <= C = {C}, got {n_components}")
    _, cov, _ = feature_covariance(features, index, pre)
    proj, w = basis_from_covariance(cov, int(n_components))
    return proj.float().to(features.device), w


def prompt_features(features: torch.Tensor, yx, gates: torch.Tensor = None) -> torch.Tensor:
    """The gated, normalised feature rows at clicked pixels (saga_gui.py:637, with :592 and :598-599): (Q, C), whose transpose is the
    reference's chosen_feature.  features (C, H, W); yx: Q pairs (y, x), wrapped modulo H and W as the reference wraps them."""
    who = "prompt_features"
    f32(who, "features", features)
    if features.dim() != 3:
        raise ValueError(f"{who}: features must be (C, H, W), got {tuple(features.shape)}")
    C, H, W = (int(v) for v in features.shape)
    f32(who, "gates", gates, optional=True)
    if gates is not None and gates.numel() != C:
        raise ValueError(f"{who}: gates must hold {C} values, got {tuple(gates.shape)}")
    yx = torch.as_tensor(yx, dtype=torch.int64).reshape(-1, 2)
    if yx.shape[0] < 1:
        raise ValueError(f"{who}: need at least one pixel")
    y, x = (yx[:, 0] % H).to(features.device), (yx[:, 1] % W).to(features.device)
    rows = features.detach()[:, y, x].t()
    rows = rows / (rows.norm(dim=-1, keepdim=True) + 1e-6)
    if gates is not None:
        rows = rows * gates.detach().reshape(1, C)
    return torch.nn.functional.normalize(rows, dim=-1, p=2)


def viewer_frame(features: torch.Tensor, rgb: torch.Tensor, *, proj: torch.Tensor = None, queries: torch.Tensor = None,
                 gates: torch.Tensor = None, threshold: float = 0.0, cluster_rgb: torch.Tensor = None, modes=("rgb",),
                 preview: bool = False, out: torch.Tensor = None) -> ViewerFrame:
    """The display buffer of one GUI frame (saga_gui.py:590-599, 645-659, 701-724) in one launch that reads `features` once.

    features (C, H, W), rgb (3, H, W), cluster_rgb (3, H, W) or None (the reference's rendered_cluster), proj (C, 3) (needed by
    "pca"), queries (Q, C) or (C,), 1 <= Q <= 16, used as given, or None (no click yet), gates (C,) or None.  modes: any of "rgb",
    "pca", "cluster", "similarity"; none behaves as ("rgb",) (:703).  Per pixel, with u = f / (|f| + 1e-6), w = normalize(u * gates):
    t_k = (<w, q_k> + 1) / 2, selected = any t_k > threshold, score = max_k (t_k > threshold ? t_k : 0), rgb_score = rgb * selected
    with preview and queries, else rgb.  The frame is the float32 average, in this order, of: rgb_score ("rgb"),
    clip(u @ proj * 0.5 + 0.5, 0, 1) ("pca"), cluster_rgb or else rgb_score ("cluster"), jet(score) or without queries rgb_score
    ("similarity").  Returns ViewerFrame(frame (H, W, 3) float32, mask (H, W) bool, score (H, W) float32); mask and score are None
    without queries.  out: an (H, W, 3) float32 contiguous tensor to write the frame into."""
    from . import _lib
    who = "viewer_frame"
    f32(who, "features", features)
    if features.dim() != 3:
        raise ValueError(f"{who}: features must be (C, H, W), got {tuple(features.shape)}")
    _, C, N, (H, W) = feature_table(who, features)
    f32(who, "rgb", rgb)
    if tuple(rgb.shape) != (3, H, W):
        raise ValueError(f"{who}: rgb must be (3, {H}, {W}), got {tuple(rgb.shape)}")
    f32(who, "cluster_rgb", cluster_rgb, optional=True)
    if cluster_rgb is not None and tuple(cluster_rgb.shape) != (3, H, W):
        raise ValueError(f"{who}: cluster_rgb must be (3, {H}, {W}), got {tuple(cluster_rgb.shape)}")
    if isinstance(modes, str):
        modes = (modes,)
    bits = 0
    for m in modes:
        if m not in VIEW_MODES:
            raise ValueError(f"{who}: unknown mode {m!r}; modes are {sorted(VIEW_MODES)}")
        bits |= VIEW_MODES[m]
    bits = bits or VIEW_MODES["rgb"]
    f32(who, "proj", proj, optional=True)
    if proj is not None and tuple(proj.shape) != (C, 3):
        raise ValueError(f"{who}: proj must be ({C}, 3), got {tuple(proj.shape)}")
    if proj is None and bits & VIEW_MODES["pca"]:
        raise ValueError(f"{who}: the \"pca\" mode needs proj ({C}, 3)")
    Q = 0
    if queries is not None:
        queries, Q = query_rows(who, queries, C, MAX_QUERIES)
    gates = gate_row(who, gates, C)
    threshold = number(who, "threshold", threshold)
    if out is not None:
        f32(who, "out", out)
        if tuple(out.shape) != (H, W, 3) or not out.is_contiguous():
            raise ValueError(f"{who}: out must be a contiguous ({H}, {W}, 3) tensor, got {tuple(out.shape)}")
    tensors = [("features", features), ("rgb", rgb)] + [(k, t) for k, t in (("cluster_rgb", cluster_rgb), ("proj", proj),
               ("queries", queries), ("gates", gates), ("out", out)) if t is not None]
    dev = no_grad_one_gpu(who, tensors, "features")
    features, rgb = features.detach().contiguous(), rgb.detach().contiguous()
    cluster_rgb, proj, queries, gates = (None if t is None else t.detach().contiguous() for t in (cluster_rgb, proj, queries, gates))
    if not bits & VIEW_MODES["pca"]:
        proj = None
    if Q == 0:
        gates = None   # the gates only shape w
    L = _lib.load()
    frame = out if out is not None else torch.empty((H, W, 3), device=dev, dtype=torch.float32)
    mask = torch.empty((H, W), device=dev, dtype=torch.bool) if Q else None
    score = torch.empty((H, W), device=dev, dtype=torch.float32) if Q else None
    with torch.cuda.device(dev):
        check(L.mi_view_frame(N, C, features.data_ptr(), rgb.data_ptr(), ptr(cluster_rgb), ptr(proj), Q, ptr(queries), ptr(gates),
                              threshold, bits, 1 if preview else 0, frame.data_ptr(), ptr(mask), ptr(score), stream_ptr(dev)))
    return ViewerFrame(frame, mask, score)
