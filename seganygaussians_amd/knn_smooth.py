"""Fused KNN feature smoothing: host side of include/mi_knn_smooth.h.

Mirrors FeatureGaussianModel.get_smoothed_point_features (scene/gaussian_model_ff.py:338-364) plus the renderer's
re-normalisation of its result (gaussian_renderer/__init__.py:362-363):

    normed = F.normalize(features, dim=-1, p=2)
    cols   = torch.randperm(K)[:int(K * dropout)]              # all K columns when dropout is outside (0, 1)
    ret    = normed[knn_idx[:, cols], :].mean(dim=1)
    ret    = ret / (ret.norm(dim=1, keepdim=True) + 1e-9)      # renderer, norm_point_features=True

as ONE gather kernel forward and two gather kernels backward (no (P, k, C) tensor, no index_put atomics).
The neighbour map itself is built once and cached by the reference (pytorch3d.ops.knn_points, absent here);
`NeighbourMap` caches the map and its inverse lists (`NeighbourMap.from_points` builds it with the exact HIP KNN of
seganygaussians_amd/knn.py); `knn_points_bruteforce` is the exhaustive checker the tests use.
There is no CPU path: CPU tensors raise.

The multi-resolution variant (get_multi_resolution_smoothed_point_features, gaussian_model_ff.py:366-400: one neighbour map per
sampled subset of the cloud, per-Gaussian level weights that are learned) runs through the same kind of kernels:
`MultiResNeighbourMap` composes the levels' maps into one map of global indices, `multi_res_smooth_point_features` is the
autograd function (gradients for the features and the weights)."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib
from ._ffi import check, dev_ptr, ptr, stream_ptr


FUSED_MAX_K = 32   # neighbours per row the fused kernels handle (include/mi_knn_smooth.h); all levels together for multi-resolution
FUSED_MAX_LEVELS = 4
FUSED_CHANNELS = (32, 64)


class NeighbourMap:
    """knn_idx [P, K] (int32 on the GPU) plus the inverse lists the backward walks, built once per map
    (the reference caches `feature_smooth_map` the same way, gaussian_model_ff.py:345-352)."""

    def __init__(self, knn_idx: torch.Tensor):
        if knn_idx.dim() != 2 or knn_idx.size(1) < 1 or knn_idx.size(1) > FUSED_MAX_K:
            raise ValueError("knn_idx must have shape (P, K) with 1 <= K <= 32")
        if not knn_idx.is_cuda:
            raise RuntimeError("knn_idx must be on the GPU: the fused smoothing has no CPU path")
        P, K = knn_idx.shape
        self.P, self.K = int(P), int(K)
        self.idx = knn_idx.to(torch.int32).contiguous()
        flat = self.idx.reshape(-1).to(torch.int64)
        if P and (int(flat.min()) < 0 or int(flat.max()) >= P):
            raise ValueError("knn_idx holds indices outside [0, P)")
        order = torch.argsort(flat, stable=True)                       # entries grouped by the referenced Gaussian
        counts = torch.bincount(flat, minlength=P)
        off = torch.zeros(P + 1, dtype=torch.int64, device=knn_idx.device)
        off[1:] = torch.cumsum(counts, 0)
        self.inv_offsets = off.to(torch.int32).contiguous()
        self.inv_entries = (((order // K) << 5) | (order % K)).to(torch.int32).contiguous()  # uint32 bit pattern


    @classmethod
    def from_points(cls, xyz: torch.Tensor, K: int = 16) -> "NeighbourMap":
        """The map SAGA builds once per scene: `pytorch3d.ops.knn_points(xyz[None], xyz[None], K=K).idx.squeeze()`
        (gaussian_model_ff.py:345-352), here by the exact HIP search (seganygaussians_amd/knn.py)."""
        from .knn import KnnIndex
        idx, _ = KnnIndex(xyz).query(None, K)
        return cls(idx)


def _mask_of(K: int, cols) -> int:
    m = 0
    for c in (cols.tolist() if torch.is_tensor(cols) else cols):
        c = int(c)
        if not 0 <= c < K:
            raise ValueError(f"neighbour column {c} outside [0, {K})")
        m |= 1 << c
    return m


class _KnnSmooth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, nmap: NeighbourMap, sel_mask: int, normalize_out: bool):
        L = _lib.load()
        if not features.is_cuda:
            raise RuntimeError("features must be on the GPU: the fused smoothing has no CPU path")
        P, C = features.shape
        if P != nmap.P:
            raise ValueError(f"features has {P} rows, the neighbour map {nmap.P}")
        dev = features.device
        f = features.contiguous().float()
        out = torch.empty_like(f)
        with torch.cuda.device(dev):
            rc = L.mi_knn_smooth_forward(P, C, nmap.K, nmap.idx.data_ptr(), sel_mask, dev_ptr(f, "features", dev),
                                         out.data_ptr(), int(bool(normalize_out)), stream_ptr(dev))
        check(rc)
        ctx.save_for_backward(f)
        ctx.nmap, ctx.sel_mask, ctx.normalize_out = nmap, sel_mask, bool(normalize_out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        L = _lib.load()
        (f,) = ctx.saved_tensors
        nmap = ctx.nmap
        P, C = f.shape
        dev = f.device
        g = grad_out.contiguous().float()
        dmean = torch.empty_like(f)
        dF = torch.empty_like(f)
        with torch.cuda.device(dev):
            rc = L.mi_knn_smooth_backward(P, C, nmap.K, nmap.idx.data_ptr(), nmap.inv_offsets.data_ptr(),
                                          nmap.inv_entries.data_ptr(), ctx.sel_mask, f.data_ptr(),
                                          dev_ptr(g, "grad", dev), dmean.data_ptr(), dF.data_ptr(),
                                          int(ctx.normalize_out), stream_ptr(dev))
        check(rc)
        return dF, None, None, None


def smooth_point_features(features: torch.Tensor, nmap: NeighbourMap, cols=None, normalize_out: bool = True):
    """mean over the neighbour columns `cols` (default: all K) of the L2-normalised rows, optionally re-normalised."""
    mask = _mask_of(nmap.K, range(nmap.K) if cols is None else cols)
    return _KnnSmooth.apply(features, nmap, mask, normalize_out)


def get_smoothed_point_features(features: torch.Tensor, nmap: NeighbourMap, K: int = 16, dropout: float = 0.5,
                                normalize_out: bool = False, generator: Optional[torch.Generator] = None):
    """Drop-in for FeatureGaussianModel.get_smoothed_point_features (gaussian_model_ff.py:338-364): same column
    draw (`torch.randperm(K)[:int(K*dropout)]` on the CPU generator), same result.  normalize_out=True also applies
    the renderer's `x / (|x| + 1e-9)` (gaussian_renderer/__init__.py:362-363) inside the same kernel."""
    if K <= 1:
        return features
    assert dropout < 0 or int(K * dropout) >= 1
    if nmap.K != K:
        raise ValueError(f"neighbour map was built for K={nmap.K}, asked for K={K}")
    cols = torch.randperm(K, generator=generator)[: int(K * dropout)] if 0 < dropout < 1 else None
    return smooth_point_features(features, nmap, cols, normalize_out)


def fused_get_smoothed_point_features(self, K=16, dropout=0.5):
    """What `install_dropin(fuse_smoothing=True)` binds to the reference's FeatureGaussianModel.get_smoothed_point_features
    (scene/gaussian_model_ff.py:338-364): same signature and state (`self.feature_smooth_map = {"K", "m"}`, built with
    pytorch3d.ops.knn_points = the HIP KNN drop-in), same `torch.randperm(K)[:int(K*dropout)]` draw from the CPU generator, the
    normalise -> gather -> mean and its backward in the fused kernels instead of PyTorch's (P, k, C) gather and index_put."""
    if K <= 1:
        return self._point_features
    # The fused kernels keep a row's K neighbours in registers (K <= 32) and the HIP search returns K real neighbours (K <= P);
    # the reference expression takes any smooth_K and pytorch3d pads: outside those limits it is the reference's own method
    # that runs.
    if K > FUSED_MAX_K or K > self._point_features.shape[0]:
        ref = getattr(type(self), "_reference_get_smoothed_point_features", None)
        if ref is None:
            raise ValueError(f"fused feature smoothing supports K <= {FUSED_MAX_K} and K <= number of points; got K={K}")
        return ref(self, K, dropout)
    assert dropout < 0 or int(K * dropout) >= 1
    with torch.no_grad():
        if self.feature_smooth_map is None or self.feature_smooth_map["K"] != K:
            import pytorch3d.ops
            xyz = self.get_xyz
            nearest_k_idx = pytorch3d.ops.knn_points(xyz.unsqueeze(0), xyz.unsqueeze(0), K=K).idx.squeeze()
            self.feature_smooth_map = {"K": K, "m": nearest_k_idx}
        m = self.feature_smooth_map["m"]
        cached = getattr(self, "_mi_neighbour_map", None)
        if cached is None or cached[0] is not m:           # inverse lists: once per neighbour map, like the map itself
            cached = (m, NeighbourMap(m))
            self._mi_neighbour_map = cached
    cols = torch.randperm(K)[: int(K * dropout)] if 0 < dropout < 1 else None
    return smooth_point_features(self._point_features, cached[1], cols, normalize_out=False)


# ---- multi-resolution smoothing (gaussian_model_ff.py:366-400) -----------------------------------------------------------------

def draw_point_masks(P: int, sample_rates, generator: Optional[torch.Generator] = None):
    """The reference's subset draw: one `torch.rand(P) < r` per level, in level order, on the CPU generator."""
    return [torch.rand(P, generator=generator) < r for r in sample_rates]


def compose_levels(levels):
    """[(point_mask bool [P], idx [P, k_l] into the compacted subset xyz[point_mask]), ...] -> (one [P, sum k_l] map of global
    indices, the levels side by side; [k_0, k_1, ...]).  Validates shapes, index ranges and the fused kernels' limits."""
    levels = list(levels)
    if not 1 <= len(levels) <= FUSED_MAX_LEVELS:
        raise ValueError(f"need 1 <= levels <= {FUSED_MAX_LEVELS}, got {len(levels)}")
    parts, level_k, P = [], [], None
    for l, (pm, idx) in enumerate(levels):
        if pm.dim() != 1 or pm.dtype != torch.bool:
            raise ValueError(f"level {l}: point_mask must be a bool tensor of shape (P,)")
        if P is None:
            P = pm.numel()
        if pm.numel() != P or idx.dim() != 2 or idx.size(0) != P or idx.size(1) < 1:
            raise ValueError(f"level {l}: need point_mask (P,) and idx (P, k >= 1) with P = {P}")
        if idx.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"level {l}: idx must be int32 or int64")
        sub = torch.nonzero(pm, as_tuple=False).squeeze(1).to(idx.device)
        if P and (sub.numel() == 0 or int(idx.min()) < 0 or int(idx.max()) >= sub.numel()):
            raise ValueError(f"level {l}: idx holds indices outside its subset of {sub.numel()} points")
        parts.append(sub[idx.long()])
        level_k.append(int(idx.size(1)))
    if sum(level_k) > FUSED_MAX_K:
        raise ValueError(f"the levels' neighbour counts must sum to <= {FUSED_MAX_K}, got {sum(level_k)}")
    return torch.cat(parts, dim=1), level_k


class MultiResNeighbourMap:
    """The levels of `multi_res_feature_smooth_map` as ONE NeighbourMap over global indices (composed once per map, like the
    inverse lists): level l owns `level_k[l]` columns of `nmap.idx`."""

    def __init__(self, levels):
        composed, self.level_k = compose_levels(levels)
        self.nmap = NeighbourMap(composed)
        self.P, self.L, self.K = self.nmap.P, len(self.level_k), self.nmap.K
        self.level_k_c = (ctypes.c_int * self.L)(*self.level_k)

    @classmethod
    def from_points(cls, xyz: torch.Tensor, sample_rates=(0.1, 0.5, 1.5), Ks=(4, 4, 16),
                    generator: Optional[torch.Generator] = None) -> "MultiResNeighbourMap":
        """The maps the reference builds once per scene (gaussian_model_ff.py:373-389): per level a `torch.rand(P) < rate` subset
        and every Gaussian's K nearest members of it, here by the exact HIP search."""
        from .knn import KnnIndex
        if len(sample_rates) != len(Ks):
            raise ValueError("sample_rates and Ks must have the same length")
        levels = []
        for pm, k in zip(draw_point_masks(xyz.size(0), sample_rates, generator), Ks):
            if int(pm.sum()) < k:
                raise ValueError(f"a level's subset has {int(pm.sum())} points, fewer than its K = {k}")
            idx, _ = KnnIndex(xyz[pm.to(xyz.device)]).query(xyz, k)
            levels.append((pm, idx))
        return cls(levels)


def _weights_arg(weights, P: int, L: int, dev):
    """(contiguous weights or None, broadcast flag) of a (P, L) or (1, L) weight tensor."""
    if weights is None:
        return None, 0
    if weights.dim() != 2 or weights.size(1) != L or weights.size(0) not in (1, P):
        raise ValueError(f"smooth_weights must have shape ({P}, {L}) or (1, {L}), got {tuple(weights.shape)}")
    w = weights.contiguous()
    dev_ptr(w, "smooth_weights", dev)
    return w, int(w.size(0) == 1 and P != 1)


class _MultiResSmooth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, weights, mrmap: MultiResNeighbourMap, normalize_out: bool):
        if not features.is_cuda:
            raise RuntimeError("features must be on the GPU: the fused smoothing has no CPU path")
        L = _lib.load()
        if features.dim() != 2 or features.size(1) not in FUSED_CHANNELS:
            raise ValueError(f"features must have shape (P, C) with C in {FUSED_CHANNELS}")
        P, C = features.shape
        if P != mrmap.P:
            raise ValueError(f"features has {P} rows, the neighbour map {mrmap.P}")
        dev = features.device
        f = features.contiguous().float()
        w, bcast = _weights_arg(weights, P, mrmap.L, dev)
        out = torch.empty_like(f)
        with torch.cuda.device(dev):
            rc = L.mi_knn_smooth_multi_forward(P, C, mrmap.L, mrmap.level_k_c, mrmap.nmap.idx.data_ptr(), ptr(w), bcast,
                                               dev_ptr(f, "features", dev), out.data_ptr(), int(bool(normalize_out)), stream_ptr(dev))
        check(rc)
        ctx.save_for_backward(f, w)
        ctx.mrmap, ctx.bcast, ctx.normalize_out = mrmap, bcast, bool(normalize_out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        L = _lib.load()
        f, w = ctx.saved_tensors
        mrmap, nmap = ctx.mrmap, ctx.mrmap.nmap
        P, C = f.shape
        dev = f.device
        g = grad_out.contiguous().float()
        dret = torch.empty_like(f)
        dF = torch.empty_like(f)
        dw = torch.empty((P, mrmap.L), dtype=torch.float32, device=dev) if (w is not None and ctx.needs_input_grad[1]) else None
        with torch.cuda.device(dev):
            rc = L.mi_knn_smooth_multi_backward(P, C, mrmap.L, mrmap.level_k_c, nmap.idx.data_ptr(), nmap.inv_offsets.data_ptr(),
                                                nmap.inv_entries.data_ptr(), ptr(w), ctx.bcast, f.data_ptr(), dev_ptr(g, "grad", dev),
                                                dret.data_ptr(), dF.data_ptr(), ptr(dw), int(ctx.normalize_out), stream_ptr(dev))
        check(rc)
        if dw is not None and ctx.bcast:
            dw = dw.sum(dim=0, keepdim=True)       # one shared row of weights: the kernel wrote every Gaussian's share
        return dF, dw, None, None


def multi_res_smooth_point_features(features: torch.Tensor, mrmap: MultiResNeighbourMap, smooth_weights: Optional[torch.Tensor] = None,
                                    normalize_out: bool = False):
    """sum over the levels of `smooth_weights[:, l]` (1 when absent) times the mean of the L2-normalised rows of level l's
    neighbours, optionally re-normalised like the renderer does; differentiable in `features` and `smooth_weights`."""
    return _MultiResSmooth.apply(features, smooth_weights, mrmap, normalize_out)


def fused_get_multi_resolution_smoothed_point_features(self, sample_rates=(0.1, 0.5, 1.5), Ks=(4, 4, 16), smooth_weights=None):
    """What `install_dropin(fuse_smoothing=True)` binds to the reference's
    FeatureGaussianModel.get_multi_resolution_smoothed_point_features (scene/gaussian_model_ff.py:366-400): same signature,
    assertion and state (`self.multi_res_feature_smooth_map`, a list of {"rate", "K", "point_mask", "m"}, rebuilt under the same
    condition with the same `torch.rand(P) < r` draws from the CPU generator and pytorch3d.ops.knn_points = the HIP KNN drop-in);
    the normalise -> gather -> mean -> weighted sum and its backward in the fused kernels."""
    assert len(sample_rates) == len(Ks) and (smooth_weights is None or smooth_weights.shape[1] == len(Ks))
    ref = getattr(type(self), "_reference_get_multi_resolution_smoothed_point_features", None)

    def outside(why):
        # the reference expression takes any number of levels, any K and any width, and pytorch3d pads a subset smaller than K:
        # outside the fused kernels' limits it is the reference's own method that runs
        if ref is None:
            raise ValueError(f"fused multi-resolution smoothing: {why}")
        return ref(self, sample_rates, Ks, smooth_weights)

    if len(Ks) < 1 or len(Ks) > FUSED_MAX_LEVELS or sum(Ks) > FUSED_MAX_K or min(Ks) < 1:
        return outside(f"needs 1 <= levels <= {FUSED_MAX_LEVELS}, every K >= 1 and sum(Ks) <= {FUSED_MAX_K}; got Ks={tuple(Ks)}")
    if self._point_features.shape[1] not in FUSED_CHANNELS:
        return outside(f"needs a feature width in {FUSED_CHANNELS}, got {self._point_features.shape[1]}")
    before = (torch.get_rng_state(), self.multi_res_feature_smooth_map)   # what a call of the reference's method must find
    if len(self.multi_res_feature_smooth_map) != len(sample_rates):
        self.multi_res_feature_smooth_map = []
    maps = list(self.multi_res_feature_smooth_map)
    with torch.no_grad():
        import pytorch3d.ops
        xyz = self.get_xyz
        for i, (r, k) in enumerate(zip(sample_rates, Ks)):
            if len(maps) <= i or maps[i]["rate"] != r or maps[i]["K"] != k:
                pm = torch.rand(xyz.shape[0]) < r
                if int(pm.sum()) < k:
                    torch.set_rng_state(before[0])
                    self.multi_res_feature_smooth_map = before[1]
                    return outside(f"level {i} drew a subset of {int(pm.sum())} points, fewer than its K = {k}")
                nearest_k_idx = pytorch3d.ops.knn_points(xyz.unsqueeze(0), xyz[pm].unsqueeze(0), K=k).idx.squeeze()
                entry = {"rate": r, "K": k, "point_mask": pm, "m": nearest_k_idx}
                if len(maps) <= i:
                    maps.append(entry)
                else:
                    maps[i] = entry
        self.multi_res_feature_smooth_map[:] = maps
        if any(mrf["m"].dim() != 2 for mrf in maps):     # a cloud of one point: .squeeze() dropped the row axis too
            return outside("needs neighbour maps of shape (P, K)")
        cached = getattr(self, "_mi_multi_res_map", None)
        key = [(mrf["m"], mrf["point_mask"]) for mrf in maps]
        if cached is None or len(cached[0]) != len(key) or any(a is not c or b is not d for (a, b), (c, d) in zip(cached[0], key)):
            cached = (key, MultiResNeighbourMap([(pm, m) for m, pm in key]))   # composed map + inverse lists: once per set of maps
            self._mi_multi_res_map = cached
    return multi_res_smooth_point_features(self._point_features, cached[1], smooth_weights, normalize_out=False)


def knn_points_bruteforce(xyz: torch.Tensor, K: int, chunk: int = 4096) -> torch.Tensor:
    """K nearest neighbours (self included, nearest first) by chunked exhaustive search: what
    pytorch3d.ops.knn_points(xyz[None], xyz[None], K=K).idx.squeeze() returns.  O(P^2): the CHECKER of the HIP search
    (seganygaussians_amd/knn.py) in the tests; NeighbourMap.from_points uses the HIP search."""
    P = xyz.size(0)
    out = torch.empty((P, K), dtype=torch.int64, device=xyz.device)
    for s in range(0, P, chunk):
        d = torch.cdist(xyz[s:s + chunk], xyz)
        out[s:s + chunk] = d.topk(K, dim=1, largest=False).indices
    return out
