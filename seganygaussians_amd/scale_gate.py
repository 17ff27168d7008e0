"""Scale conditioning on the MI355X (C entry points: include/mi_scale_gate.h): the two steps every SAGA stage
that takes a 3-D scale goes through -- q_trans, scikit-learn's QuantileTransformer with the uniform output
(train_contrastive_feature.py:42-62, applied at :228, in the notebook's language loop and in get_similarity_map), and scale_gate,
Linear(1, 32) + Sigmoid (:83-86, :241), or the fixed 1 / 0 gates of :243-244.

  * ScaleQuantile      -- the transformer on the device: fit (no device-to-host read) and transform (one launch), both the bits of
                          scikit-learn 1.7.2 / numpy 2.2.6; state_dict / from_state_dict keep the table next to scale_gate.pt.
  * scale_gates        -- transform and gates in ONE launch, differentiable in weight and bias (one launch, float64 sums in a fixed
                          order, no atomics).  No gradient for the scales: the reference computes them under no_grad.
  * fixed_scale_gates  -- the other branch of :240-245, exact.
  * get_quantile_func  -- the reference's signature: returns q_trans, whose result is (n, 1) on the input's device.

output_distribution="normal" is not offered: no caller of the reference uses it.  The kernels need contiguous float32 tensors on
one GPU; there is no CPU path and neither scikit-learn nor a host round trip."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._args import f32
from ._ffi import check, stream_ptr

MAX_QUANTILES = _lib.MI_SCALE_MAX_QUANTILES
MAX_CHANNELS = _lib.MI_SCALE_MAX_CHANNELS
_NONE, _LEARNED, _FIXED = (_lib.MI_SCALE_GATE[n] for n in ("none", "learned", "fixed"))


def _uniform_only(who, distribution):
    if distribution != "uniform":
        raise ValueError(f'{who}: only output_distribution "uniform" is implemented, got {distribution!r} '
                         "(no caller of the reference uses another, and scipy's norm.ppf is not reproduced)")


def _gpu_scales(who, name, scales):
    """A float32 GPU tensor of any shape, flattened; detached, for the scales carry no gradient.  The device is looked at last:
    callers check everything that needs no device (f32 first) before they come here."""
    f32(who, name, scales)
    if not scales.is_cuda:
        raise ValueError(f"{who}: {name} must be on a GPU, got {scales.device} (there is no CPU fallback)")
    return scales.detach().reshape(-1).contiguous()


class ScaleQuantile:
    """QuantileTransformer(output_distribution="uniform") on the device.  quantiles and references are float64 (n_quantiles_,) device
    tensors, scikit-learn's quantiles_[:, 0] and references_."""

    def __init__(self, quantiles: torch.Tensor, references: torch.Tensor):
        who = "ScaleQuantile"
        for name, t in (("quantiles", quantiles), ("references", references)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() != 1:
                raise ValueError(f"{who}: {name} must be a float64 (n_quantiles,) tensor, got {getattr(t, 'dtype', type(t))}")
            if not t.is_cuda:
                raise ValueError(f"{who}: {name} must be on a GPU, got {t.device} (there is no CPU fallback)")
        if quantiles.shape != references.shape or quantiles.device != references.device:
            raise ValueError(f"{who}: quantiles {tuple(quantiles.shape)} on {quantiles.device} and references {tuple(references.shape)} "
                             f"on {references.device} do not belong together")
        if not 1 <= quantiles.shape[0] <= MAX_QUANTILES:
            raise ValueError(f"{who}: {quantiles.shape[0]} quantiles, need 1 to {MAX_QUANTILES}")
        self.quantiles, self.references = quantiles.detach().contiguous(), references.detach().contiguous()
        self.n_quantiles_ = int(quantiles.shape[0])

    @property
    def device(self):
        return self.quantiles.device

    @classmethod
    def fit(cls, scales, n_quantiles: int = 1000, subsample=10_000):
        """QuantileTransformer(n_quantiles=, subsample=).fit(scales.reshape(-1, 1)) for a float32 GPU tensor of any shape.  With
        subsample < scales.numel() the rows are drawn as scikit-learn draws them with random_state=None, from numpy's GLOBAL
        RandomState (seed it with np.random.seed to repeat a fit); subsample=None uses every scale and draws nothing.  NaNs are
        ignored.  No device-to-host read: the draw and np.linspace are made on the host and uploaded."""
        who = "ScaleQuantile.fit"
        f32(who, "scales", scales)
        N, n_quantiles = int(scales.numel()), int(n_quantiles)
        if N < 1:
            raise ValueError(f"{who}: scales is empty")
        if not 1 <= n_quantiles <= MAX_QUANTILES:
            raise ValueError(f"{who}: n_quantiles must be 1 to {MAX_QUANTILES} (MI_SCALE_MAX_QUANTILES), got {n_quantiles}")
        if subsample is not None and int(subsample) < n_quantiles:
            raise ValueError(f"{who}: n_quantiles ({n_quantiles}) is greater than subsample ({subsample})")      # as scikit-learn
        data = _gpu_scales(who, "scales", scales)
        L = _lib.load()
        dev = data.device
        nq = max(1, min(n_quantiles, N))
        references = torch.from_numpy(np.linspace(0, 1, nq)).to(dev)
        if subsample is not None and int(subsample) < N:
            idx = np.arange(N)
            np.random.mtrand._rand.shuffle(idx)      # sklearn.utils.resample(replace=False), random_state=None
            data = data.index_select(0, torch.from_numpy(idx[:int(subsample)]).to(dev))
        ordered = torch.sort(data).values            # ascending, NaN last
        quantiles = torch.empty((nq,), device=dev, dtype=torch.float64)
        with torch.cuda.device(dev):
            check(L.mi_scale_quantile_fit(int(ordered.shape[0]), ordered.data_ptr(), nq, references.data_ptr(), quantiles.data_ptr(), stream_ptr(dev)))
        return cls(quantiles, references)

    def _run(self, who, x, mode=_NONE, channels=1, weight=None, bias=None, dim=0, want_u=True):
        """One launch over the flat float32 scales x: (u or None, gates or None)."""
        if x.device != self.device:
            raise ValueError(f"{who}: scales is on {x.device}, the quantile table on {self.device}")
        n, dev = int(x.shape[0]), x.device
        u = torch.empty((n,), device=dev, dtype=torch.float32) if want_u else None
        gates = None if mode == _NONE else torch.empty((n, channels), device=dev, dtype=torch.float32)
        if n:
            L = _lib.load()
            with torch.cuda.device(dev):
                check(L.mi_scale_gate_forward(n, x.data_ptr(), self.n_quantiles_, self.quantiles.data_ptr(), self.references.data_ptr(), mode,
                                              channels, None if weight is None else weight.data_ptr(), None if bias is None else bias.data_ptr(),
                                              dim, None if u is None else u.data_ptr(), None if gates is None else gates.data_ptr(),
                                              stream_ptr(dev)))
        return u, gates

    def transform(self, scales):
        """scikit-learn's transform for a float32 GPU tensor: the same shape and dtype, values in [0, 1], NaN for NaN.  One launch on
        the current stream, no host read."""
        x = _gpu_scales("ScaleQuantile.transform", "scales", scales)
        return self._run("ScaleQuantile.transform", x)[0].reshape(scales.shape)

    def state_dict(self):
        return {"quantiles": self.quantiles.clone(), "references": self.references.clone()}

    @classmethod
    def from_state_dict(cls, state, device="cuda"):
        """From state_dict(), or from a fitted scikit-learn object: {"quantiles": qt.quantiles_, "references": qt.references_}
        (numpy arrays or tensors; an (nq, 1) column is flattened)."""
        def table(name):
            t = torch.as_tensor(state[name])
            if t.dtype != torch.float64:
                raise ValueError(f"ScaleQuantile.from_state_dict: {name} must be float64, got {t.dtype}")
            return t.reshape(-1).to(device)
        return cls(table("quantiles"), table("references"))


def _gate_parameters(who, weight, bias):
    f32(who, "weight", weight), f32(who, "bias", bias)
    if bias.dim() != 1 or tuple(weight.shape) not in ((bias.shape[0],), (bias.shape[0], 1)):
        raise ValueError(f"{who}: weight must be (C, 1) or (C,) and bias (C,), got {tuple(weight.shape)} and {tuple(bias.shape)}")
    if not 1 <= bias.shape[0] <= MAX_CHANNELS:
        raise ValueError(f"{who}: {bias.shape[0]} channels, need 1 to {MAX_CHANNELS}")
    return int(bias.shape[0])


class _ScaleGates(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, sq, weight, bias):
        w, b = weight.detach().reshape(-1).contiguous(), bias.detach().contiguous()
        u, gates = sq._run("scale_gates", x, _LEARNED, int(b.shape[0]), w, b)
        ctx.save_for_backward(u, w, b)
        ctx.weight_shape = weight.shape
        return gates

    @staticmethod
    def backward(ctx, g):
        u, w, b = ctx.saved_tensors
        n, channels, dev = int(u.shape[0]), int(b.shape[0]), u.device
        if n == 0:
            return None, None, torch.zeros(ctx.weight_shape, device=dev), torch.zeros_like(b)
        L = _lib.load()
        g = g.to(torch.float32).contiguous()
        d_weight, d_bias = torch.empty_like(w), torch.empty_like(b)
        with torch.cuda.device(dev):
            check(L.mi_scale_gate_backward(n, channels, u.data_ptr(), w.data_ptr(), b.data_ptr(), g.data_ptr(), d_weight.data_ptr(),
                                           d_bias.data_ptr(), stream_ptr(dev)))
        return None, None, d_weight.reshape(ctx.weight_shape), d_bias


def scale_gates(scales, sq: ScaleQuantile, weight, bias):
    """scale_gate(q_trans(scales).reshape(-1, 1)) of train_contrastive_feature.py:228 and :241 in one launch: (n, C) float32,
    sigmoid(w_c * u_n + b_c) with u = sq.transform(scales).  scales: float32 GPU tensor of any shape (n values); weight (C, 1) or
    (C,) and bias (C,) float32 on the same GPU -- scale_gate[0].weight and .bias --, 1 <= C <= 256.  Differentiable in weight and
    bias; the scales get no gradient."""
    who = "scale_gates"
    f32(who, "scales", scales)
    _gate_parameters(who, weight, bias)
    if not isinstance(sq, ScaleQuantile):
        raise ValueError(f"{who}: sq must be a ScaleQuantile, got {type(sq)}")
    x = _gpu_scales(who, "scales", scales)
    for name, t in (("weight", weight), ("bias", bias)):
        if t.device != x.device:
            raise ValueError(f"{who}: {name} is on {t.device}, the scales on {x.device}")
    return _ScaleGates.apply(x, sq, weight, bias)


def fixed_scale_gates(scales, sq: ScaleQuantile, scale_aware_dim: int, channels: int = 32):
    """fixed_scale_gate[((1 - q_trans(scales)) * scale_aware_dim).long()] of train_contrastive_feature.py:131 and :243-244 in one
    launch: (n, channels) float32, 1.0 in the first channels - scale_aware_dim + i columns and 0.0 behind, a NaN row for a NaN
    scale.  1 <= scale_aware_dim < channels <= 256."""
    who = "fixed_scale_gates"
    f32(who, "scales", scales)
    channels, dim = int(channels), int(scale_aware_dim)
    if not 1 <= channels <= MAX_CHANNELS:
        raise ValueError(f"{who}: {channels} channels, need 1 to {MAX_CHANNELS}")
    if not 1 <= dim < channels:
        raise ValueError(f"{who}: need 1 <= scale_aware_dim < channels = {channels}, got {dim} (outside it the reference uses the learned gates)")
    if not isinstance(sq, ScaleQuantile):
        raise ValueError(f"{who}: sq must be a ScaleQuantile, got {type(sq)}")
    x = _gpu_scales(who, "scales", scales)
    return sq._run(who, x, _FIXED, channels, dim=dim, want_u=False)[1]


def get_quantile_func(scales: torch.Tensor, distribution="normal"):
    """train_contrastive_feature.py:42-62 with its signature: fits on `scales` (any shape; a CPU tensor is moved to the current
    GPU, as the reference's all_scales lives on the host) and returns q_trans, which maps a float32 GPU tensor of n scales to
    (n, 1) on its device.  Only distribution="uniform", which is what every caller of the reference passes."""
    who = "get_quantile_func"
    _uniform_only(who, distribution)
    f32(who, "scales", scales)
    sq = ScaleQuantile.fit(scales if scales.is_cuda else scales.cuda())

    def quantile_transformer_func(scales):
        return sq.transform(scales.reshape(-1, 1))

    quantile_transformer_func.scale_quantile = sq
    return quantile_transformer_func
