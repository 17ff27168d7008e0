"""SAGA's contrastive loss on the MI355X: SAM-mask targets and the pair loss.

Replaces two blocks of train_contrastive_feature.py for a caller who edits the script as INTEGRATION.md section 6 shows:

  * :145-226 (under no_grad, before the render) -- sample_contrastive_targets().  The reference turns the (M, H, W) bool masks
    into floats (a 995 MB tensor at M = 120 and 1080p), sums them densely three times and builds one (S, S) gt_corr per sampled
    scale in a loop of ~4 (si + 1) + 6 small kernels with a host sync each.  Here the masks are bit-packed (pack_sam_masks,
    31 MB at that size, cacheable per camera), one streaming pass gives the exact mask areas and the sampled rays, and each
    ray's targets are ceil(M / 64) 64-bit words per scale: gt_corr[n][h][j] = (g_h[n] & g_j[n]) != 0.
  * :255-299 (the pair loss) -- contrastive_loss().  No (N, S, S) tensor exists: the kernels visit each pair h < j once,
    recompute corr, the gt bits, the selections and the weight, and reduce deterministically.

Same random draws as the reference, in the same order, from the same generators: torch.randperm(M) and torch.rand(H, W) on
the CPU, then one torch.rand(1) at :197 and one per sampled scale (draw_sampled_scales), and torch.rand_like over (S, S) on
the device where :266 draws it (contrastive_loss).  The scalar work of :156-206 stays on the host in f32 (one IEEE op per
element, the same bits as the reference's device tensors) after ONE device-to-host copy of the sorted scales and indices;
the ray count is the second and last host sync of an iteration."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _lib
from ._ffi import check, ptr, stream_ptr
from .packed_masks import MAX_MASKS, PackedSamMasks, pack_sam_masks   # their home; all three stay names of this module

MAX_SCALES = _lib.MI_CONTRASTIVE_LOSS_MAX_SCALES
MAX_CHANNELS = 256
_ROW_STATS = 8       # CL_ROW_STATS (csrc/contrastive_loss.h)
_ACC_HEAD = 5        # class counts (3), max a, ~min a; then the M mask areas


def draw_sampled_scales(sorted_scales: torch.Tensor, sampled_scale_index: torch.Tensor, upper_bound_scale: float,
                        num_sampled_scales: int = 8):
    """train_contrastive_feature.py:160-170 and :197-206 on the host, after the caller's torch.randperm and torch.rand(H, W).

    sorted_scales: the (M,) f32 mask scales sorted descending (CPU); sampled_scale_index: torch.randperm(M)[:num_sampled_scales].
    Draws one torch.rand(1) for :197 and one per sampled scale, as the reference does, from the CPU generator.
    Returns (index (N,) int64 -- -1, the drawn indices (zero-padded), M - 1 --, upper_bound (N,) bool, sampled_scales (N,) f32)
    with N = num_sampled_scales + 2; every value is the reference's f32 result bit for bit."""
    if sorted_scales.dtype != torch.float32 or sorted_scales.dim() != 1 or sorted_scales.numel() < 1:
        raise ValueError("draw_sampled_scales: need a non-empty (M,) float32 tensor of sorted scales")
    mask_scales = sorted_scales.cpu()
    M = mask_scales.shape[0]
    below = mask_scales[mask_scales < upper_bound_scale]
    if below.numel() == 0:
        # the reference's mask_scales[mask_scales < upper_bound_scale].max() (:170) raises on the empty selection
        raise ValueError(f"draw_sampled_scales: no mask scale lies below upper_bound_scale={upper_bound_scale!r}, so the "
                         f"reference's second_big_scale (max of an empty selection) is undefined")
    # :160-168
    tmp = torch.zeros(num_sampled_scales + 2)
    tmp[1:len(sampled_scale_index) + 1] = sampled_scale_index
    tmp[-1] = M - 1
    tmp[0] = -1
    index = tmp.long()
    sampled_scales = mask_scales[index]
    second_big_scale = below.max()
    # :197-206, the same f32 expressions on CPU tensors
    sampled_scales[0] = upper_bound_scale + upper_bound_scale * torch.rand(1)[0]
    upper = torch.zeros(index.shape[0], dtype=torch.bool)
    for idx, si in enumerate(index.tolist()):
        upper_bound = bool(sampled_scales[idx] >= upper_bound_scale)
        upper[idx] = upper_bound
        if si != M - 1 and not upper_bound:
            sampled_scales[idx] -= (sampled_scales[idx] - mask_scales[si + 1]) * torch.rand(1)[0]
        elif upper_bound:
            sampled_scales[idx] -= (sampled_scales[idx] - second_big_scale) * torch.rand(1)[0]
        else:
            sampled_scales[idx] -= sampled_scales[idx] * torch.rand(1)[0]
    return index, upper, sampled_scales


@dataclass
class ContrastiveTargets:
    """What sample_contrastive_targets hands to the front end and to contrastive_loss.  Public: sampled_ray (H, W) bool,
    ray_yx (S, 2) int32 (row-major), sampled_scales (N,) f32 before q_trans (scale_gate.scale_gates takes them as they are), scale_index (N,) and upper_bound (N,) on the host.
    The rest is device state of the loss kernels (include/mi_contrastive.h)."""
    sampled_ray: torch.Tensor
    ray_yx: torch.Tensor
    sampled_scales: torch.Tensor
    scale_index: torch.Tensor
    upper_bound: torch.Tensor
    num_masks: int
    gt: torch.Tensor        # (S, N, ceil(M / 64)) int64 words
    mean_size: torch.Tensor  # (S,) f32
    acc: torch.Tensor       # (5 + M,) int64: class counts, max / ~min mean size bits, mask areas

    @property
    def num_rays(self) -> int:
        return int(self.ray_yx.shape[0])

    @property
    def num_scales(self) -> int:
        return int(self.scale_index.shape[0])

    @property
    def class_counts(self) -> torch.Tensor:
        """(consistent positive, consistent negative, inconsistent) over the full S x S matrix, diagonal included."""
        return self.acc[:3]


def sample_contrastive_targets(masks, mask_scales: torch.Tensor, upper_bound_scale: float, num_sampled_rays: int = 1000,
                               ray_sample_rate: float = 0, num_sampled_scales: int = 8, device=None) -> ContrastiveTargets:
    """train_contrastive_feature.py:145-226 without :228 (q_trans is scale_gate.py's, fused with the gates): the sampled rays, the sampled scales and the
    per-ray, per-scale gt bitsets.  `masks` is a PackedSamMasks or bool (M, H, W) masks (packed here, on the device);
    `mask_scales` (M,) float32 in the masks' order.  Draws the reference's CPU random numbers in its order."""
    if isinstance(masks, PackedSamMasks):
        packed = masks
    elif isinstance(masks, torch.Tensor):
        packed = pack_sam_masks(masks, device=device)
    else:
        raise ValueError(f"sample_contrastive_targets: masks must be a bool (M, H, W) tensor or PackedSamMasks, got {type(masks)}")
    M, H, W = packed.shape
    dev = packed.device
    if not isinstance(mask_scales, torch.Tensor) or mask_scales.dtype != torch.float32 or tuple(mask_scales.shape) != (M,):
        raise ValueError(f"sample_contrastive_targets: mask_scales must be a float32 ({M},) tensor, got "
                         f"{getattr(mask_scales, 'dtype', type(mask_scales))} {tuple(getattr(mask_scales, 'shape', ()))}")
    N = num_sampled_scales + 2
    if not 1 <= N <= MAX_SCALES:
        raise ValueError(f"sample_contrastive_targets: at most {MAX_SCALES - 2} sampled scales")
    L = _lib.load()
    # :152-156: the same device sort, then ONE device-to-host copy of the sorted scales and indices (host sync 1 of 2)
    scales_dev, sort_idx = torch.sort(mask_scales.to(dev), descending=True)
    both = torch.cat([scales_dev.view(torch.int32).to(torch.int64), sort_idx]).cpu()
    sorted_scales = both[:M].to(torch.int32).view(torch.float32)
    sampled_scale_index = torch.randperm(M)[:num_sampled_scales]                          # :160
    rate = ray_sample_rate if ray_sample_rate > 0 else num_sampled_rays / (W * H)         # :172
    ray_rand = torch.rand(H, W)                                                           # :174
    index, upper, sampled_scales = draw_sampled_scales(sorted_scales, sampled_scale_index, upper_bound_scale, num_sampled_scales)

    acc = torch.zeros((_ACC_HEAD + M,), device=dev, dtype=torch.int64)
    sampled_ray = torch.empty((H, W), device=dev, dtype=torch.bool)
    ray_rand_dev = ray_rand.to(dev)
    with torch.cuda.device(dev):
        check(L.mi_contrastive_cover(M, H, W, packed.words.data_ptr(), ray_rand_dev.data_ptr(), float(torch.tensor(rate, dtype=torch.float32)),
                                     sampled_ray.data_ptr(), acc.data_ptr(), stream_ptr(dev)))
    ray_yx = torch.nonzero(sampled_ray).to(torch.int32).contiguous()                      # row-major; host sync 2 of 2
    S, Wd = int(ray_yx.shape[0]), (M + 63) // 64
    scale_args = torch.stack([index.to(torch.int32), upper.to(torch.int32)]).to(dev)
    gt = torch.empty((S, N, Wd), device=dev, dtype=torch.int64)
    mean_size = torch.empty((S,), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        check(L.mi_contrastive_targets(M, H, W, packed.words.data_ptr(), sort_idx.data_ptr(), S, ptr(ray_yx), N,
                                       scale_args[0].data_ptr(), scale_args[1].data_ptr(), ptr(gt), ptr(mean_size), acc.data_ptr(),
                                       stream_ptr(dev)))
    return ContrastiveTargets(sampled_ray, ray_yx, sampled_scales.to(dev), index, upper, M, gt, mean_size, acc)


@dataclass
class ContrastiveStats:
    """No-grad statistics of contrastive_loss, device tensors (no host sync): cosine_pos / cosine_neg (:297-298), n_pos / n_neg
    the selected pairs h < j of sampled_mask_positive / _negative, class_counts (consistent positive, consistent negative,
    inconsistent) over the full S x S matrix."""
    cosine_pos: torch.Tensor
    cosine_neg: torch.Tensor
    n_pos: torch.Tensor
    n_neg: torch.Tensor
    class_counts: torch.Tensor


class _PairLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, tg, rand, out_f32, out_i64):
        L = _lib.load()
        N, S, C = feats.shape
        dev = feats.device
        partials = torch.empty((S, _ROW_STATS), device=dev, dtype=torch.float64)
        with torch.cuda.device(dev):
            check(L.mi_contrastive_loss_forward(S, N, C, tg.num_masks, ptr(feats), ptr(tg.gt), ptr(tg.mean_size), tg.acc.data_ptr(),
                                                ptr(rand), ptr(partials), out_f32.data_ptr(), out_i64.data_ptr(), stream_ptr(dev)))
        ctx.tg = tg
        ctx.save_for_backward(feats, rand, out_i64)
        return out_f32[0].clone()

    @staticmethod
    def backward(ctx, g):
        L = _lib.load()
        feats, rand, out_i64 = ctx.saved_tensors
        tg = ctx.tg
        N, S, C = feats.shape
        dev = feats.device
        d_feats = torch.empty_like(feats)
        g = g.reshape(1).to(dev, torch.float32).contiguous()
        with torch.cuda.device(dev):
            check(L.mi_contrastive_loss_backward(S, N, C, tg.num_masks, ptr(feats), ptr(tg.gt), ptr(tg.mean_size), tg.acc.data_ptr(),
                                                 ptr(rand), out_i64.data_ptr(), g.data_ptr(), ptr(d_feats), stream_ptr(dev)))
        return d_feats, None, None, None, None


def contrastive_loss(feats: torch.Tensor, tg: ContrastiveTargets):
    """The first two terms of train_contrastive_feature.py:293-294 and the statistics of :297-298.

    feats (N, S, C) float32 on the targets' device: the normalised scale-conditioned features of the sampled rays
    (contrastive_front_end).  Draws torch.rand_like over (S, S) on the device, as :266 does.  Returns (loss, stats): loss is a
    differentiable 0-d f32 tensor, NaN where the reference's is (no rays, no selected pair, all pair weights equal)."""
    if not isinstance(tg, ContrastiveTargets):
        raise ValueError("contrastive_loss: tg must come from sample_contrastive_targets")
    dev = tg.gt.device
    N, S = tg.num_scales, tg.num_rays
    if not isinstance(feats, torch.Tensor) or feats.dtype != torch.float32 or feats.dim() != 3:
        raise ValueError(f"contrastive_loss: feats must be a float32 (N, S, C) tensor, got "
                         f"{getattr(feats, 'dtype', type(feats))} {tuple(getattr(feats, 'shape', ()))}")
    if feats.device != dev:
        raise ValueError(f"contrastive_loss: feats are on {feats.device}, the targets on {dev}")
    if tuple(feats.shape[:2]) != (N, S):
        raise ValueError(f"contrastive_loss: feats have shape {tuple(feats.shape)}, the targets need ({N}, {S}, C)")
    C = int(feats.shape[2])
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError(f"contrastive_loss: need 1 <= C <= {MAX_CHANNELS} channels, got {C}")
    if N > MAX_SCALES:
        raise ValueError(f"contrastive_loss: at most {MAX_SCALES} scales, got {N}")
    rand = torch.rand((S, S), device=dev, dtype=torch.float32)      # rand_like(sum_0) (:266)
    out_f32 = torch.empty((3,), device=dev, dtype=torch.float32)
    out_i64 = torch.empty((2,), device=dev, dtype=torch.int64)
    feats = feats.contiguous()
    if feats.data_ptr() % 16:
        # cl_pair_corr reads rows of C % 4 == 0 channels as float4: a view with a storage offset goes through a fresh buffer
        feats = feats.clone()
    loss = _PairLoss.apply(feats, tg, rand, out_f32, out_i64)
    stats = ContrastiveStats(out_f32[1], out_f32[2], out_i64[0], out_i64[1], tg.class_counts)
    return loss, stats
