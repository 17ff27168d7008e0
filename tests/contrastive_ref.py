"""Plain high-precision restatement of SAGA's contrastive loss, for checking csrc/contrastive_loss.h.

Used by tests/test_contrastive_loss_edges.py (GPU) and checked itself by tests/test_contrastive_ref.py (CPU).  It shares no code
with seganygaussians_amd/contrastive_loss.py.  Every boolean decision is taken exactly as the reference writes it
(train_contrastive_feature.py:145-226 for the targets, :255-299 for the pair loss); every sum, mean and product of the loss and
its gradient is evaluated in float64, so with dyadic features (corr exact in any precision) the only difference left between
the kernels and this module is the kernels' f32 rounding, which the tests bound.

* pack_ref     -- the bit-packed masks of include/mi_contrastive.h: np.packbits(..., bitorder="little"), 8 bytes per word.
* targets_ref  -- the gt bitsets of :207-218 (vectorised), the mean mask size a of :180-183 two ways: the documented f32
                  contract (covering masks' areas added one at a time in sorted order, over f32(cnt) + 1e-9f) and float64.
* classes_ref  -- the pair classes of :260-263 over the full S x S matrix, diagonal included, by brute force.
* weight_ref32 -- per_pixel_weight of :185-190 in f32, the reference's operations in its order.
* loss_ref64   -- :255-299: selections, loss, cosine statistics, selected pair counts and the gradient by float64 autograd,
                  with the magnitudes A_L and A_g the tests' error bounds are built from.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch


def _pack_last(bits: np.ndarray, words: int) -> torch.Tensor:
    """bool (..., K) -> int64 (..., words): bit b of word q = element 64 q + b, padding bits 0."""
    packed = np.packbits(bits.astype(bool), axis=-1, bitorder="little")
    out = np.zeros(bits.shape[:-1] + (words * 8,), np.uint8)
    out[..., :packed.shape[-1]] = packed
    return torch.from_numpy(np.ascontiguousarray(out).view("<u8").view(np.int64))


def unpack_words(words: torch.Tensor, K: int) -> torch.Tensor:
    """int64 (..., Wd) words -> bool (..., K), the inverse of _pack_last."""
    shifts = torch.arange(64, device=words.device)
    bits = ((words.unsqueeze(-1) >> shifts) & 1).bool()
    return bits.flatten(-2)[..., :K]


def pack_ref(masks: torch.Tensor) -> torch.Tensor:
    """bool (M, H, W) -> int64 (M, H, ceil(W / 64)) on the CPU."""
    W = masks.shape[-1]
    return _pack_last(masks.cpu().numpy(), (W + 63) // 64)


def targets_ref(masks: torch.Tensor, sort_idx: torch.Tensor, ray_yx: torch.Tensor, scale_si, scale_ub):
    """The targets of :180-183 and :207-218 for the rays ray_yx (S, 2) (y, x), on the masks' device.

    masks bool (M, H, W); sort_idx (M,) the descending scale order; scale_si (N,) sorted-mask indices (-1 .. M-1) and
    scale_ub (N,) upper-bound flags.  Returns gt (S, N, ceil(M / 64)) int64 words, gt_bits (S, N, M) bool, a (S,) f32 by
    the contract, a64 (S,) float64, cnt (S,) covering masks per ray and areas (M,) int64 in the masks' own order."""
    dev = masks.device
    M = masks.shape[0]
    sort_idx = sort_idx.to(dev).long()
    ys, xs = ray_yx[:, 0].to(dev).long(), ray_yx[:, 1].to(dev).long()
    cov = masks[sort_idx][:, ys, xs].T.contiguous()                                     # (S, M) sorted-mask cover
    areas = masks.sum((1, 2), dtype=torch.int64)
    sorted_areas = areas[sort_idx]
    cnt = cov.sum(1)
    # :180-183 per the contract: f32, one covering mask at a time in sorted order (adding 0 for the others is exact)
    acc = torch.zeros(cov.shape[0], dtype=torch.float32, device=dev)
    for k in range(M):
        acc = acc + torch.where(cov[:, k], sorted_areas[k].to(torch.float32), torch.zeros((), dtype=torch.float32, device=dev))
    a = acc / (cnt.to(torch.float32) + 1e-9)
    # float64; f32(cnt) + 1e-9f == f32(cnt) for every cnt >= 1, so the f32 contract evaluates sum / cnt
    a64 = (cov.double() * sorted_areas.double()).sum(1) / cnt.double()
    # :207-218: the covering masks of sorted index > si, plus the highest-index covering mask <= si (or all when ub / si < 0)
    order = torch.arange(M, device=dev)
    gts = []
    for si, ub in zip([int(v) for v in scale_si], [bool(v) for v in scale_ub]):
        if ub or si < 0:
            gts.append(cov)
            continue
        above = order > si
        highest = torch.where(cov & ~above, order, torch.full_like(order, -1)).max(1).values
        g = cov & above
        has = highest >= 0
        g[has.nonzero()[:, 0], highest[has]] = True
        gts.append(g)
    gt_bits = torch.stack(gts, 1)                                                        # (S, N, M)
    gt = _pack_last(gt_bits.cpu().numpy(), (M + 63) // 64).to(dev)
    return SimpleNamespace(gt=gt, gt_bits=gt_bits, a=a, a64=a64, cnt=cnt, areas=areas)


def classes_ref(gt: torch.Tensor, M: int):
    """gt (S, N, Wd) words -> gt_corrs (N, S, S) bool (:220-226: (g_h & g_j) != 0) and the class counts (consistent positive,
    consistent negative, inconsistent) of :260-263 over the full matrix, diagonal included."""
    bits = unpack_words(gt, M).double()                                                  # (S, N, M)
    N = bits.shape[1]
    gt_corrs = torch.stack([(bits[:, n] @ bits[:, n].T) > 0 for n in range(N)])          # exact: counts <= M in float64
    sum_0 = gt_corrs.sum(0)
    counts = torch.stack([(sum_0 == N).sum(), (sum_0 == 0).sum(), ((sum_0 != N) & (sum_0 != 0)).sum()])
    return gt_corrs, counts


def weight_ref32(a: torch.Tensor) -> torch.Tensor:
    """per_pixel_weight (S, S) of :185-190 from the mean mask sizes a (S,) f32, the reference's f32 operations in order."""
    pixel_to_pixel_mask_size = a.unsqueeze(0) * a.unsqueeze(1)
    ptp_max_size = pixel_to_pixel_mask_size.max()
    pixel_to_pixel_mask_size[pixel_to_pixel_mask_size == 0] = 1e10
    w = torch.clamp(ptp_max_size / pixel_to_pixel_mask_size, 1.0, None)
    return (w - w.min()) / (w.max() - w.min()) * 9. + 1.


def loss_ref64(feats: torch.Tensor, gt_corrs: torch.Tensor, weight: torch.Tensor, rand: torch.Tensor):
    """:255-299 in float64 from feats (N, S, C), gt_corrs (N, S, S) bool, the f32 per_pixel_weight (S, S) and the f32 draw
    rand (S, S) of :266.

    Decisions as the reference writes them: t_pos / t_neg are its f32 expressions of the integer counts, the compares are
    against the f32 rand, the hints compare corr (exact for dyadic features) with 0.75 and 0.5.  Returns loss, its two means,
    cosine_pos / cosine_neg, n_pos / n_neg, the selections, grad = d loss / d feats (float64 autograd, g = 1), and the
    magnitudes of the error bounds: A_L = mean |positive terms| + mean |negative terms|, A_g[n, h, c] = sum_j |dcorr_hj| |f_jc|
    with dcorr symmetrised."""
    N, S, _ = feats.shape
    f64 = feats.detach().double().requires_grad_(True)
    corr = torch.einsum('nhc,njc->nhj', f64, f64)                                       # :256
    c = corr.detach()
    gt = gt_corrs.bool()
    diag_mask = torch.eye(S, dtype=torch.bool, device=feats.device)
    sum_0 = gt.sum(0)                                                                    # :260
    consistent_negative = sum_0 == 0
    consistent_positive = sum_0 == N
    inconsistent = ~(consistent_negative | consistent_positive)
    sampled_num = inconsistent.count_nonzero() / 2                                       # f32, as :263
    sampled_positive = consistent_positive & (rand < sampled_num / consistent_positive.count_nonzero())
    sampled_negative = consistent_negative & (rand < sampled_num / consistent_negative.count_nonzero())
    pos = (sampled_positive | (gt & (c < 0.75)).any(0) | inconsistent) & ~diag_mask
    pos = torch.triu(pos, diagonal=0)
    neg = (sampled_negative | (~gt & (c > 0.5)).any(0) | inconsistent) & ~diag_mask
    neg = torch.triu(neg, diagonal=0)
    w = weight.double().unsqueeze(0)
    g64 = gt.double()
    t_pos = -w[:, pos] * g64[:, pos] * corr[:, pos]                                      # :293
    t_neg = w[:, neg] * (1 - g64[:, neg]) * torch.relu(corr[:, neg])                    # :294
    mean_pos, mean_neg = t_pos.mean(), t_neg.mean()
    loss = mean_pos + mean_neg
    grad, dcorr = torch.autograd.grad(loss, [f64, corr])
    dsym = dcorr + dcorr.transpose(1, 2)
    A_g = torch.bmm(dsym.abs(), f64.detach().abs())
    with torch.no_grad():
        A_L = t_pos.abs().mean() + t_neg.abs().mean()
        cosine_pos = c[gt].mean()                                                        # :297-298
        cosine_neg = c[~gt].mean()
    counts = torch.stack([consistent_positive.count_nonzero(), consistent_negative.count_nonzero(), inconsistent.count_nonzero()])
    return SimpleNamespace(loss=loss.detach(), mean_pos=mean_pos.detach(), mean_neg=mean_neg.detach(), A_L=A_L, grad=grad,
                           A_g=A_g, cosine_pos=cosine_pos, cosine_neg=cosine_neg, n_pos=int(pos.sum()), n_neg=int(neg.sum()),
                           pos=pos, neg=neg, counts=counts)
