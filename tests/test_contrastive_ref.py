"""The float64 reference of the contrastive loss (tests/contrastive_ref.py) checked before the GPU tests use it: against the
literal loops restated in tests/test_contrastive_loss.py (train_contrastive_feature.py:180-183, :207-218, :255-299) and a
per-bit packer.  CPU only."""
import numpy as np
import pytest
import torch

from tests.contrastive_ref import classes_ref, loss_ref64, pack_ref, targets_ref, unpack_words, weight_ref32
from tests.test_contrastive_loss import _reference_gt_vec, _reference_loss

U = 2.0 ** -24


def _masks(M, H, W, seed):
    """Random overlapping masks, densities from sparse to dense, every pixel of the first rows covered by some mask."""
    g = torch.Generator().manual_seed(seed)
    p = 0.02 + 0.5 * torch.rand(M, 1, 1, generator=g)
    masks = torch.rand(M, H, W, generator=g) < p
    masks[torch.randint(0, M, (H * W,), generator=g), torch.arange(H * W) // W, torch.arange(H * W) % W] = True
    return masks


def _edges(M):
    return sorted({si for si in (-1, 0, 62, 63, 64, 65, M - 2, M - 1) if -1 <= si <= M - 1})


@pytest.mark.parametrize("M", [1, 63, 64, 65, 129])
def test_targets_ref_matches_literal_loop(M):
    H, W = 6, 11
    masks = _masks(M, H, W, seed=M)
    g = torch.Generator().manual_seed(100 + M)
    scales = torch.randperm(M, generator=g).float() / M + 0.01
    _, sort_idx = torch.sort(scales, descending=True)
    yx = torch.nonzero(masks.any(0)).to(torch.int32)
    si_list = [si for si in _edges(M) for _ in (0, 1)]
    ub_list = [ub for _ in _edges(M) for ub in (False, True)]
    ref = targets_ref(masks, sort_idx, yx, si_list, ub_list)
    sam_masks_sampled_ray = masks[sort_idx][:, yx[:, 0].long(), yx[:, 1].long()].float()     # :193, floats as :148
    for n, (si, ub) in enumerate(zip(si_list, ub_list)):
        literal = _reference_gt_vec(sam_masks_sampled_ray, si, ub)
        assert torch.equal(ref.gt_bits[:, n, :], literal.T.bool()), (si, ub)
    assert torch.equal(unpack_words(ref.gt, M), ref.gt_bits)
    # :180-183 literally (every partial sum is an integer below 2^24, so any summation order is exact)
    sam = masks[sort_idx].float()
    per_pixel_mask_size = sam * sam.sum(-1).sum(-1)[:, None, None]
    a_lit = (per_pixel_mask_size.sum(dim=0) / (sam.sum(dim=0) + 1e-9))[yx[:, 0].long(), yx[:, 1].long()]
    assert torch.equal(ref.a.view(torch.int32), a_lit.view(torch.int32))
    assert torch.equal(ref.areas, masks.sum((1, 2)))
    assert (ref.cnt >= 1).all()
    assert torch.equal(ref.cnt.float() + 1e-9, ref.cnt.float())
    assert ((ref.a.double() - ref.a64).abs() <= ref.cnt * U * ref.a64).all()


@pytest.mark.parametrize("W", [1, 7, 63, 64, 65, 130])
def test_pack_ref_matches_per_bit_loop(W):
    M, H = 3, 2
    masks = _masks(M, H, W, seed=W)
    words = pack_ref(masks)
    Wq = (W + 63) // 64
    assert words.shape == (M, H, Wq) and words.dtype == torch.int64
    for m in range(M):
        for y in range(H):
            for q in range(Wq):
                v = 0
                for b in range(64):
                    x = 64 * q + b
                    if x < W and masks[m, y, x]:
                        v |= 1 << b
                assert int(words[m, y, q]) & (2 ** 64 - 1) == v


def test_classes_ref_brute_force():
    M, H, W = 70, 5, 9
    masks = _masks(M, H, W, seed=3)
    sort_idx = torch.randperm(M, generator=torch.Generator().manual_seed(4))
    yx = torch.nonzero(masks.any(0)).to(torch.int32)
    si, ub = [-1, 5, 64, 69], [True, False, False, False]
    ref = targets_ref(masks, sort_idx, yx, si, ub)
    gt_corrs, counts = classes_ref(ref.gt, M)
    S, N = yx.shape[0], len(si)
    for n in range(N):
        for h in range(S):
            for j in range(S):
                assert bool(gt_corrs[n, h, j]) == bool((ref.gt_bits[h, n] & ref.gt_bits[j, n]).any())
    sum_0 = gt_corrs.sum(0)
    assert int(counts.sum()) == S * S
    assert int(counts[0]) == int((sum_0 == N).sum()) and int(counts[1]) == int((sum_0 == 0).sum())


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_loss_ref64_matches_reference_on_dyadic_inputs(seed):
    """Dyadic features and weights: corr, every product and every f32 partial sum of _reference_loss are exact, so the
    selections, counts, the two means (one rounding each) and the loss (their f32 sum) must agree bit for bit."""
    g = torch.Generator().manual_seed(seed)
    N, S, C, M = 4, 40, 3, 9
    feats = torch.randint(-4, 5, (N, S, C), generator=g).float() / 4
    masks = torch.rand(M, 1, S, generator=g) < 0.3
    masks[torch.randint(0, M, (S,), generator=g), 0, torch.arange(S)] = True
    yx = torch.nonzero(masks.any(0)).to(torch.int32)
    ref_t = targets_ref(masks, torch.randperm(M, generator=g), yx, [-1, 2, 5, M - 1], [True, False, False, False])
    gt_corrs, counts = classes_ref(ref_t.gt, M)
    weight = (torch.randint(4, 41, (S, S), generator=g).float() / 4).triu()
    weight = weight + weight.T.triu(1)
    torch.manual_seed(seed)
    loss, cos_pos, cos_neg, counts_r, n_pos, n_neg = _reference_loss(feats, gt_corrs.float(), weight)
    torch.manual_seed(seed)
    rand = torch.rand(S, S)                                                               # the rand_like of :266
    r = loss_ref64(feats, gt_corrs, weight, rand)
    assert torch.equal(r.counts, counts_r) and torch.equal(counts, counts_r)
    assert (r.n_pos, r.n_neg) == (int(n_pos), int(n_neg))
    assert r.n_pos > 0 and r.n_neg > 0
    assert float(r.mean_pos.float() + r.mean_neg.float()) == float(loss)
    assert float(r.cosine_pos.float()) == float(cos_pos) and float(r.cosine_neg.float()) == float(cos_neg)
    # the reference's f32 gradient: within the summation bound of the float64 one
    feats_r = feats.clone().requires_grad_(True)
    (g32,) = torch.autograd.grad(_reference_loss(feats_r, gt_corrs.float(), weight)[0], feats_r)
    assert ((g32.double() - r.grad).abs() <= (S + 8) * U * r.A_g).all()
    assert float(r.A_g.max()) > 0


def test_weight_ref32_is_the_reference_expression():
    a = torch.tensor([3.0, 7.5, 1.25, 7.5], dtype=torch.float32)
    w = weight_ref32(a)
    assert float(w.min()) == 1.0 and float(w.max()) == 10.0
    assert torch.equal(w, w.T)
    # all sizes equal: (w - min) / (max - min) = 0 / 0
    assert torch.isnan(weight_ref32(torch.full((3,), 2.0))).all()
    assert np.isfinite(w.numpy()).all()
