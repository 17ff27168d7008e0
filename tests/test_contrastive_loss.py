"""The contrastive loss on the MI355X (seganygaussians_amd/contrastive_loss.py, csrc/contrastive_loss.h) against the reference
block restated below from train_contrastive_feature.py:145-226 (targets) and :255-299 (pair loss), same seeds, same device."""
import time

import pytest
import torch

from seganygaussians_amd.contrastive_frontend import contrastive_front_end
from seganygaussians_amd.contrastive_loss import contrastive_loss, pack_sam_masks, sample_contrastive_targets

DEV = "cuda:0"


# ---- the reference, restated ---------------------------------------------------------------------------------------------------

def _reference_targets(original_masks, mask_scales, upper_bound_scale, num_sampled_rays=1000, ray_sample_rate=0,
                       num_sampled_scales=8, dev=DEV):
    """train_contrastive_feature.py:145-226 without the q_trans of :228."""
    sam_masks = original_masks.to(dev).float()                                               # :148
    mask_scales = mask_scales.to(dev)                                                        # :152
    mask_scales, sort_indices = torch.sort(mask_scales, descending=True)                     # :154
    sam_masks = sam_masks[sort_indices, :, :]                                                # :155
    sampled_scale_index = torch.randperm(len(mask_scales))[:num_sampled_scales]              # :159
    tmp = torch.zeros(num_sampled_scales + 2)                                                # :161-166
    tmp[1:len(sampled_scale_index) + 1] = sampled_scale_index
    tmp[-1] = len(mask_scales) - 1
    tmp[0] = -1
    sampled_scale_index = tmp.long()
    sampled_scales = mask_scales[sampled_scale_index]                                        # :168
    second_big_scale = mask_scales[mask_scales < upper_bound_scale].max()                    # :170
    rate = ray_sample_rate if ray_sample_rate > 0 else num_sampled_rays / (sam_masks.shape[-1] * sam_masks.shape[-2])
    sampled_ray = torch.rand(sam_masks.shape[-2], sam_masks.shape[-1]).to(dev) < rate        # :174
    non_mask_region = sam_masks.sum(dim=0) == 0                                              # :175
    sampled_ray = torch.logical_and(sampled_ray, ~non_mask_region)                           # :177
    per_pixel_mask_size = sam_masks * sam_masks.sum(-1).sum(-1)[:, None, None]               # :180
    per_pixel_mean_mask_size = per_pixel_mask_size.sum(dim=0) / (sam_masks.sum(dim=0) + 1e-9)
    per_pixel_mean_mask_size = per_pixel_mean_mask_size[sampled_ray]                         # :184
    pixel_to_pixel_mask_size = per_pixel_mean_mask_size.unsqueeze(0) * per_pixel_mean_mask_size.unsqueeze(1)
    ptp_max_size = pixel_to_pixel_mask_size.max()
    pixel_to_pixel_mask_size[pixel_to_pixel_mask_size == 0] = 1e10
    per_pixel_weight = torch.clamp(ptp_max_size / pixel_to_pixel_mask_size, 1.0, None)
    per_pixel_weight = (per_pixel_weight - per_pixel_weight.min()) / (per_pixel_weight.max() - per_pixel_weight.min()) * 9. + 1.
    sam_masks_sampled_ray = sam_masks[:, sampled_ray]                                        # :193
    gt_corrs = []
    sampled_scales[0] = upper_bound_scale + upper_bound_scale * torch.rand(1)[0]             # :197
    for idx, si in enumerate(sampled_scale_index):                                           # :198-221
        upper_bound = sampled_scales[idx] >= upper_bound_scale
        if si != len(mask_scales) - 1 and not upper_bound:
            sampled_scales[idx] -= (sampled_scales[idx] - mask_scales[si + 1]) * torch.rand(1)[0]
        elif upper_bound:
            sampled_scales[idx] -= (sampled_scales[idx] - second_big_scale) * torch.rand(1)[0]
        else:
            sampled_scales[idx] -= sampled_scales[idx] * torch.rand(1)[0]
        gt_vec = _reference_gt_vec(sam_masks_sampled_ray, si, upper_bound)
        gt_corr = torch.einsum('nh,nj->hj', gt_vec, gt_vec)
        gt_corr[gt_corr != 0] = 1
        gt_corrs.append(gt_corr)
    gt_corrs = torch.stack(gt_corrs, dim=0)                                                  # :226
    return sampled_ray, sampled_scales, gt_corrs, per_pixel_weight


def _reference_gt_vec(sam_masks_sampled_ray, si, upper_bound):
    """train_contrastive_feature.py:207-218: one scale's gt_vec (M sorted masks, S rays) from the sorted masks at the rays."""
    if not upper_bound:
        gt_vec = torch.zeros_like(sam_masks_sampled_ray)
        gt_vec[:si + 1, :] = sam_masks_sampled_ray[:si + 1, :]
        for j in range(si, -1, -1):
            gt_vec[j, :] = torch.logical_and(torch.logical_not(gt_vec[j + 1:, :].any(dim=0)), gt_vec[j, :])
        gt_vec[si + 1:, :] = sam_masks_sampled_ray[si + 1:, :]
    else:
        gt_vec = sam_masks_sampled_ray
    return gt_vec


def _reference_loss(scale_conditioned_features_sam, gt_corrs, per_pixel_weight):
    """train_contrastive_feature.py:255-299: the first two terms of the loss, the cosine statistics, the pair classes and the
    selected pair counts."""
    corr = torch.einsum('nhc,njc->nhj', scale_conditioned_features_sam, scale_conditioned_features_sam)   # :256
    diag_mask = torch.eye(corr.shape[1], dtype=bool, device=corr.device)
    sum_0 = gt_corrs.sum(dim=0)                                                              # :260
    consistent_negative = sum_0 == 0
    consistent_positive = sum_0 == len(gt_corrs)
    inconsistent = torch.logical_not(torch.logical_or(consistent_negative, consistent_positive))
    inconsistent_num = inconsistent.count_nonzero()
    sampled_num = inconsistent_num / 2
    rand_num = torch.rand_like(sum_0)                                                        # :266
    sampled_positive = torch.logical_and(consistent_positive, rand_num < sampled_num / consistent_positive.count_nonzero())
    sampled_negative = torch.logical_and(consistent_negative, rand_num < sampled_num / consistent_negative.count_nonzero())
    sampled_mask_positive = torch.logical_or(torch.logical_or(
        sampled_positive, torch.any(torch.logical_and(corr < 0.75, gt_corrs == 1), dim=0)), inconsistent)
    sampled_mask_positive = torch.logical_and(sampled_mask_positive, ~diag_mask)
    sampled_mask_positive = torch.triu(sampled_mask_positive, diagonal=0).bool()
    sampled_mask_negative = torch.logical_or(torch.logical_or(
        sampled_negative, torch.any(torch.logical_and(corr > 0.5, gt_corrs == 0), dim=0)), inconsistent)
    sampled_mask_negative = torch.logical_and(sampled_mask_negative, ~diag_mask)
    sampled_mask_negative = torch.triu(sampled_mask_negative, diagonal=0).bool()
    per_pixel_weight = per_pixel_weight.unsqueeze(0)
    loss = (- per_pixel_weight[:, sampled_mask_positive] * gt_corrs[:, sampled_mask_positive] * corr[:, sampled_mask_positive]).mean() \
        + (per_pixel_weight[:, sampled_mask_negative] * (1 - gt_corrs[:, sampled_mask_negative]) * torch.relu(corr[:, sampled_mask_negative])).mean()
    with torch.no_grad():
        cosine_pos = corr[gt_corrs == 1].mean()
        cosine_neg = corr[gt_corrs == 0].mean()
    counts = torch.stack([consistent_positive.count_nonzero(), consistent_negative.count_nonzero(), inconsistent.count_nonzero()])
    return loss, cosine_pos, cosine_neg, counts, sampled_mask_positive.count_nonzero(), sampled_mask_negative.count_nonzero()


# ---- inputs --------------------------------------------------------------------------------------------------------------------

def synthetic_masks(M, H, W, seed, dev=DEV, full=False):
    """M seeded nested rectangles (each inside its parent, parents earlier) on the CPU, and scales growing with their size."""
    g = torch.Generator().manual_seed(seed)
    boxes = []
    for m in range(M):
        if full:
            boxes.append((0, H, 0, W))
            continue
        if m == 0 or torch.rand(1, generator=g).item() < 0.3:
            py0, py1, px0, px1 = 0, H, 0, W
        else:
            py0, py1, px0, px1 = boxes[int(torch.randint(0, m, (1,), generator=g))]
        hh = max(1, int((py1 - py0) * (0.2 + 0.75 * torch.rand(1, generator=g).item())))
        ww = max(1, int((px1 - px0) * (0.2 + 0.75 * torch.rand(1, generator=g).item())))
        y0 = py0 + int(torch.randint(0, py1 - py0 - hh + 1, (1,), generator=g))
        x0 = px0 + int(torch.randint(0, px1 - px0 - ww + 1, (1,), generator=g))
        boxes.append((y0, y0 + hh, x0, x0 + ww))
    b = torch.tensor(boxes, device=dev)
    ys = torch.arange(H, device=dev)[None, :, None]
    xs = torch.arange(W, device=dev)[None, None, :]
    masks = ((ys >= b[:, 0, None, None]) & (ys < b[:, 1, None, None]) & (xs >= b[:, 2, None, None]) & (xs < b[:, 3, None, None])).cpu()
    area = ((b[:, 1] - b[:, 0]) * (b[:, 3] - b[:, 2])).float().cpu()
    scales = (area.sqrt() / max(H, W) * (0.9 + 0.2 * torch.rand(M, generator=g))).float()
    return masks, scales


def _dyadic(N, S, C, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-4, 5, (N, S, C), generator=g).float() / 16).to(DEV)


def _both(masks, scales, ub, seed, feats_fn, num_sampled_rays):
    """The new path and the restated reference from the same RNG state: targets, loss, d loss / d features."""
    torch.manual_seed(seed)
    tg = sample_contrastive_targets(masks, scales, ub, num_sampled_rays=num_sampled_rays)
    feats = feats_fn(tg.num_scales, tg.num_rays).requires_grad_(True)
    cuda_state = torch.cuda.get_rng_state(DEV)
    loss, stats = contrastive_loss(feats, tg)
    (g_new,) = torch.autograd.grad(loss, feats)

    torch.manual_seed(seed)
    sampled_ray, sampled_scales, gt_corrs, weight = _reference_targets(masks, scales, ub, num_sampled_rays=num_sampled_rays)
    torch.cuda.set_rng_state(cuda_state, DEV)
    feats_r = feats.detach().clone().requires_grad_(True)
    ref = _reference_loss(feats_r, gt_corrs, weight)
    (g_ref,) = torch.autograd.grad(ref[0], feats_r)
    return tg, loss, stats, g_new, sampled_ray, sampled_scales, ref, g_ref


# ---- 1. exact arithmetic -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 5, 64, 65, 130])
@pytest.mark.parametrize("tie", [False, True])
def test_exact_arithmetic(M, tie):
    """Dyadic features (integers in [-4, 4] / 16, C = 32): every corr is exact in any order, so every selection is the
    reference's.  Index -1 and M - 1 are always sampled, 0 pads M < 8; `tie` puts a second mask at the upper bound."""
    H, W = 48, 150
    masks, scales = synthetic_masks(M, H, W, seed=M)
    ub = float(scales.max())
    if M == 1:
        ub = float(scales[0]) * 1.5
    elif tie:
        top = torch.argsort(scales, descending=True)[:2]
        scales[top[1]] = scales[top[0]]
    tg, loss, stats, g_new, sampled_ray, sampled_scales, ref, g_ref = _both(
        masks, scales, ub, 100 + M, lambda N, S: _dyadic(N, S, 32, M), num_sampled_rays=200)
    loss_r, cos_pos_r, cos_neg_r, counts_r, n_pos_r, n_neg_r = ref
    assert torch.equal(tg.sampled_ray, sampled_ray)
    assert torch.equal(tg.sampled_scales.view(torch.int32), sampled_scales.view(torch.int32))
    assert tg.num_rays > 20
    assert torch.equal(stats.class_counts, counts_r)
    assert int(stats.n_pos) == int(n_pos_r) and int(stats.n_neg) == int(n_neg_r)
    torch.testing.assert_close(loss, loss_r, rtol=1e-6, atol=0, equal_nan=True)
    torch.testing.assert_close(stats.cosine_pos, cos_pos_r, rtol=1e-5, atol=1e-6, equal_nan=True)
    torch.testing.assert_close(stats.cosine_neg, cos_neg_r, rtol=1e-5, atol=1e-6, equal_nan=True)
    torch.testing.assert_close(g_new, g_ref, rtol=1e-5, atol=1e-6 * float(g_ref.nan_to_num().abs().max()) + 1e-12, equal_nan=True)


# ---- 2. full size, same seed ---------------------------------------------------------------------------------------------------

def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


def _time(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


@pytest.mark.gpu
def test_full_size_same_seed():
    H, W, M, C = 1080, 1920, 120, 32
    masks, scales = synthetic_masks(M, H, W, seed=120)
    ub = float(scales.max())

    def unit(N, S):
        g = torch.Generator().manual_seed(5)
        return torch.nn.functional.normalize(torch.randn(N, S, C, generator=g), dim=-1).to(DEV)

    tg, loss, stats, g_new, sampled_ray, sampled_scales, ref, g_ref = _both(masks, scales, ub, 7, unit, num_sampled_rays=1000)
    loss_r, cos_pos_r, cos_neg_r, counts_r, n_pos_r, n_neg_r = ref
    assert torch.equal(tg.sampled_ray, sampled_ray)
    assert torch.equal(tg.sampled_scales.view(torch.int32), sampled_scales.view(torch.int32))
    assert 800 < tg.num_rays < 1200
    assert torch.equal(stats.class_counts, counts_r)
    assert abs(int(stats.n_pos) - int(n_pos_r)) <= 4 and abs(int(stats.n_neg) - int(n_neg_r)) <= 4
    torch.testing.assert_close(loss, loss_r, rtol=1e-4, atol=0)
    torch.testing.assert_close(stats.cosine_pos, cos_pos_r, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(stats.cosine_neg, cos_neg_r, rtol=1e-5, atol=1e-6)
    # norm-wise, and per ray (row) with an allowance for the rows of pairs whose selection flipped at 0.75 / 0.5
    assert float((g_new - g_ref).norm() / g_ref.norm()) <= 1e-4
    row_err = (g_new - g_ref).norm(dim=(0, 2)) / g_ref.norm(dim=(0, 2)).clamp_min(1e-30)
    assert int((row_err > 1e-4).sum()) <= 2 * 4 + 2 * abs(int(stats.n_pos) - int(n_pos_r)) + 2 * abs(int(stats.n_neg) - int(n_neg_r))

    feats = unit(tg.num_scales, tg.num_rays).requires_grad_(True)

    def new():
        t = sample_contrastive_targets(masks, scales, ub, num_sampled_rays=1000)
        f = feats if t.num_rays == feats.shape[1] else unit(t.num_scales, t.num_rays).requires_grad_(True)
        loss, _ = contrastive_loss(f, t)
        loss.backward()
        return loss

    def old():
        _, _, gt, w = _reference_targets(masks, scales, ub, num_sampled_rays=1000)
        f = feats if gt.shape[1] == feats.shape[1] else unit(gt.shape[0], gt.shape[1]).requires_grad_(True)
        loss = _reference_loss(f, gt, w)[0]
        loss.backward()
        return loss

    torch.manual_seed(1)
    _, peak_new = _peak(new)
    torch.manual_seed(1)
    _, peak_old = _peak(old)
    t_new, t_old = _time(new), _time(old)
    print(f"\ncontrastive targets + loss fwd/bwd at 1080p, M=120, S~1000: new {t_new:.2f} ms, peak +{peak_new / 2**20:.0f} MiB; "
          f"reference restated {t_old:.2f} ms, peak +{peak_old / 2**20:.0f} MiB")
    assert peak_new <= 0.2 * peak_old
    assert t_new < t_old


# ---- 3. through the front end --------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_through_front_end():
    H, W, M, C, h, w = 120, 200, 40, 32, 60, 100
    masks, scales = synthetic_masks(M, H, W, seed=3)
    ub = float(scales.max())
    g = torch.Generator().manual_seed(11)
    rendered = torch.randn(C, h, w, generator=g).to(DEV).requires_grad_(True)
    gates = torch.rand(10, C, generator=g).to(DEV).requires_grad_(True)

    torch.manual_seed(21)
    tg = sample_contrastive_targets(masks, scales, ub, num_sampled_rays=300)
    cuda_state = torch.cuda.get_rng_state(DEV)
    feats, _ = contrastive_front_end(rendered, (H, W), tg.sampled_ray, gates)
    loss, _ = contrastive_loss(feats, tg)
    g_new = torch.autograd.grad(loss, [rendered, gates])

    torch.manual_seed(21)
    sampled_ray, _, gt_corrs, weight = _reference_targets(masks, scales, ub, num_sampled_rays=300)
    assert torch.equal(sampled_ray, tg.sampled_ray)
    torch.cuda.set_rng_state(cuda_state, DEV)
    r = torch.nn.functional.interpolate(rendered.unsqueeze(0), (H, W), mode='bilinear').squeeze(0)   # :237
    fws = r.unsqueeze(0).repeat([gates.shape[0], 1, 1, 1]) * gates.unsqueeze(-1).unsqueeze(-1)       # :247-248
    s = fws[:, :, sampled_ray].permute([0, 2, 1])                                                    # :250-252
    s = torch.nn.functional.normalize(s, dim=-1, p=2)                                                # :254
    loss_r = _reference_loss(s, gt_corrs, weight)[0]
    g_ref = torch.autograd.grad(loss_r, [rendered, gates])
    torch.testing.assert_close(loss, loss_r, rtol=1e-4, atol=0)
    for a, b in zip(g_new, g_ref):
        assert float((a - b).norm() / b.norm()) <= 1e-4


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_deterministic():
    H, W, M, C = 200, 300, 70, 32
    masks, scales = synthetic_masks(M, H, W, seed=4)
    packed = pack_sam_masks(masks, device=DEV)
    ub = float(scales.max())
    outs = []
    for _ in range(2):
        torch.manual_seed(9)
        tg = sample_contrastive_targets(packed, scales, ub, num_sampled_rays=600)
        g = torch.Generator().manual_seed(1)
        f = torch.nn.functional.normalize(torch.randn(tg.num_scales, tg.num_rays, C, generator=g), dim=-1).to(DEV).requires_grad_(True)
        loss, stats = contrastive_loss(f, tg)
        (gr,) = torch.autograd.grad(loss, f)
        outs.append((loss, gr, stats.cosine_pos, stats.cosine_neg))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 5. degenerate cases -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_degenerate_cases_give_nan():
    H, W, C = 64, 96, 32
    # no rays: S = 0
    masks, scales = synthetic_masks(6, H, W, seed=5)
    torch.manual_seed(0)
    tg = sample_contrastive_targets(masks, scales, float(scales.max()), num_sampled_rays=0)
    assert tg.num_rays == 0
    f = torch.zeros(tg.num_scales, 0, C, device=DEV, requires_grad=True)
    loss, _ = contrastive_loss(f, tg)
    (gr,) = torch.autograd.grad(loss, f)
    assert torch.isnan(loss) and gr.shape == f.shape
    # one mask over the whole image: every pair weight equal, (w - min) / (max - min) = NaN
    masks, scales = synthetic_masks(1, H, W, seed=6, full=True)
    torch.manual_seed(0)
    tg = sample_contrastive_targets(masks, scales, float(scales[0]) * 1.5, num_sampled_rays=100)
    assert tg.num_rays > 10
    g = torch.Generator().manual_seed(2)
    f = torch.nn.functional.normalize(torch.randn(tg.num_scales, tg.num_rays, C, generator=g), dim=-1).to(DEV).requires_grad_(True)
    loss, _ = contrastive_loss(f, tg)
    (gr,) = torch.autograd.grad(loss, f)
    torch.cuda.synchronize()
    assert torch.isnan(loss)
