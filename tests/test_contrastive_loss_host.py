"""Host side of the contrastive loss (seganygaussians_amd/contrastive_loss.py): the scalar work of
train_contrastive_feature.py:156-174 and :197-206 draws the reference's random numbers in its order and gives its f32 bits;
bad inputs are refused before any launch; the library exports the loss's C-ABI.  No GPU."""
import ctypes

import pytest
import torch

from seganygaussians_amd import _lib, build, contrastive_loss as cl
from seganygaussians_amd.contrastive_loss import (PackedSamMasks, contrastive_loss, draw_sampled_scales, pack_sam_masks,
                                                  sample_contrastive_targets)


def _reference_scales(mask_scales, upper_bound_scale, H, W, num_sampled_scales=8):
    """train_contrastive_feature.py:156-174 and :197-206, restated on CPU tensors (the reference runs the scale arithmetic on
    device f32 tensors: one IEEE op per element, the same bits)."""
    mask_scales, sort_indices = torch.sort(mask_scales, descending=True)                  # :156
    sampled_scale_index = torch.randperm(len(mask_scales))[:num_sampled_scales]            # :160
    tmp = torch.zeros(num_sampled_scales + 2)                                              # :162-166
    tmp[1:len(sampled_scale_index) + 1] = sampled_scale_index
    tmp[-1] = len(mask_scales) - 1
    tmp[0] = -1
    sampled_scale_index = tmp.long()
    sampled_scales = mask_scales[sampled_scale_index]                                      # :168
    second_big_scale = mask_scales[mask_scales < upper_bound_scale].max()                  # :170
    ray_rand = torch.rand(H, W)                                                            # :174
    sampled_scales[0] = upper_bound_scale + upper_bound_scale * torch.rand(1)[0]           # :197
    upper = []
    for idx, si in enumerate(sampled_scale_index):                                         # :198-206
        upper_bound = sampled_scales[idx] >= upper_bound_scale
        upper.append(bool(upper_bound))
        if si != len(mask_scales) - 1 and not upper_bound:
            sampled_scales[idx] -= (sampled_scales[idx] - mask_scales[si + 1]) * torch.rand(1)[0]
        elif upper_bound:
            sampled_scales[idx] -= (sampled_scales[idx] - second_big_scale) * torch.rand(1)[0]
        else:
            sampled_scales[idx] -= sampled_scales[idx] * torch.rand(1)[0]
    return sampled_scale_index, torch.tensor(upper), sampled_scales, ray_rand


def _scales(M, seed, tie_upper=False):
    g = torch.Generator().manual_seed(seed)
    s = torch.rand(M, generator=g) * 3.0 + 0.01
    ub = float(s.max())
    if tie_upper and M > 2:
        s[0] = s[1] = s.max()   # a second mask at the upper bound: a non-zero sorted index whose scale equals upper_bound_scale
    if M == 1:
        ub = float(s[0]) * 1.5   # M = 1: the one scale lies below upper_bound_scale
    return s, ub


@pytest.mark.parametrize("M", [1, 3, 8, 9, 120])
@pytest.mark.parametrize("tie_upper", [False, True])
def test_draws_match_reference_bit_for_bit(M, tie_upper):
    scales, ub = _scales(M, 7 * M + tie_upper, tie_upper)
    H, W = 17, 23
    for seed in (0, 1, 12345):
        torch.manual_seed(seed)
        want_idx, want_ub, want_scales, want_rand = _reference_scales(scales.clone(), ub, H, W)
        want_state = torch.get_rng_state()

        torch.manual_seed(seed)
        sorted_scales, _ = torch.sort(scales.clone(), descending=True)
        ssi = torch.randperm(M)[:8]
        got_rand = torch.rand(H, W)
        idx, upper, got_scales = draw_sampled_scales(sorted_scales, ssi, ub)
        assert torch.equal(torch.get_rng_state(), want_state)
        assert torch.equal(got_rand, want_rand)
        assert torch.equal(idx, want_idx)
        assert torch.equal(upper, want_ub)
        assert got_scales.dtype == torch.float32
        assert torch.equal(got_scales.view(torch.int32), want_scales.view(torch.int32))
        assert bool(upper[0])
        if tie_upper and M > 2:
            assert int((sorted_scales >= ub).sum()) >= 2


def test_tied_upper_bound_index_is_an_upper_bound():
    # sorted index 1 has the upper-bound scale: that scale is an upper bound although its index is not -1
    s = torch.tensor([2.0, 1.0, 2.0, 0.5])
    sorted_scales, _ = torch.sort(s, descending=True)
    torch.manual_seed(3)
    idx, upper, _ = draw_sampled_scales(sorted_scales, torch.tensor([1, 2]), 2.0, num_sampled_scales=2)
    assert idx.tolist() == [-1, 1, 2, 3]
    assert upper.tolist() == [True, True, False, False]


def test_no_scale_below_upper_bound_raises():
    with pytest.raises(ValueError, match="second_big_scale"):
        draw_sampled_scales(torch.tensor([2.0, 2.0]), torch.tensor([0, 1]), 2.0)
    with pytest.raises(ValueError, match="second_big_scale"):
        draw_sampled_scales(torch.tensor([1.0]), torch.tensor([0]), 1.0)


def test_bad_inputs_refused_before_any_launch():
    with pytest.raises(ValueError):
        pack_sam_masks(torch.zeros(2, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        pack_sam_masks(torch.zeros(4, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="1024"):
        pack_sam_masks(torch.zeros(1025, 1, 1, dtype=torch.bool))
    with pytest.raises(ValueError):
        pack_sam_masks(torch.zeros(2, 4, 4, dtype=torch.bool), device="cpu")
    with pytest.raises(ValueError):
        draw_sampled_scales(torch.tensor([1.0], dtype=torch.float64), torch.tensor([0]), 2.0)
    packed = PackedSamMasks(torch.zeros(3, 4, 1, dtype=torch.int64), (3, 4, 4))
    with pytest.raises(ValueError, match="mask_scales"):
        sample_contrastive_targets(packed, torch.ones(4), 1.0)
    with pytest.raises(ValueError, match="mask_scales"):
        sample_contrastive_targets(packed, torch.ones(3, dtype=torch.float64), 1.0)
    with pytest.raises(ValueError, match="sampled scales"):
        sample_contrastive_targets(packed, torch.ones(3), 1.0, num_sampled_scales=31)
    with pytest.raises(ValueError):
        sample_contrastive_targets(torch.zeros(3, 4, 4), torch.ones(3), 1.0)
    with pytest.raises(ValueError, match="sample_contrastive_targets"):
        contrastive_loss(torch.zeros(10, 4, 32), object())


def test_loss_abi_exported():
    build.build_library()
    L = _lib.load()
    names = ["mi_contrastive_pack_masks", "mi_contrastive_cover", "mi_contrastive_targets", "mi_contrastive_loss_forward",
             "mi_contrastive_loss_backward"]
    assert _lib.DECLARED["mi_contrastive.h"][2:] == names            # the header's second section: the loss itself
    assert (cl.MAX_MASKS, cl.MAX_SCALES) == (1024, 32) == (_lib.MI_CONTRASTIVE_LOSS_MAX_MASKS, _lib.MI_CONTRASTIVE_LOSS_MAX_SCALES)
    for name in names:
        assert name in _lib.ALL_EXPORTS
        assert ctypes.cast(getattr(L, name), ctypes.c_void_p).value
    # argument checks run before any launch: no device needed
    assert L.mi_contrastive_pack_masks(1025, 4, 4, None, None, None) != 0
    assert "1024" in _lib.last_error()
    assert L.mi_contrastive_loss_forward(10, 33, 32, 4, None, None, None, None, None, None, None, None, None) != 0
    assert L.mi_contrastive_loss_forward(10, 10, 257, 4, None, None, None, None, None, None, None, None, None) != 0
    assert "256" in _lib.last_error()
