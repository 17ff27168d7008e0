"""CPU checks of the SAM-mask scales: the float64 restatement (tests/mask_scales_ref.py) against the literal lines of
get_scale.py:128-157, input refusals before any launch, and the exports.  No GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

from seganygaussians_amd import _lib, build
from seganygaussians_amd.contrastive_loss import PackedSamMasks
from seganygaussians_amd.mask_scales import erode_sam_masks, sam_mask_scales
from tests.mask_scales_ref import grid_index, mask_scales_ref, points64


def literal_scales(depth, masks, FoVx, FoVy):
    """get_scale.py:128-157 as written, in f32 (masks as .float() at :107).  Needs M >= 2 (the .squeeze() of :152)."""
    corresponding_masks = masks.float()
    depth = depth.cpu().squeeze()                                                            # :128
    grid_index_ = grid_index(*depth.shape)                                                   # :130
    points_in_3D = torch.zeros(depth.shape[0], depth.shape[1], 3).cpu()                      # :132
    points_in_3D[:, :, -1] = depth                                                           # :133
    cx = depth.shape[1] / 2                                                                  # :136
    cy = depth.shape[0] / 2                                                                  # :137
    fx = cx / np.tan(FoVx / 2)                                                               # :138
    fy = cy / np.tan(FoVy / 2)                                                               # :139
    points_in_3D[:, :, 0] = (grid_index_[:, :, 0] - cx) * depth / fx                         # :142
    points_in_3D[:, :, 1] = (grid_index_[:, :, 1] - cy) * depth / fy                         # :143
    upsampled_mask = torch.nn.functional.interpolate(corresponding_masks.unsqueeze(1), mode='bilinear',
                                                     size=(depth.shape[0], depth.shape[1]), align_corners=False)   # :145
    eroded_masks = torch.conv2d(upsampled_mask.float(), torch.full((3, 3), 1.0).view(1, 1, 3, 3), padding=1)       # :147-151
    eroded_masks = (eroded_masks >= 5).squeeze()                                             # :152
    scale = torch.zeros(len(corresponding_masks))                                            # :154
    counts = torch.zeros(len(corresponding_masks), dtype=torch.int64)
    for mask_id in range(len(corresponding_masks)):                                          # :155
        point_in_3D_in_mask = points_in_3D[eroded_masks[mask_id] == 1]                       # :157
        counts[mask_id] = point_in_3D_in_mask.shape[0]
        scale[mask_id] = (point_in_3D_in_mask.std(dim=0) * 2).norm()                         # :159
    return eroded_masks, counts, scale


def synthetic_case(H, W, h, w, seed):
    """f32 depth with a zero patch, masks: random blobs, nested rectangles, a thin line (vanishes), one that leaves a single pixel,
    one over the zero-depth patch, one empty."""
    g = torch.Generator().manual_seed(seed)
    depth = 1.0 + 4.0 * torch.rand(H, W, generator=g)
    depth[: H // 4, : W // 4] = 0.0
    ms = []
    noise = torch.rand(h, w, generator=g)
    ms.append(noise > 0.3)
    for k in range(3):
        m = torch.zeros(h, w, dtype=torch.bool)
        m[k * h // 8: h - k * h // 8, k * w // 8: w - k * w // 8] = True
        ms.append(m)
    line = torch.zeros(h, w, dtype=torch.bool)
    line[h // 2, :] = True
    ms.append(line)
    single = torch.zeros(h, w, dtype=torch.bool)
    single[h // 2 - 1: h // 2 + 2, w // 2] = True   # a plus: only its centre has 5 set pixels in its window
    single[h // 2, w // 2 - 1: w // 2 + 2] = True
    ms.append(single)
    zero = torch.zeros(h, w, dtype=torch.bool)
    zero[: h // 4, : w // 4] = True
    ms.append(zero)
    ms.append(torch.zeros(h, w, dtype=torch.bool))
    return depth, torch.stack(ms)


@pytest.mark.parametrize("H,W,h,w", [(37, 53, 37, 53), (40, 24, 20, 12), (24, 40, 48, 80)])
def test_restatement_matches_literal_lines(H, W, h, w):
    depth, masks = synthetic_case(H, W, h, w, seed=H * W)
    fovx, fovy = 0.9, 0.7
    eroded, counts, scales, box = mask_scales_ref(depth, masks, fovx, fovy)
    lit_eroded, lit_counts, lit_scales = literal_scales(depth, masks, fovx, fovy)
    # same size or dyadic ratios: every box sum is exact in f32 and f64 alike, so the decisions agree bit for bit
    assert torch.equal(eroded, lit_eroded)
    assert torch.equal(counts, lit_counts)
    assert torch.equal(torch.isnan(scales), torch.isnan(lit_scales))
    ok = ~torch.isnan(scales)
    assert torch.allclose(lit_scales[ok].double(), scales[ok], rtol=1e-4, atol=1e-6)
    assert box.dtype == torch.float64 and box.shape == (masks.shape[0], H, W)
    if (h, w) != (H, W):
        return
    # the cases the masks were built for
    assert counts[4] == 0 and math.isnan(scales[4])                 # a 1-pixel line vanishes
    assert counts[5] == 1 and math.isnan(scales[5])                 # one point: torch's unbiased std is NaN
    assert counts[6] >= 2 and scales[6] == 0.0                      # depth 0: every point is the origin
    assert counts[7] == 0 and math.isnan(scales[7])


def test_axis_pairing_is_the_reference_one():
    H, W = 6, 10
    depth = torch.full((H, W), 2.0)
    fovx, fovy = 1.0, 0.5
    p = points64(depth, fovx, fovy)
    fx, fy = (W / 2) / math.tan(fovx / 2), (H / 2) / math.tan(fovy / 2)
    # x pairs the ROW index with W/2 and fx, y the column index with H/2 and fy (get_scale.py:142-143)
    assert p[4, 7, 0] == (4 - W / 2) * 2.0 / fx
    assert p[4, 7, 1] == (7 - H / 2) * 2.0 / fy
    assert p[4, 7, 2] == 2.0
    # and it changes the scale against a camera model with the usual pairing
    masks = torch.zeros(2, H, W, dtype=torch.bool)
    masks[0, 1:5, 1:9] = True
    masks[1] = True
    _, _, scales, _ = mask_scales_ref(depth, masks, fovx, fovy)
    yy, xx = grid_index(H, W).double().unbind(-1)
    usual = torch.stack([(xx - W / 2) * 2.0 / fx, (yy - H / 2) * 2.0 / fy, depth.double()], -1)
    eroded = mask_scales_ref(depth, masks, fovx, fovy)[0]
    assert not math.isclose(float(scales[0]), float((usual[eroded[0]].std(0) * 2).norm()), rel_tol=1e-3)


def test_single_mask_defined_by_the_same_formula():
    depth, masks = synthetic_case(20, 30, 20, 30, seed=5)
    _, counts2, scales2, _ = mask_scales_ref(depth, masks[1:3], 0.8, 0.6)
    _, counts1, scales1, _ = mask_scales_ref(depth, masks[1:2], 0.8, 0.6)
    assert counts1[0] == counts2[0] and scales1[0] == scales2[0]


def test_bad_inputs_refused_before_any_launch():
    cpu_depth = torch.ones(8, 8)
    masks = torch.zeros(2, 8, 8, dtype=torch.bool)
    with pytest.raises(ValueError, match="GPU"):
        sam_mask_scales(cpu_depth, masks, 1.0, 1.0)
    with pytest.raises(ValueError, match="float32"):
        sam_mask_scales(cpu_depth.double(), masks, 1.0, 1.0)
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        sam_mask_scales(torch.ones(2, 8, 8), masks, 1.0, 1.0)
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        sam_mask_scales(torch.ones(8), masks, 1.0, 1.0)
    with pytest.raises(ValueError):
        sam_mask_scales(np.ones((8, 8), np.float32), masks, 1.0, 1.0)
    with pytest.raises(ValueError, match="bool"):
        erode_sam_masks(masks.to(torch.uint8), (8, 8))
    with pytest.raises(ValueError, match="bool"):
        erode_sam_masks(masks[0], (8, 8))
    with pytest.raises(ValueError, match="1024"):
        erode_sam_masks(torch.zeros(1025, 1, 1, dtype=torch.bool), (1, 1))
    with pytest.raises(ValueError, match="size"):
        erode_sam_masks(masks, (0, 8))
    with pytest.raises(ValueError, match="size"):
        erode_sam_masks(masks, 8)
    with pytest.raises(ValueError, match="PackedSamMasks"):
        erode_sam_masks(PackedSamMasks(torch.zeros(2, 8, 2, dtype=torch.int64), (2, 8, 8)), (8, 8))
    with pytest.raises(ValueError, match="1024"):
        erode_sam_masks(PackedSamMasks(torch.zeros(1025, 1, 1, dtype=torch.int64), (1025, 1, 1)), (1, 1))
    with pytest.raises(ValueError):
        erode_sam_masks("masks", (8, 8))


def test_abi_exported_and_checks_arguments():
    build.build_library()
    L = _lib.load()
    assert _lib.DECLARED["mi_mask_scales.h"] == ["mi_mask_scales_workspace_bytes", "mi_mask_erode", "mi_mask_erode_min_sum", "mi_mask_scales",
                                                 "mi_mask_resize"]
    for name in ("mi_mask_scales_workspace_bytes", "mi_mask_erode", "mi_mask_scales"):
        assert name in _lib.ALL_EXPORTS
        assert ctypes.cast(getattr(L, name), ctypes.c_void_p).value
    # M ceil(H / 16) ceil(W / 64) tiles of 5 doubles
    assert L.mi_mask_scales_workspace_bytes(120, 1080, 1920) == 120 * 68 * 30 * 5 * 8
    assert L.mi_mask_scales_workspace_bytes(0, 1080, 1920) == 0
    # argument checks run before any launch: no device needed
    assert L.mi_mask_erode(1025, 4, 4, 8, 4, 4, 4096, None) != 0 and "1024" in _lib.last_error()
    assert L.mi_mask_erode(2, 4, 4, None, 4, 4, None, None) != 0 and "null" in _lib.last_error()
    assert L.mi_mask_erode(2, 4, 4, 4096, 4, 4, 4096 + 8, None) != 0 and "overlap" in _lib.last_error()
    assert L.mi_mask_scales(2, 4, 4, 8, 8, 1.0, 1.0, 8, 8, 8, 8, None) != 0 and "workspace" in _lib.last_error()
    assert L.mi_mask_scales(2, 4, 4, 8, 8, 0.0, 1.0, 8, 1 << 20, 8, 8, None) != 0 and "focal" in _lib.last_error()
    assert L.mi_mask_scales(0, 4, 4, 8, 8, 1.0, 1.0, 8, 1 << 20, 8, 8, None) != 0


def test_module_exports():
    import seganygaussians_amd.mask_scales as ms
    assert callable(ms.erode_sam_masks) and callable(ms.sam_mask_scales)
