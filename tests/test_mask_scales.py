"""GPU tests of the SAM-mask scales (seganygaussians_amd/mask_scales.py) against the float64 restatement of
get_scale.py:128-159 (tests/mask_scales_ref.py): the erosion bit for bit at the same size and at dyadic ratios, within rounding of
the threshold otherwise; counts exactly, scales within 1e-5 relative, NaN where the restatement has NaN; determinism and input
forms; the full 1080p chain from the depth drop-in."""
import math

import numpy as np
import pytest
import torch

from seganygaussians_amd.contrastive_loss import PackedSamMasks, pack_sam_masks
from seganygaussians_amd.mask_scales import erode_sam_masks, sam_mask_scales
from tests.mask_scales_ref import box_sums64, mask_scales_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def unpack(p: PackedSamMasks) -> torch.Tensor:
    """PackedSamMasks -> bool (M, H, W) on the CPU."""
    M, H, W = p.shape
    words = p.words.cpu()
    bits = (words[..., None] >> torch.arange(64)) & 1
    return bits.reshape(M, H, -1)[:, :, :W].bool()


def assert_padding_zero(p: PackedSamMasks):
    M, H, W = p.shape
    if W % 64:
        pad = p.words[:, :, -1].cpu() >> (W % 64)
        assert not pad.any(), "padding bits set"


def patterns(H, W, seed):
    """Random masks, lines of width 1..3 both ways, full and empty, bits on the border and on the word seams."""
    g = torch.Generator().manual_seed(seed)
    ms = [torch.rand(H, W, generator=g) < p for p in (0.5, 0.8, 0.95)]
    for k in (1, 2, 3):
        m = torch.zeros(H, W, dtype=torch.bool)
        m[H // 2: H // 2 + k, :] = True
        ms.append(m)
        m = torch.zeros(H, W, dtype=torch.bool)
        m[:, W // 2: W // 2 + k] = True
        ms.append(m)
    ms.append(torch.ones(H, W, dtype=torch.bool))
    ms.append(torch.zeros(H, W, dtype=torch.bool))
    border = torch.zeros(H, W, dtype=torch.bool)
    border[:2, :] = border[-2:, :] = border[:, :2] = border[:, -2:] = True
    ms.append(border)
    ms.append(~border)
    seams = torch.zeros(H, W, dtype=torch.bool)
    for c in (62, 63, 64, 65, 126, 127, 128, 129):
        if c < W:
            seams[:, c] = True
    ms.append(seams)
    ms.append(seams | (torch.rand(H, W, generator=g) < 0.6))
    return torch.stack(ms)


@pytest.mark.parametrize("W", [1, 2, 63, 64, 65, 127, 128, 129, 1920])
def test_erode_same_size_bit_exact(W):
    H = 9 if W == 1920 else 13
    masks = patterns(H, W, seed=W)
    got = erode_sam_masks(masks, (H, W))
    want = box_sums64(masks, (H, W)) >= 5
    assert got.shape == (masks.shape[0], H, W)
    assert torch.equal(unpack(got), want)
    assert_padding_zero(got)
    # the same from packed masks on the device
    got2 = erode_sam_masks(pack_sam_masks(masks, device=DEV), (H, W))
    assert torch.equal(got2.words, got.words)


@pytest.mark.parametrize("h,w,H,W", [(11, 70, 22, 140), (9, 33, 36, 132), (24, 130, 12, 65), (1, 1, 4, 4)])
def test_erode_dyadic_bit_exact(h, w, H, W):
    masks = patterns(h, w, seed=h * w)
    got = erode_sam_masks(masks, (H, W))
    want = box_sums64(masks, (H, W)) >= 5    # dyadic weights: every box sum is exact
    assert torch.equal(unpack(got), want)
    assert_padding_zero(got)


@pytest.mark.parametrize("h,w,H,W,M", [(20, 30, 30, 45, 18), (10, 12, 30, 36, 18), (720, 1280, 1080, 1920, 3)])
def test_erode_non_dyadic_within_rounding(h, w, H, W, M):
    masks = patterns(h, w, seed=h + w)[:M]
    got = unpack(erode_sam_masks(masks, (H, W)))
    box = box_sums64(masks, (H, W))
    differ = got != (box >= 5)
    assert not differ[(box - 5).abs() >= 1e-5].any()


def scene(H, W, seed):
    """A depth with a zero patch and a far region, and masks: blobs, nested rectangles, a thin line, a plus (one eroded pixel),
    a mask over depth 0, an empty mask, and a small mask far off-centre at large depth."""
    g = torch.Generator().manual_seed(seed)
    depth = 2.0 + 3.0 * torch.rand(H, W, generator=g)
    depth[: H // 5, W // 3: W // 2] = 0.0
    far = depth[-(H // 6):, -(W // 6):]
    far.copy_(300.0 + torch.rand(far.shape, generator=g))
    ms = [torch.rand(H, W, generator=g) < 0.7]
    for k in range(6):
        m = torch.zeros(H, W, dtype=torch.bool)
        m[k * H // 14: H - k * H // 14, k * W // 14: W - k * W // 14] = True
        ms.append(m)
    m = torch.zeros(H, W, dtype=torch.bool)
    m[H // 2, :] = True
    ms.append(m)
    m = torch.zeros(H, W, dtype=torch.bool)
    m[H // 2 - 1: H // 2 + 2, W // 3] = True
    m[H // 2, W // 3 - 1: W // 3 + 2] = True
    ms.append(m)
    m = torch.zeros(H, W, dtype=torch.bool)
    m[: H // 5, W // 3: W // 2] = True
    ms.append(m)
    ms.append(torch.zeros(H, W, dtype=torch.bool))
    far = torch.zeros(H, W, dtype=torch.bool)
    far[-8:-2, -8:-2] = True
    ms.append(far)
    return depth, torch.stack(ms)


FAR = -1   # index of the far small off-centre mask in scene()


def test_scales_and_counts_against_float64():
    H, W = 97, 203
    fovx, fovy = 1.1, 0.8
    depth, masks = scene(H, W, seed=7)
    _, counts, scales, _ = mask_scales_ref(depth, masks, fovx, fovy, keep_box=False)
    got, got_counts = sam_mask_scales(depth.to(DEV), masks, fovx, fovy, return_counts=True)
    assert got.dtype == torch.float32 and got.shape == (masks.shape[0],) and got.device == DEV
    assert torch.equal(got_counts.cpu(), counts)
    got = got.cpu().double()
    nan = torch.isnan(scales)
    assert torch.equal(torch.isnan(got), nan)
    assert nan.sum() >= 3                                   # the line, the plus and the empty mask
    ok = ~nan
    rel = ((got[ok] - scales[ok]).abs() / scales[ok].abs().clamp_min(1e-30))
    zero = scales[ok] == 0
    assert torch.all(got[ok][zero] == 0)                     # the mask over depth 0: every point is the origin
    assert rel[~zero].max() < 1e-5, rel.max()
    # the far mask is the case a one-pass f32 E[x^2] - E[x]^2 gets wrong
    from tests.mask_scales_ref import points64
    pts = points64(depth, fovx, fovy)[box_sums64(masks[FAR:], (H, W))[0] >= 5].float()
    n = pts.shape[0]
    one_pass = 2 * math.sqrt(max(float(((pts * pts).sum(0) - pts.sum(0) ** 2 / n).sum()) / (n - 1), 0.0))
    assert abs(one_pass - float(scales[FAR])) / float(scales[FAR]) > 1e-5
    assert abs(float(got[FAR]) - float(scales[FAR])) / float(scales[FAR]) < 1e-5


def test_single_mask():
    H, W = 40, 70
    depth, masks = scene(H, W, seed=3)
    _, counts, scales, _ = mask_scales_ref(depth, masks[1:2], 0.9, 0.9, keep_box=False)
    got, got_counts = sam_mask_scales(depth.to(DEV), masks[1:2], 0.9, 0.9, return_counts=True)
    assert got.shape == (1,) and int(got_counts[0]) == int(counts[0])
    assert abs(float(got[0]) - float(scales[0])) <= 1e-5 * float(scales[0])


def test_input_forms_and_determinism():
    H, W = 130, 257
    fovx, fovy = 1.0, 0.7
    depth, masks = scene(H, W, seed=11)
    d = depth.to(DEV)
    a = sam_mask_scales(d, masks, fovx, fovy)                                  # bool masks on the CPU
    b = sam_mask_scales(d, pack_sam_masks(masks, device=DEV), fovx, fovy)      # PackedSamMasks
    c = sam_mask_scales(d, masks.to(DEV), fovx, fovy)                          # bool masks on the device
    e = sam_mask_scales(d[None], masks, fovx, fovy)                            # (1, H, W) as the renderer returns it
    big = torch.zeros(H, 2 * W, device=DEV)
    big[:, ::2] = d
    f = sam_mask_scales(big[:, ::2], masks, fovx, fovy)                        # non-contiguous view
    g = sam_mask_scales(d.t().contiguous().t(), masks, fovx, fovy)             # transposed strides
    again = sam_mask_scales(d, masks, fovx, fovy)
    for x in (b, c, e, f, g, again):
        assert torch.equal(x.view(torch.int32), a.view(torch.int32))
    # resampled masks: the same through packed and bool inputs, and twice
    small = masks[:, ::2, ::2].contiguous()
    r1 = sam_mask_scales(d, small, fovx, fovy)
    r2 = sam_mask_scales(d, pack_sam_masks(small, device=DEV), fovx, fovy)
    assert torch.equal(r1.view(torch.int32), r2.view(torch.int32))


def test_refusals_on_the_device():
    d = torch.ones(8, 8, device=DEV)
    with pytest.raises(ValueError, match="fovx"):
        sam_mask_scales(d, torch.zeros(2, 8, 8, dtype=torch.bool), 0.0, 1.0)
    with pytest.raises(ValueError, match="1024"):
        sam_mask_scales(d, torch.zeros(1025, 8, 8, dtype=torch.bool), 1.0, 1.0)
    with pytest.raises(ValueError, match="bool"):
        sam_mask_scales(d, torch.zeros(2, 8, 8, dtype=torch.uint8), 1.0, 1.0)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="masks are on"):
            sam_mask_scales(d, torch.zeros(2, 8, 8, dtype=torch.bool, device="cuda:1"), 1.0, 1.0)


def test_full_size_chain_from_the_depth_dropin():
    import seganygaussians_amd
    from tests import helpers as hp
    from tests.test_contrastive_loss import synthetic_masks
    seganygaussians_amd.install_dropin()
    import diff_gaussian_rasterization_depth as mod

    inp = hp.inputs_from_config("cfg2", use_mask=True)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(DEV)
    settings = mod.GaussianRasterizationSettings(
        image_height=inp.image_height, image_width=inp.image_width, tanfovx=inp.tanfovx, tanfovy=inp.tanfovy, bg=t(inp.bg),
        scale_modifier=inp.scale_modifier, viewmatrix=t(inp.viewmatrix), projmatrix=t(inp.projmatrix), sh_degree=inp.sh_degree,
        campos=t(inp.campos), prefiltered=False, debug=False)
    with torch.no_grad():
        _, _, depth, _ = mod.GaussianRasterizer(raster_settings=settings)(
            means3D=t(inp.means3D), means2D=torch.zeros(inp.means3D.shape, device=DEV), shs=None, colors_precomp=t(inp.colors_precomp),
            opacities=t(inp.opacities), mask=t(inp.mask), scales=t(inp.scales), rotations=t(inp.rotations), cov3D_precomp=None)
    assert depth.shape == (1, 1080, 1920)
    assert float((depth > 0).float().mean()) > 0.2
    fovx, fovy = 2 * math.atan(inp.tanfovx), 2 * math.atan(inp.tanfovy)
    masks, _ = synthetic_masks(120, 1080, 1920, seed=120)
    got, got_counts = sam_mask_scales(depth, masks, fovx, fovy, return_counts=True)
    _, counts, scales, _ = mask_scales_ref(depth[0].cpu(), masks, fovx, fovy, keep_box=False)
    assert torch.equal(got_counts.cpu(), counts)
    got = got.cpu().double()
    assert torch.equal(torch.isnan(got), torch.isnan(scales))
    ok = ~torch.isnan(scales) & (scales > 0)
    assert ok.sum() > 100
    assert ((got[ok] - scales[ok]).abs() / scales[ok]).max() < 1e-5
