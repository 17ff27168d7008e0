"""GPU checks of the CLIP tiles (seganygaussians_amd/clip_tiles.py; resize_sam_masks and mask_index_map of sam_masks.py; DESIGN.md
section 24) against the restatement (tests/clip_tiles_ref.py) and the reference's own crops (tests/golden/clip_tiles/clip_tiles.npz).

The tolerance against tiles_ref64 is derived, not tuned.  Plane values lie in [0, 1]; the float32 weights are non-negative and sum
to 1 within rounding.  The kernel sums w_j v_j in float32 in ascending source column, then the width-pass values times their height
weights in ascending source row; a float32 sum of n such products errs by at most 2 n 2^-24 (n roundings of products, n of sums, every
partial sum <= 1), the weights' divisions and their sum's distance from 1 by at most 4 more units.  So an element with n_x and n_y
taps errs by at most 2 (n_x + n_y + 4) 2^-24 before the normalisation, that / std_c after it, plus 2^-23 |want| for the subtraction
and the division; a float16 result adds 2^-11 |want| for its one conversion.  Each resize case is also held against F.interpolate +
normalise on the CPU on the same planes -- the reference's operation itself -- with twice the allowance, because both sides round."""
import numpy as np
import pytest
import torch

from seganygaussians_amd import clip_tiles as ct
from seganygaussians_amd import sam_masks
from seganygaussians_amd.contrastive_loss import pack_sam_masks
from tests import clip_tiles_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def check_tiles(image, masks, size=(224, 224), layout="crop", background=None, antialias=True, mean=ref.CLIP_MEAN, std=ref.CLIP_STD,
                dtype=torch.float32, rects=None, inclusive=False, interpolate=True):
    """clip_tiles against tiles_ref64 within the bound, against F.interpolate within twice the bound, invalid tiles exactly.
    Returns (tiles, valid) on the CPU."""
    masks = np.asarray(masks, dtype=bool)
    kw = dict(size=size, layout=layout, background=background, antialias=antialias, mean=mean, std=std, dtype=dtype)
    if rects is None:
        want_rects, want_valid = ref.rects_ref(masks, inclusive)
        tiles, valid = ct.clip_tiles(image, torch.from_numpy(masks).to(DEV), inclusive=inclusive, **kw)
    else:
        want_rects, want_valid = ref.mark_valid(rects, masks.reshape(len(masks), -1).any(axis=1))
        tiles, valid = ct.clip_tiles(image, torch.from_numpy(masks).to(DEV), rects=torch.as_tensor(np.asarray(rects), dtype=torch.int32).to(DEV), **kw)
    assert tiles.shape == (len(masks), 3) + tuple(size) and tiles.dtype == dtype and tiles.device == DEV and valid.dtype == torch.bool
    tiles, valid = tiles.cpu(), valid.cpu()
    np.testing.assert_array_equal(valid.numpy(), want_valid)
    bg = {"crop": 1.0, "pad_square": 0.0}[layout] if background is None else background
    worst = worst_i = 0.0
    for m in range(len(masks)):
        got = tiles[m].double().numpy()
        if not want_valid[m]:
            fill = torch.from_numpy(ref.normalised_background(bg, mean, std)).to(dtype)[:, None, None].expand(3, *size)
            assert torch.equal(tiles[m], fill), m
            continue
        plane = ref.plane_ref(image, masks[m], want_rects[m], layout, bg)
        want, bound = ref.tiles_ref64(plane, size, antialias, mean, std)
        if dtype == torch.float16:
            bound = ref.half_bound(want, bound)
        ratio = np.abs(got - want) / bound
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), (m, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
        if interpolate:
            ratio = np.abs(got - ref.tiles_interpolate(plane, size, antialias, mean, std).astype(np.float64)) / (2.0 * bound)
            worst_i = max(worst_i, float(ratio.max()))
            assert (ratio <= 1.0).all(), (m, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
    print(f"clip_tiles {image.shape} M={len(masks)} {size} {layout} aa={antialias} {dtype}: max error / bound {worst:.3f}, "
          f"against F.interpolate / (2 bound) {worst_i:.3f}")
    return tiles, valid


def random_image(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("antialias", [True, False])
def test_corner_mask_in_the_last_word(antialias):
    """A 2 x 2 mask in the last corner of a 5 x 65 image: the last word of a row holds one bit.  The exclusive slice is a 1 x 1 crop,
    a constant tile; inclusive=True a 2 x 2 crop."""
    image = random_image(5, 65, 1)
    masks = np.zeros((1, 5, 65), bool)
    masks[0, 3:, 63:] = True
    tiles, valid = check_tiles(image, masks, size=(9, 11), antialias=antialias)
    assert valid.all()
    want = (torch.from_numpy(image[3, 63].astype(np.float32)) / 255.0 - torch.tensor(ref.CLIP_MEAN)) / torch.tensor(ref.CLIP_STD)
    if antialias:   # one tap of weight w / w = 1; without antialias the two taps coincide and v l0 + v l1 rounds
        assert torch.equal(tiles[0], want[:, None, None].expand(3, 9, 11))
    tiles, valid = check_tiles(image, masks, size=(9, 11), antialias=antialias, inclusive=True)
    assert valid.all() and len(torch.unique(tiles[0, 0])) > 1


@pytest.mark.parametrize("antialias", [True, False])
def test_identity_resize_is_exact(antialias):
    image = random_image(16, 24, 2)
    masks = np.ones((1, 16, 24), bool)
    tiles, valid = check_tiles(image, masks, size=(16, 24), antialias=antialias, mean=(0, 0, 0), std=(1, 1, 1), inclusive=True)
    plane = ref.plane_ref(image, masks[0], (0, 0, 24, 16))
    assert valid.all() and torch.equal(tiles[0], torch.from_numpy(plane).permute(2, 0, 1))


@pytest.mark.parametrize("antialias", [True, False])
def test_one_row_crop_across_words(antialias):
    """A one-row mask from x = 63 to x = 193: the crop starts at the last bit of a word and runs through the next ones."""
    image = random_image(4, 200, 3)
    masks = np.zeros((1, 4, 200), bool)
    masks[0, 2, 63:194] = True
    masks[0, 2, 100:110] = False
    tiles, valid = check_tiles(image, masks, size=(6, 50), antialias=antialias, inclusive=True)
    assert valid.all()
    _, valid = check_tiles(image, masks, size=(6, 50), antialias=antialias)   # the exclusive slice of one row is empty
    assert not valid.any()


@pytest.mark.parametrize("size,antialias", [((224, 224), True), ((224, 224), False), ((7, 5), True), ((7, 5), False)])
def test_tall_crop_many_height_taps(size, antialias):
    """A 1200 x 8 crop: at size (7, 5) an output row has 343 or more height taps with antialias; the same code, only slower."""
    image = random_image(1200, 8, 4)
    masks = np.ones((1, 1200, 8), bool)
    masks[0, 5::7, 3] = False
    if antialias and size == (7, 5):
        assert max(len(w) for _, w in ref.aa_weights(1200, 7)) >= 343
    check_tiles(image, masks, size=size, antialias=antialias, inclusive=True)


@pytest.mark.parametrize("antialias", [True, False])
def test_wide_crop_in_chunks_and_two_column_sets(antialias):
    """A 2086-pixel-wide crop is staged in three chunks of 1024 pixels, with taps on both sides of a chunk's end; 300 output columns
    are two column sets of the 256 threads."""
    image = random_image(3, 2100, 12)
    masks = np.random.default_rng(12).random((1, 3, 2100)) < 0.8
    masks[0, :, :5] = masks[0, :, 2091:] = False
    masks[0, 1, 5] = masks[0, 1, 2090] = True
    check_tiles(image, masks, size=(3, 300), antialias=antialias, inclusive=True)
    check_tiles(image, masks, size=(2, 7), antialias=antialias, dtype=torch.float16)


@pytest.mark.parametrize("background", [1.0, 0.0, 0.5])
def test_checkerboard_mask_and_backgrounds(background):
    image = random_image(70, 130, 5)
    ys, xs = np.mgrid[:70, :130]
    masks = np.stack([(ys + xs) % 2 == 0, ((ys // 3 + xs // 5) % 2 == 0) & (ys > 10) & (xs < 97)])
    check_tiles(image, masks, size=(37, 41), background=background, inclusive=True)
    check_tiles(image, masks, size=(224, 224), background=background, antialias=False)


def test_1024_masks():
    image = random_image(2, 70, 6)
    masks = np.random.default_rng(6).random((1024, 2, 70)) < 0.05
    masks[17] = False
    tiles, valid = check_tiles(image, masks, size=(4, 4), inclusive=True)
    assert not valid[17] and valid.sum() > 900


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("layout", ["crop", "pad_square"])
def test_empty_and_one_row_masks_are_invalid(layout, dtype):
    image = random_image(9, 70, 7)
    masks = np.zeros((3, 9, 70), bool)
    masks[1, 4, 10:30] = True      # one row: the exclusive slice has no row
    masks[2, 2:7, 60:68] = True
    for background in (None, 0.5):
        _, valid = check_tiles(image, masks, size=(8, 12), layout=layout, background=background, dtype=dtype)
        assert valid.tolist() == [False, False, True]


@pytest.mark.parametrize("antialias", [True, False])
@pytest.mark.parametrize("box", [(3, 2, 10, 20), (3, 2, 30, 10), (5, 4, 16, 15)])   # [X0, Y0, X1, Y1): 18 x 7, 8 x 27, 11 x 11
def test_pad_square(box, antialias):
    """pad_img: ch > cw and cw > ch with an odd difference each, and a square crop."""
    image = random_image(24, 40, 8)
    masks = np.zeros((1, 24, 40), bool)
    masks[0, box[1]:box[3], box[0]:box[2]] = np.random.default_rng(8).random((box[3] - box[1], box[2] - box[0])) < 0.7
    masks[0, box[1], box[0]] = masks[0, box[3] - 1, box[2] - 1] = True
    ch, cw = box[3] - box[1], box[2] - box[0]
    assert (ch - cw) % 2 == 1 or ch == cw
    for dtype in (torch.float32, torch.float16):
        check_tiles(image, masks, size=(20, 23), layout="pad_square", antialias=antialias, inclusive=True, dtype=dtype)
    check_tiles(image, masks, size=(20, 23), layout="pad_square", background=0.5, antialias=antialias)


def test_rects_that_leave_the_image():
    image = random_image(12, 70, 9)
    masks = np.random.default_rng(9).random((4, 12, 70)) < 0.6
    masks[3] = False
    rects = [[-5, -3, 20, 9], [50, 6, 80, 20], [0, 0, 70, 12], [2, 2, 9, 9]]   # two sides each; the whole image; an empty mask's
    for layout in ("crop", "pad_square"):
        _, valid = check_tiles(image, masks, size=(16, 18), layout=layout, rects=rects)
        assert valid.tolist() == [True, True, True, False]
    _, valid = check_tiles(image, masks, size=(5, 5), rects=[[4, 4, 4, 9], [9, 3, 2, 7], [0, 0, 1, 40000], [0, 0, 5, 5]], interpolate=False)
    assert not valid.any()   # empty, reversed, longer than 32768, an empty mask


def test_options_and_bookkeeping():
    image = random_image(20, 70, 10)
    masks = torch.from_numpy(np.random.default_rng(10).random((5, 20, 70)) < 0.3)
    packed = pack_sam_masks(masks, device=DEV)
    for dtype in (torch.float16, torch.float32):
        a, va = ct.clip_tiles(image, packed, size=(30, 28), dtype=dtype)
        out = torch.full((5, 3, 30, 28), 7.0, device=DEV, dtype=dtype)
        b, vb = ct.clip_tiles(torch.from_numpy(image).to(DEV), masks, size=(30, 28), dtype=dtype, out=out)   # CPU masks, GPU image
        assert b is out and torch.equal(a, b) and torch.equal(va, vb) and a.dtype == dtype   # two runs, bit-identical
        c, _ = ct.clip_tiles(torch.from_numpy(image), masks.to(DEV), size=(30, 28), dtype=dtype)
        assert torch.equal(a, c)
    a, _ = ct.clip_tiles(image, packed)
    assert a.shape == (5, 3, 224, 224) and a.dtype == torch.float16
    with pytest.raises(ValueError, match="resize_sam_masks"):
        ct.clip_tiles(image[:10], packed)
    with pytest.raises(ValueError, match="uint8"):
        ct.clip_tiles(torch.from_numpy(image).to(DEV).float(), packed)
    with pytest.raises(ValueError, match="out must be"):
        ct.clip_tiles(image, packed, out=torch.empty((5, 3, 224, 224), device=DEV, dtype=torch.float32))
    with pytest.raises(ValueError, match="out must be"):
        ct.clip_tiles(image, packed, out=torch.empty((5, 3, 224, 224), dtype=torch.float16))
    with pytest.raises(ValueError, match="rects must be"):
        ct.clip_tiles(image, packed, rects=torch.zeros((5, 4), device=DEV, dtype=torch.int64))
    with pytest.raises(ValueError, match="rects must be"):
        ct.clip_tiles(image, packed, rects=torch.zeros((4, 4), device=DEV, dtype=torch.int32))
    with pytest.raises(ValueError, match="the rects on cpu"):
        ct.clip_tiles(image, packed, rects=torch.zeros((5, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="inclusive"):
        ct.clip_tiles(image, packed, rects=torch.zeros((5, 4), device=DEV, dtype=torch.int32), inclusive=True)


def test_every_golden_crop():
    """Per mask of every golden case, with size set to the recorded crop's shape, mean 0, std 1 and float32, the tile IS the crop
    the reference handed to its encoder."""
    n = 0
    for k, case in enumerate(ref.load_cases()):
        image, masks = case["image"], torch.from_numpy(case["masks"])
        at_size = sam_masks.resize_sam_masks(masks, image.shape[:2])   # a copy in the even cases, :99-102 in the odd ones
        bits = torch.from_numpy(ref.resize_masks_ref(case["masks"], image.shape[:2])).to(DEV)
        assert torch.equal(pack_sam_masks(bits, device=DEV).words, at_size.words), k
        image_gpu = torch.from_numpy(image).to(DEV)
        for m, crop in enumerate(case["crops"]):
            for antialias in (True, False):
                tiles, valid = ct.clip_tiles(image_gpu, bits[m:m + 1], size=crop.shape[1:], background=case["background"],
                                             antialias=antialias, mean=(0, 0, 0), std=(1, 1, 1), dtype=torch.float32)
                assert bool(valid[0]) and torch.equal(tiles[0].cpu(), torch.from_numpy(crop)), (k, m, antialias)
            n += 1
    assert n >= 24


# ---- resize_sam_masks --------------------------------------------------------------------------------------------------------------

def seeded_masks(shape, seed):
    rng = np.random.default_rng(seed)
    h, w = shape
    rect = np.zeros((h, w), bool)
    rect[h // 4:h // 4 + max(1, h // 2), w // 5:w // 5 + max(1, w // 2)] = True
    return np.concatenate([rng.random((5, h, w)) < 0.5, rect[None]])


@pytest.mark.parametrize("src,dst", [((7, 63), (24, 130)), ((12, 35), (24, 70)), ((13, 37), (24, 70)), ((1, 1), (3, 64)),
                                     ((24, 130), (24, 130)), ((23, 129), (7, 37))])
def test_resize_sam_masks_every_bit(src, dst):
    """Bits equal F.interpolate(masks.float(), size, mode='bilinear') > 0.5 on the CPU.  No float64 value of these cases lies within
    2^-20 of 0.5 (asserted), so float32 rounding cannot decide a bit and equality is demanded of every one.  (23, 129) -> (7, 37)
    downsamples with non-dyadic ratios on both axes."""
    masks = seeded_masks(src, 7)
    assert np.abs(ref.resize_values64(masks, dst) - 0.5).min() >= 2.0 ** -20
    want = torch.from_numpy(ref.resize_masks_ref(masks, dst))
    for given in (torch.from_numpy(masks), pack_sam_masks(torch.from_numpy(masks), device=DEV)):
        got = sam_masks.resize_sam_masks(given, dst)
        assert got.shape == (6,) + dst and got.words.shape == (6, dst[0], (dst[1] + 63) // 64)
        assert torch.equal(got.words, pack_sam_masks(want.to(DEV), device=DEV).words)   # padding bits 0 on both sides
    if src == dst:
        assert torch.equal(got.words, given.words) and got.words.data_ptr() != given.words.data_ptr()   # a copy
    assert int(want.sum()) > 0 and not bool(want.all())


# ---- mask_index_map ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("offset", [0, 37])
@pytest.mark.parametrize("shape", [(1, 1, 1), (33, 5, 65), (70, 7, 63), (1024, 2, 70)])
def test_mask_index_map_is_the_numpy_loop(shape, offset):
    M, h, w = shape
    masks = np.random.default_rng(M).random(shape) < (0.5 if M == 1 else 2.0 / M)
    if M > 1:
        masks[M // 2] = False   # an empty mask
        masks[M // 3] = True    # a full mask: nothing below it shows, and no pixel is left at -1
        masks[M // 3 + 1:, :, : w // 2 + 1] &= np.random.default_rng(1).random((M - M // 3 - 1, h, w // 2 + 1)) < 0.3
    want = ref.index_map_ref(masks, offset)
    got = sam_masks.mask_index_map(torch.from_numpy(masks).to(DEV), offset=offset)
    assert got.dtype == torch.int32 and got.device == DEV
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    holes = masks.copy()
    holes[:, :, ::3] = False    # columns that no mask covers: -1, without the offset
    out = torch.empty((h, w), device=DEV, dtype=torch.int32)
    assert sam_masks.mask_index_map(pack_sam_masks(torch.from_numpy(holes), device=DEV), offset=offset, out=out) is out
    np.testing.assert_array_equal(out.cpu().numpy(), ref.index_map_ref(holes, offset))
    assert (out[:, ::3] == -1).all()
    with pytest.raises(ValueError, match="out must be"):
        sam_masks.mask_index_map(torch.from_numpy(masks).to(DEV), out=torch.empty((h, w), device=DEV, dtype=torch.int64))


# ---- the drop-in -------------------------------------------------------------------------------------------------------------------

class StubClip:
    """What get_features_from_image_and_masks needs of the reference's OpenCLIPNetwork: .model.encode_image."""
    class model:
        calls = []

        @staticmethod
        def encode_image(x):
            StubClip.model.calls.append(tuple(x.shape))
            return x.float().mean((2, 3))


@pytest.mark.parametrize("half_size", [False, True])
def test_dropin_features(half_size):
    """Against the reference's per-mask formulation (clip_utils/__init__.py:99-173, clip_utils/clip_utils.py:60-68) written with
    torch operations on the CPU.  The stub's feature is the mean of a tile, so it errs by no more than the largest element bound of
    the tile -- float16 tiles on both sides, hence twice -- plus the float32 mean's own rounding, 16 x 2^-24 x max |tile| for the 2^16
    elements of a pairwise sum."""
    H, W = 24, 90
    image = random_image(H, W, 11)
    h, w = (H // 2, W // 2) if half_size else (H, W)
    masks = seeded_masks((h, w), 11)
    masks[2] = False          # the reference raises at an empty mask; here its row is NaN
    masks[4, h // 2:] = False
    StubClip.model.calls = []
    feats = ct.get_features_from_image_and_masks(StubClip, image, torch.from_numpy(masks), background=0.5, batch=4)
    assert feats.device.type == "cpu" and feats.shape == (6, 3) and StubClip.model.calls == [(4, 3, 224, 224), (2, 3, 224, 224)]
    assert torch.isnan(feats[2]).all() and not torch.isnan(feats[[0, 1, 3, 4, 5]]).any()
    F = torch.nn.functional
    m = F.interpolate(torch.from_numpy(masks).unsqueeze(0).float(), (H, W), mode="bilinear").squeeze(0)
    m = (m > 0.5).float()
    keep = m.unsqueeze(-1)                                                  # :108 in float32: the image inside, 255 x 0.5 outside
    masked = keep * torch.from_numpy(image).unsqueeze(0) + (1 - keep) * 127.5
    boxes = ref.boxes_ref(m.numpy() != 0)
    mean, std = torch.tensor(ref.CLIP_MEAN)[:, None, None], torch.tensor(ref.CLIP_STD)[:, None, None]
    for i in (0, 1, 3, 4, 5):
        x0, y0, x1, y1 = (int(v) for v in boxes[i])
        crop = masked[i][y0:y1, x0:x1, :][None].permute(0, 3, 1, 2) / 255.0
        tile = ((F.interpolate(crop, (224, 224), mode="bilinear", align_corners=False, antialias=True)[0] - mean) / std).half()
        want64, bound = ref.tiles_ref64(crop[0].permute(1, 2, 0).numpy(), (224, 224), True)
        allow = 2.0 * ref.half_bound(want64, bound).max(axis=(1, 2)) + 16 * 2.0 ** -24 * np.abs(want64).max(axis=(1, 2))
        err = np.abs(feats[i].double().numpy() - tile.float().mean((1, 2)).double().numpy())
        print(f"drop-in mask {i}: error / allowance {float((err / allow).max()):.3f}")
        assert (err <= allow).all(), (i, err, allow)
