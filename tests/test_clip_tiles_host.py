"""CPU checks of the CLIP tiles (seganygaussians_amd/clip_tiles.py, resize_sam_masks and mask_index_map of sam_masks.py; DESIGN.md
section 24): the restatement (tests/clip_tiles_ref.py) against the reference's own crops (tests/golden/clip_tiles/clip_tiles.npz,
written by tests/golden/make_clip_tiles_golden.py), its two weight tables against F.interpolate, the exports, and the refusals that
come before any launch.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from seganygaussians_amd import _lib, build, clip_tiles, sam_masks
from tests import clip_tiles_ref as ref


@pytest.fixture(scope="module")
def golden():
    return ref.load_cases()


def test_restatement_reproduces_every_recorded_crop(golden):
    assert len(golden) == 12
    assert {c["background"] for c in golden} == {1.0, 0.0, 0.5}
    resized = crops = 0
    for k, case in enumerate(golden):
        image, masks = case["image"], case["masks"]
        assert image.dtype == np.uint8 and image.shape[0] == 24 and 70 <= image.shape[1] <= 130 and 2 <= len(masks) <= 8
        resized += masks.shape[1:] != image.shape[:2]
        up = ref.resize_masks_ref(masks, image.shape[:2])   # clip_utils/__init__.py:99-102
        rects, valid = ref.rects_ref(up)                    # :115, :157, :168
        assert valid.all() and len(case["crops"]) == len(masks)
        for m, crop in enumerate(case["crops"]):
            want = ref.plane_ref(image, up[m], rects[m], "crop", case["background"]).transpose(2, 0, 1)   # :108, :173
            assert crop.dtype == np.float32 and crop.shape == want.shape and min(crop.shape[1:]) >= 1, (k, m)
            np.testing.assert_array_equal(want, crop, err_msg=f"case {k} mask {m}")
            crops += 1
    assert resized == 6 and crops >= 24   # half of the cases give the masks at half size


@pytest.mark.parametrize("antialias", [True, False])
@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (37, 53), (225, 223), (1000, 7)])
def test_weight_tables_match_interpolate(shape, antialias):
    """Both weight tables, contracted in float64, against F.interpolate on the CPU on [0, 1] data, within the bound of
    tiles_ref64 at mean 0 and std 1 (the resize alone)."""
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    plane = rng.random(shape + (3,), dtype=np.float32)
    want, bound = ref.tiles_ref64(plane, (224, 224), antialias, mean=(0, 0, 0), std=(1, 1, 1))
    got = ref.tiles_interpolate(plane, (224, 224), antialias, mean=(0, 0, 0), std=(1, 1, 1))
    ratio = np.abs(got - want) / bound
    print(f"{shape} -> 224 x 224 antialias={antialias}: max |diff| {np.abs(got - want).max():.2e}, max diff / bound {ratio.max():.3f}")
    assert (ratio <= 1.0).all()
    n_taps = [len(w) for _, w in ref.weights(shape[0], 224, antialias)]
    assert all(abs(float(np.sum(w, dtype=np.float64)) - 1.0) < 1e-6 for _, w in ref.weights(shape[0], 224, antialias))
    assert max(n_taps) >= (2 * shape[0] // 224 if antialias else 1)


def test_identity_resize_weights_are_exact():
    """At the same size both tables are the identity: weight 1 on the pixel itself (and 0 on its neighbour)."""
    for antialias in (True, False):
        Wm, _ = ref.dense(ref.weights(16, 16, antialias), 16)
        np.testing.assert_array_equal(Wm, np.eye(16))


def test_plane_layouts():
    image = np.arange(6 * 9 * 3, dtype=np.uint8).reshape(6, 9, 3)
    mask = np.zeros((6, 9), bool)
    mask[1:5, 2:5] = True
    mask[2, 3] = False
    crop = ref.plane_ref(image, mask, (2, 1, 5, 5), "crop")                # 4 x 3, background 1.0
    assert crop.shape == (4, 3, 3) and (crop[1, 1] == 1.0).all() and crop[0, 0, 0] == np.float32(image[1, 2, 0]) / np.float32(255)
    pad = ref.plane_ref(image, mask, (2, 1, 5, 5), "pad_square")           # ch > cw: L = 4, the crop at column (4 - 3) // 2 = 0
    assert pad.shape == (4, 4, 3) and (pad[:, 3] == 0.0).all() and np.array_equal(pad[0, 0], crop[0, 0])
    pad = ref.plane_ref(image, mask, (2, 1, 5, 2), "pad_square")           # cw > ch: L = 3, the crop at row (3 - 1) // 2 = 1
    assert pad.shape == (3, 3, 3) and (pad[0] == 0.0).all() and (pad[2] == 0.0).all() and np.array_equal(pad[1], crop[0])
    out = ref.plane_ref(image, mask, (-2, -1, 4, 3), "crop", 0.5)          # leaves the image on two sides
    assert out.shape == (4, 6, 3) and (out[0] == 0.5).all() and (out[:, :2] == 0.5).all() and np.array_equal(out[2, 4], crop[0, 0])
    np.testing.assert_array_equal(ref.index_map_ref(np.stack([mask, ~mask & (np.arange(9) < 3)[None]]), 5)[:2, :4],
                                  [[6, 6, 6, -1], [6, 6, 5, 5]])


def test_exports_resolve_and_one_includer():
    build.build_library()
    L = _lib.load()
    names = ["mi_mask_resize", "mi_mask_clip_tiles", "mi_mask_index_map"]
    assert _lib.DECLARED["mi_clip_tiles.h"] == names[1:] and _lib.DECLARED["mi_mask_scales.h"][-1] == names[0]      # resize: next to its definition
    for name in names:
        assert name in _lib.ALL_EXPORTS
        assert ctypes.cast(getattr(L, name), ctypes.c_void_p).value
    for name in ("clip_tiles", "get_features_from_image_and_masks"):
        assert callable(getattr(clip_tiles, name))
    for name in ("resize_sam_masks", "mask_index_map"):
        assert callable(getattr(sam_masks, name))
    assert clip_tiles.CLIP_MEAN == ref.CLIP_MEAN and clip_tiles.CLIP_STD == ref.CLIP_STD
    hdr = open(next(h for h in build.HEADERS if os.path.basename(h) == "mi_clip_tiles.h")).read()
    assert f"#define MI_CLIP_TILES_MAX_SIZE {clip_tiles.MAX_SIZE}\n" in hdr and clip_tiles.MAX_SIZE >= 336
    assert f"#define MI_CLIP_TILES_MAX_SIDE {clip_tiles.MAX_SIDE}\n" in hdr and clip_tiles.MAX_SIDE == ref.MAX_SIDE
    includers = [f for f in build.SOURCES if '"clip_tiles.h"' in open(os.path.join(build.SRC_DIR, f)).read()]
    assert includers == ["mi_clip_tiles.hip"]
    includers = [f for f in build.SOURCES if '"mask_scales.h"' in open(os.path.join(build.SRC_DIR, f)).read()]
    assert includers == ["mi_mask_scales.hip"]


def test_abi_refuses_bad_arguments_before_any_launch():
    """Refused calls of every new entry point, with their messages; the pointers are never read, so no device is needed."""
    build.build_library()
    L = _lib.load()
    three = (ctypes.c_float * 3)(1, 1, 1)
    # csrc/mi_clip_tiles.hip
    assert L.mi_mask_clip_tiles(0, 4, 4, 8, 8, 8, 0, 1.0, 1, three, three, 224, 224, 1, 8, None) != 0
    assert _lib.last_error() == "clip tiles: need 1 <= M <= 1024 masks and H, W >= 1"
    assert L.mi_mask_clip_tiles(2, 4096, 4096, 8, 8, 8, 0, 1.0, 1, three, three, 224, 224, 1, 8, None) != 0
    assert _lib.last_error() == "clip tiles: need H * W < 2^24 pixels"
    for size in ((0, 224), (224, 513)):
        assert L.mi_mask_clip_tiles(2, 4, 4, 8, 8, 8, 0, 1.0, 1, three, three, size[0], size[1], 1, 8, None) != 0
        assert _lib.last_error() == "clip tiles: need 1 <= Sh, Sw <= 512 (MI_CLIP_TILES_MAX_SIZE)"
    assert L.mi_mask_clip_tiles(2, 4, 4, 8, 8, 8, 2, 1.0, 1, three, three, 224, 224, 1, 8, None) != 0
    assert _lib.last_error() == "clip tiles: layout must be MI_CLIP_TILES_CROP or MI_CLIP_TILES_PAD_SQUARE"
    assert L.mi_mask_clip_tiles(2, 4, 4, 8, 8, None, 0, 1.0, 1, three, three, 224, 224, 1, 8, None) != 0
    assert _lib.last_error() == "clip tiles: null pointer"
    assert L.mi_mask_clip_tiles(2, 4, 4, 8, 8, 8, 0, float("nan"), 1, three, three, 224, 224, 1, 8, None) != 0
    assert _lib.last_error() == "clip tiles: background is NaN"
    zero = (ctypes.c_float * 3)(1, 0, 1)
    assert L.mi_mask_clip_tiles(2, 4, 4, 8, 8, 8, 0, 1.0, 1, three, zero, 224, 224, 1, 8, None) != 0
    assert _lib.last_error() == "clip tiles: need mean and std without NaN and std != 0"
    assert L.mi_mask_index_map(1025, 4, 4, 8, 0, 8, None) != 0
    assert _lib.last_error() == "clip tiles: need 1 <= M <= 1024 masks and H, W >= 1"
    assert L.mi_mask_index_map(2, 4, 4, 8, -1, 8, None) != 0
    assert _lib.last_error() == "mask index map: need 0 <= offset <= 2^31 - 1 - 1024"
    assert L.mi_mask_index_map(2, 4, 4, 8, 0, None, None) != 0 and _lib.last_error() == "clip tiles: null pointer"
    # csrc/mi_mask_scales.hip: mi_mask_resize
    assert L.mi_mask_resize(0, 4, 4, 8, 4, 4, 0.5, 4096, None) != 0
    assert _lib.last_error() == "mask scales: need 1 <= M <= 1024 masks and h, w >= 1"
    assert L.mi_mask_resize(2, 4, 4, 8, 4096, 4096, 0.5, 4096, None) != 0
    assert _lib.last_error() == "mask resize: need h * w and H * W < 2^24 pixels"
    assert L.mi_mask_resize(2, 4, 4, 8, 4, 4, float("nan"), 4096, None) != 0 and _lib.last_error() == "mask resize: threshold is NaN"
    assert L.mi_mask_resize(2, 4, 4, 4096, 4, 4, 0.5, 4096 + 8, None) != 0
    assert _lib.last_error() == "mask resize: the resized masks must not overlap the input masks"


def test_python_refusals_before_any_launch():
    b = lambda *shape: torch.zeros(*shape, dtype=torch.bool)
    img = torch.zeros(4, 6, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="resize_sam_masks"):
        clip_tiles.clip_tiles(img, b(2, 2, 3))
    with pytest.raises(ValueError, match="uint8"):
        clip_tiles.clip_tiles(img.float(), b(2, 4, 6))
    with pytest.raises(ValueError, match="uint8"):
        clip_tiles.clip_tiles(np.zeros((4, 6), np.uint8), b(2, 4, 6))
    with pytest.raises(ValueError, match="1 <= Sh, Sw <= 512"):
        clip_tiles.clip_tiles(img, b(2, 4, 6), size=(224, 513))
    with pytest.raises(ValueError, match="positive"):
        clip_tiles.clip_tiles(img, b(2, 4, 6), size=(0, 224))
    with pytest.raises(ValueError, match="layout"):
        clip_tiles.clip_tiles(img, b(2, 4, 6), layout="pad")
    with pytest.raises(ValueError, match="float16 or torch.float32"):
        clip_tiles.clip_tiles(img, b(2, 4, 6), dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="NaN"):
        clip_tiles.clip_tiles(img, b(2, 4, 6), background=float("nan"))
    with pytest.raises(ValueError, match="three numbers"):
        clip_tiles.clip_tiles(img, b(2, 4, 6), mean=(0.5, 0.5))
    with pytest.raises(ValueError, match="std must not be 0"):
        clip_tiles.clip_tiles(img, b(2, 4, 6), std=(1, 0, 1))
    with pytest.raises(ValueError, match="bool"):
        clip_tiles.clip_tiles(img, torch.zeros(2, 4, 6))
    with pytest.raises(ValueError, match="1 <= M <= 1024"):
        clip_tiles.clip_tiles(img, b(1025, 4, 6))
    for call in (lambda m: sam_masks.resize_sam_masks(m, (8, 8)), lambda m: sam_masks.mask_index_map(m)):
        with pytest.raises(ValueError, match="1 <= M <= 1024"):
            call(b(0, 4, 4))
        with pytest.raises(ValueError, match=r"h \* w < 2\^24"):
            call(b(1, 4096, 4096))
        with pytest.raises(ValueError, match="bool"):
            call(torch.zeros(2, 4, 4))
    with pytest.raises(ValueError, match=r"H \* W < 2\^24"):
        sam_masks.resize_sam_masks(b(1, 4, 4), (4096, 4096))
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        sam_masks.resize_sam_masks(b(1, 4, 4), 8)
    with pytest.raises(ValueError, match="NaN"):
        sam_masks.resize_sam_masks(b(1, 4, 4), (8, 8), threshold=float("nan"))
    for offset in (-1, 1 << 31, 1.5, True):
        with pytest.raises(ValueError, match="offset"):
            sam_masks.mask_index_map(b(1, 4, 4), offset=offset)
