"""The packed SAM masks' Python home (seganygaussians_amd/packed_masks.py), called directly: the row width, what check_shape and
as_packed accept and the exact text of each refusal, and the old import paths.  CPU-only; a GPU tensor is stood in for by a CPU
tensor whose is_cuda and device say otherwise."""
import torch

from seganygaussians_amd import contrastive_loss, mask_scales, packed_masks
from seganygaussians_amd.packed_masks import PackedSamMasks
from tests.test_args_host import on_gpu, refuses


def test_row_words():
    assert [packed_masks.row_words(w) for w in (1, 63, 64, 65, 128, 129)] == [1, 1, 1, 2, 2, 3]


def test_old_import_paths_give_the_same_objects():
    for name in ("PackedSamMasks", "pack_sam_masks", "MAX_MASKS"):
        assert getattr(contrastive_loss, name) is getattr(packed_masks, name), name
    for name in ("PackedSamMasks", "pack_sam_masks", "MAX_MASKS", "MAX_PIXELS", "as_packed", "check_shape"):
        assert getattr(mask_scales, name) is getattr(packed_masks, name), name
    assert (packed_masks.MAX_MASKS, packed_masks.MAX_PIXELS) == (1024, 1 << 24)
    assert mask_scales.erode.__module__ == "seganygaussians_amd.mask_scales"   # a kernel call, not layout


def test_mask_dims_is_check_shape_without_the_pixel_limit():
    assert packed_masks.mask_dims("f", torch.zeros(3, 4, 6, dtype=torch.bool)) == (3, 4, 6)
    assert packed_masks.mask_dims("f", PackedSamMasks(None, (1, 4096, 4096))) == (1, 4096, 4096)
    with refuses("f: masks must be a bool (M, h, w) tensor or PackedSamMasks, got <class 'NoneType'> ()"):
        packed_masks.mask_dims("f", None)
    with refuses("f: need 1 <= M <= 1024 masks, got 1025"):
        packed_masks.mask_dims("f", PackedSamMasks(None, (1025, 1, 1)))


def test_check_shape():
    assert packed_masks.check_shape("f", torch.zeros(3, 4, 6, dtype=torch.bool)) is None
    assert packed_masks.check_shape("f", PackedSamMasks(torch.zeros(3, 4, 1, dtype=torch.int64), (3, 4, 6))) is None
    with refuses("f: masks must be a bool (M, h, w) tensor or PackedSamMasks, got torch.float32 (3, 4, 6)"):
        packed_masks.check_shape("f", torch.zeros(3, 4, 6))
    with refuses("f: masks must be a bool (M, h, w) tensor or PackedSamMasks, got torch.bool (4, 6)"):
        packed_masks.check_shape("f", torch.zeros(4, 6, dtype=torch.bool))
    with refuses("f: masks must be a bool (M, h, w) tensor or PackedSamMasks, got <class 'NoneType'> ()"):
        packed_masks.check_shape("f", None)
    with refuses("f: need 1 <= M <= 1024 masks, got 0"):
        packed_masks.check_shape("f", torch.zeros(0, 4, 6, dtype=torch.bool))
    with refuses("f: need 1 <= M <= 1024 masks, got 1025"):
        packed_masks.check_shape("f", PackedSamMasks(None, (1025, 1, 1)))
    with refuses("f: need h * w < 2^24 pixels, got 4096 x 4096"):
        packed_masks.check_shape("f", PackedSamMasks(None, (1, 4096, 4096)))


def test_as_packed(monkeypatch):
    dev = torch.device("cuda:0")
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64)
    words = on_gpu(i64(3, 4, 1))
    for d in (None, dev):
        got = packed_masks.as_packed("f", PackedSamMasks(words, (3, 4, 6)), d)
        assert isinstance(got, PackedSamMasks) and got.words.data_ptr() == words.data_ptr() and got.shape == (3, 4, 6)
    # masks on another GPU than the tensor they go with, under each of its three names (and the default)
    elsewhere = PackedSamMasks(on_gpu(i64(3, 4, 1), "cuda:1"), (3, 4, 6))
    with refuses("f: the masks are on cuda:1, the depth on cuda:0"):
        packed_masks.as_packed("f", elsewhere, dev)
    for versus in ("depth", "scores", "image"):
        with refuses(f"f: the masks are on cuda:1, the {versus} on cuda:0"):
            packed_masks.as_packed("f", elsewhere, dev, versus)
    masks = torch.zeros(3, 4, 6, dtype=torch.bool)
    for versus in ("depth", "scores", "image"):
        with refuses(f"f: the masks are on cuda:1, the {versus} on cuda:0"):
            packed_masks.as_packed("f", on_gpu(masks, "cuda:1"), dev, versus)
    # a bool tensor goes to pack_sam_masks with the device
    seen = []
    monkeypatch.setattr(packed_masks, "pack_sam_masks", lambda m, device=None: seen.append((m, device)) or "packed")
    assert packed_masks.as_packed("f", masks, dev) == "packed" and seen[0][0] is masks and seen[0][1] == dev
    assert packed_masks.as_packed("f", on_gpu(masks, "cuda:1"), None) == "packed" and seen[1][1] is None
    with refuses("f: need 1 <= M <= 1024 masks and a non-empty image, got (3, 0, 6)"):
        packed_masks.as_packed("f", PackedSamMasks(words, (3, 0, 6)), dev)
    with refuses("f: need 1 <= M <= 1024 masks and a non-empty image, got (1025, 4, 6)"):
        packed_masks.as_packed("f", PackedSamMasks(words, (1025, 4, 6)), dev)
    with refuses("f: PackedSamMasks words must be int64 (3, 4, 1) on a GPU, got torch.int64 (3, 4, 2) on cuda:0"):
        packed_masks.as_packed("f", PackedSamMasks(on_gpu(i64(3, 4, 2)), (3, 4, 6)), dev)
    with refuses("f: PackedSamMasks words must be int64 (3, 4, 1) on a GPU, got torch.int32 (3, 4, 1) on cuda:0"):
        packed_masks.as_packed("f", PackedSamMasks(on_gpu(i64(3, 4, 1).int()), (3, 4, 6)), dev)
    with refuses("f: PackedSamMasks words must be int64 (3, 4, 1) on a GPU, got torch.int64 (3, 4, 1) on cpu"):
        packed_masks.as_packed("f", PackedSamMasks(torch.zeros(3, 4, 1, dtype=torch.int64), (3, 4, 6)), dev)
    with refuses("f: masks must be a bool (M, h, w) tensor or PackedSamMasks, got torch.float32 (3, 4, 6)"):
        packed_masks.as_packed("f", torch.zeros(3, 4, 6), dev)
    with refuses("f: masks must be a bool (M, h, w) tensor or PackedSamMasks, got torch.bool (4, 6)"):
        packed_masks.as_packed("f", torch.zeros(4, 6, dtype=torch.bool), dev)
    with refuses("f: masks on meta; need the CPU or a GPU"):
        packed_masks.as_packed("f", torch.zeros(3, 4, 6, dtype=torch.bool, device="meta"), dev)
    with refuses("f: masks must be a bool (M, h, w) tensor or PackedSamMasks, got <class 'list'>"):
        packed_masks.as_packed("f", [[True]], dev)
