"""CPU checks of the SAM-mask set operations (seganygaussians_amd/sam_masks.py): the float32 restatement of
mask_nms (tests/sam_masks_ref.py) against the reference's own selections (tests/golden/sam_masks/sam_masks.npz, written by
tests/golden/make_sam_masks_golden.py), the exports, and the refusals that come before any launch.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from seganygaussians_amd import _lib, build, sam_masks
from seganygaussians_amd.contrastive_loss import PackedSamMasks
from tests import sam_masks_ref as ref


@pytest.fixture(scope="module")
def golden():
    return ref.load_cases()


def test_restatement_reproduces_every_reference_selection(golden):
    assert len(golden) >= 60
    thresholds = {thr for _, _, thr, _ in golden}
    assert thresholds == {(0.7, 0.1, 0.2), (0.8, 0.7, 0.5)}   # the defaults and sam_utils.py:210
    mixed = 0
    for c, (masks, scores, thr, selected) in enumerate(golden):
        assert len(np.unique(scores)) == len(scores)
        got = ref.mask_nms_ref(masks, scores, *thr)
        np.testing.assert_array_equal(got, selected, err_msg=f"case {c}: M={len(scores)} thresholds={thr}")
        mixed += 0 < len(selected) < len(scores)
    assert 2 * mixed >= len(golden)


def test_every_test_of_the_decision_decides_somewhere(golden):
    """Across the fixture each of the four tests (IoU, score, upper inner, lower inner) is the sole reason for a rejection."""
    sole = np.zeros(4, np.int64)
    for masks, scores, thr, _ in golden:
        s, idx = torch.sort(torch.from_numpy(scores), descending=True, stable=True)
        inter, areas = ref.overlaps_ref(masks, idx.numpy())
        tests = np.stack(ref.nms_tests_ref(inter, areas, s.numpy(), *thr))
        for row in range(4):
            sole[row] += int((~tests[row] & np.delete(tests, row, axis=0).all(axis=0)).sum())
    assert (sole >= 1).all(), sole


def test_restatement_fallbacks_and_quirks():
    # no score above the threshold: the score test is switched on for the three best-scored masks
    masks = np.zeros((5, 4, 8), bool)
    for m in range(5):
        masks[m, :, m] = True
    scores = np.asarray([0.01, 0.05, 0.03, 0.02, 0.04], np.float32)
    np.testing.assert_array_equal(ref.mask_nms_ref(masks, scores), [1, 4, 2])
    np.testing.assert_array_equal(ref.mask_nms_ref(masks[:2], scores[:2]), [1, 0])
    # two empty masks: the lower-scored one is dropped (0 / 0 union), the other kept
    masks = np.zeros((3, 4, 8), bool)
    masks[0, :2] = True
    np.testing.assert_array_equal(ref.mask_nms_ref(masks, np.asarray([0.9, 0.5, 0.7], np.float32)), [0, 2])
    # the superdiagonal quirk: big (0.9) over small (0.8), adjacent in the order: the small one fails the upper test AND the lower one
    masks = np.zeros((2, 10, 10), bool)
    masks[0] = True
    masks[1, :2, :5] = True
    s, idx = torch.sort(torch.tensor([0.9, 0.8]), descending=True, stable=True)
    inter, areas = ref.overlaps_ref(masks, idx.numpy())
    k_iou, k_conf, k_u, k_l = ref.nms_tests_ref(inter, areas, s.numpy())
    assert k_iou.all() and k_conf.all() and list(k_u) == [True, False] and list(k_l) == [True, False]


def test_exports_resolve():
    build.build_library()
    L = _lib.load()
    names = ["mi_mask_overlaps", "mi_mask_boxes", "mi_mask_nms_keep", "mi_mask_score_images"]
    assert _lib.DECLARED["mi_mask_sets.h"] == names
    for name in names:
        assert name in _lib.ALL_EXPORTS
        assert ctypes.cast(getattr(L, name), ctypes.c_void_p).value
    for name in ("mask_overlaps", "masks_to_boxes", "mask_nms", "masks_update", "mask_score_images"):
        assert callable(getattr(sam_masks, name))


def test_abi_refuses_bad_arguments_before_any_launch():
    """One refused call per entry point, with its message; the pointers are never read, so no device is needed."""
    build.build_library()
    L = _lib.load()
    assert L.mi_mask_overlaps(0, 4, 4, 8, None, 8, None, None) != 0
    assert _lib.last_error() == "mask sets: need 1 <= M <= 1024 masks and H, W >= 1"
    assert L.mi_mask_overlaps(2, 4096, 4096, 8, None, 8, None, None) != 0
    assert _lib.last_error() == "mask sets: need H * W < 2^24 pixels (every count is then exact in f32)"
    assert L.mi_mask_overlaps(2, 4, 4, 8, None, None, None, None) != 0 and _lib.last_error() == "mask sets: null pointer"
    assert L.mi_mask_boxes(1025, 4, 4, 8, 8, None, None) != 0
    assert _lib.last_error() == "mask sets: need 1 <= M <= 1024 masks and H, W >= 1"
    assert L.mi_mask_boxes(2, 4, 4, 8, None, None, None) != 0 and _lib.last_error() == "mask sets: null pointer"
    assert L.mi_mask_nms_keep(1025, 8, 8, 8, 0.7, 0.1, 0.8, 8, None) != 0
    assert _lib.last_error() == "mask nms: need 1 <= M <= 1024 masks"
    assert L.mi_mask_nms_keep(4, 8, 8, 8, float("nan"), 0.1, 0.8, 8, None) != 0 and _lib.last_error() == "mask nms: a threshold is NaN"
    assert L.mi_mask_nms_keep(4, 8, None, 8, 0.7, 0.1, 0.8, 8, None) != 0 and _lib.last_error() == "mask nms: null pointer"
    assert L.mi_mask_score_images(2, 4, 4, 65, 8, 8, 0, 8, None) != 0
    assert _lib.last_error() == "mask score images: need 1 <= K <= 64 score columns"
    assert L.mi_mask_score_images(2, 4, 4, 3, 8, 8, 3, 8, None) != 0
    assert _lib.last_error() == "mask score images: mode must be MI_MASK_SCORE_SUM, _MEAN or _MAX"
    assert L.mi_mask_score_images(2, 4, 4, 3, 8, 8, 1, None, None) != 0 and _lib.last_error() == "mask score images: null pointer"


def test_python_refusals_before_any_launch():
    b = lambda *shape: torch.zeros(*shape, dtype=torch.bool)
    every = [lambda m: sam_masks.mask_overlaps(m), lambda m: sam_masks.masks_to_boxes(m),
             lambda m: sam_masks.mask_nms(m, torch.zeros(m.shape[0])), lambda m: sam_masks.mask_score_images(torch.zeros(m.shape[0]), m)]
    for call in every:
        with pytest.raises(ValueError, match="1 <= M <= 1024"):
            call(b(0, 4, 4))
        with pytest.raises(ValueError, match="1 <= M <= 1024"):
            call(b(1025, 1, 1))
        with pytest.raises(ValueError, match=r"h \* w < 2\^24"):
            call(b(1, 4096, 4096))
        with pytest.raises(ValueError, match="bool"):
            call(torch.zeros(2, 4, 4))
        with pytest.raises(ValueError, match="bool"):
            call(b(4, 4))
    with pytest.raises(ValueError, match="1 <= M <= 1024"):
        sam_masks.mask_overlaps(PackedSamMasks(torch.zeros(1025, 1, 1, dtype=torch.int64), (1025, 1, 1)))
    with pytest.raises(ValueError, match=r"h \* w < 2\^24"):
        sam_masks.masks_to_boxes(PackedSamMasks(torch.zeros(1, 1, 1, dtype=torch.int64), (1, 4096, 4096)))
    with pytest.raises(ValueError, match="PackedSamMasks"):
        sam_masks.mask_overlaps(PackedSamMasks(torch.zeros(2, 8, 2, dtype=torch.int64), (2, 8, 8)))
    with pytest.raises(ValueError, match="1 <= K <= 64"):
        sam_masks.mask_score_images(torch.zeros(2, 65), b(2, 4, 4))
    with pytest.raises(ValueError, match="1 <= K <= 64"):
        sam_masks.mask_score_images(torch.zeros(2, 0), b(2, 4, 4))
    with pytest.raises(ValueError, match=r"\(M,\) or \(M, K\)"):
        sam_masks.mask_score_images(torch.zeros(2, 3, 1), b(2, 4, 4))
    with pytest.raises(ValueError, match="mode"):
        sam_masks.mask_score_images(torch.zeros(2), b(2, 4, 4), mode="median")
    for wrong in (torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float16), np.zeros(2, np.float32), [0.0, 0.0]):
        with pytest.raises(ValueError, match="float32"):
            sam_masks.mask_score_images(wrong, b(2, 4, 4))
        with pytest.raises(ValueError, match="float32"):
            sam_masks.mask_nms(b(2, 4, 4), wrong)
    with pytest.raises(ValueError, match="NaN"):
        sam_masks.mask_nms(b(2, 4, 4), torch.zeros(2), iou_thr=float("nan"))
    with pytest.raises(ValueError, match="number"):
        sam_masks.mask_nms(b(2, 4, 4), torch.zeros(2), inner_thr="low")
    # masks and scores must share one GPU: scores on the CPU are refused, whatever the masks are on
    with pytest.raises(ValueError, match="scores must be on a GPU"):
        sam_masks.mask_nms(b(2, 4, 4), torch.zeros(2))
    with pytest.raises(ValueError, match="scores must be on a GPU"):
        sam_masks.mask_score_images(torch.zeros(2, 3), b(2, 4, 4))
    # and masks that are neither on the CPU nor on a GPU
    with pytest.raises(ValueError, match="need the CPU or a GPU"):
        sam_masks.masks_to_boxes(torch.zeros(2, 4, 4, dtype=torch.bool, device="meta"))


def test_masks_update_restatement_filters_each_level_in_place_order():
    rng = np.random.default_rng(3)
    def level(n):
        out = []
        for i in range(n):
            seg = np.zeros((6, 16), bool)
            seg[:, 2 * (i % 4): 2 * (i % 4) + 2 + (i // 4)] = True
            out.append({"segmentation": seg, "predicted_iou": float(rng.uniform(0.6, 1)), "stability_score": float(rng.uniform(0.6, 1)), "id": i})
        return out
    a, b = level(8), level(3)
    ka, kb, kc = ref.masks_update_ref(a, b, [], iou_thr=0.8, score_thr=0.5, inner_thr=0.5)
    assert kc == [] and 0 < len(ka) < len(a)
    assert [m["id"] for m in ka] == sorted(m["id"] for m in ka) and all(any(m is x for x in a) for m in ka) and all(any(m is x for x in b) for m in kb)
