"""GPU tests of the SAM-mask set operations (seganygaussians_amd/sam_masks.py, csrc/mask_sets.h) against the
restatement of tests/sam_masks_ref.py and the reference's own mask_nms selections (tests/golden/sam_masks/sam_masks.npz).

Overlaps, areas, boxes, the NMS selection, the covering count and the "max" images are exact.  "sum" and "mean" are sequential
float32 sums in ascending mask order, so against the float64 restatement a pixel covered by n masks may differ by at most
n 2^-24 sum_m |scores[m, k]| bit_m(p) (n - 1 additions, and for "mean" the division: one more rounding, a factor 1 + 2^-24)."""
import functools

import numpy as np
import pytest
import torch

from seganygaussians_amd import lifting, sam_masks
from seganygaussians_amd.contrastive_loss import pack_sam_masks
from tests import helpers as hp
from tests import sam_masks_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24

# (M, h, w): one mask of one pixel; a full last word; a last word of one bit; more than one 64 x 64 pair tile, three words a row and
# more words than one staged chunk; 63 pixels in a partial word; the cap on M (16 x 16 pair tiles, 8 slabs of 128 masks)
SHAPES = [(1, 1, 1), (2, 3, 64), (33, 5, 65), (65, 24, 130), (70, 7, 63), (1024, 2, 70)]
IDS = ["x".join(str(v) for v in s) for s in SHAPES]


@functools.lru_cache(maxsize=None)
def make_masks(M, h, w):
    """Seeded masks: random rectangles and random bits of several densities; then, as far as M allows, a mask of only the last
    valid bit of the last word of the last row, an empty mask and a full one."""
    rng = np.random.default_rng(1000 * M + 10 * h + w)
    masks = np.zeros((M, h, w), bool)
    for m in range(M):
        if m % 3 == 0:
            masks[m] = rng.random((h, w)) < rng.choice([0.05, 0.5, 0.9])
        else:
            y0, x0 = rng.integers(0, h), rng.integers(0, w)
            masks[m, y0: y0 + rng.integers(1, h + 1), x0: x0 + rng.integers(1, w + 1)] = True
    last = np.zeros((h, w), bool)
    last[h - 1, w - 1] = True
    for m, special in zip(range(M - 1, -1, -1), [last, np.zeros((h, w), bool), np.ones((h, w), bool)]):
        masks[m] = special
    masks.setflags(write=False)
    return masks


@functools.lru_cache(maxsize=None)
def packed_masks(M, h, w):
    return pack_sam_masks(torch.from_numpy(make_masks(M, h, w).copy()), device=DEV)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_overlaps_and_boxes_exact(shape):
    M = shape[0]
    masks = make_masks(*shape)
    want_inter, want_areas = ref.overlaps_ref(masks)
    want_boxes = ref.boxes_ref(masks)
    assert M < 3 or (np.isnan(want_boxes[M - 2]).all() and want_areas[M - 1] == 1 and want_areas[M - 3] == shape[1] * shape[2])
    for source in (torch.from_numpy(masks.copy()), packed_masks(*shape)):   # a bool tensor on the CPU, packed masks on the device
        inter, areas = sam_masks.mask_overlaps(source)
        assert inter.dtype == torch.int32 and areas.dtype == torch.int64 and inter.shape == (M, M) and areas.shape == (M,)
        np.testing.assert_array_equal(inter.cpu().numpy(), want_inter)
        np.testing.assert_array_equal(areas.cpu().numpy(), want_areas)
        boxes, box_areas = sam_masks.masks_to_boxes(source, return_areas=True)
        assert boxes.dtype == torch.float32 and boxes.shape == (M, 4)
        np.testing.assert_array_equal(boxes.cpu().numpy(), want_boxes)   # NaN rows compare equal to NaN rows
        np.testing.assert_array_equal(box_areas.cpu().numpy(), want_areas)
        assert torch.equal(sam_masks.masks_to_boxes(source).isnan(), boxes.isnan())
    order = torch.from_numpy(np.random.default_rng(M).permutation(M))
    want_inter, want_areas = ref.overlaps_ref(masks, order.numpy())
    inter, areas = sam_masks.mask_overlaps(packed_masks(*shape), order=order.to(DEV))
    np.testing.assert_array_equal(inter.cpu().numpy(), want_inter)
    np.testing.assert_array_equal(areas.cpu().numpy(), want_areas)
    inter, _ = sam_masks.mask_overlaps(torch.from_numpy(masks.copy()).to(DEV), order=order.to(DEV))
    np.testing.assert_array_equal(inter.cpu().numpy(), want_inter)


def test_overlaps_order_must_be_a_permutation():
    p = packed_masks(33, 5, 65)
    with pytest.raises(ValueError, match="permutation"):
        sam_masks.mask_overlaps(p, order=torch.zeros(33, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="int64"):
        sam_masks.mask_overlaps(p, order=torch.arange(33, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="the order on"):
        sam_masks.mask_overlaps(p, order=torch.arange(33))


def _nms(masks, scores, *thr):
    got = sam_masks.mask_nms(torch.from_numpy(np.ascontiguousarray(masks)), torch.as_tensor(scores, dtype=torch.float32).to(DEV), *thr)
    assert got.dtype == torch.int64 and got.device == DEV
    return got.cpu().numpy()


def test_mask_nms_equals_every_reference_selection():
    cases = ref.load_cases()
    assert len(cases) >= 60
    for c, (masks, scores, thr, selected) in enumerate(cases):
        np.testing.assert_array_equal(_nms(masks, scores, *thr), selected, err_msg=f"case {c}: M={len(scores)} thresholds={thr}")


def _strips(M, h=4, w=8):
    masks = np.zeros((M, h, w), bool)
    for m in range(M):
        masks[m, :, m] = True
    return masks


def test_mask_nms_fallbacks_and_empty_masks():
    # no score above the threshold: the score test is switched on for the three best-scored masks (what sam_utils.py:173-175 means)
    scores = np.asarray([0.01, 0.05, 0.03, 0.02, 0.04], np.float32)
    for M, want in ((5, [1, 4, 2]), (3, [1, 2, 0]), (2, [1, 0])):
        got = _nms(_strips(M), scores[:M])
        np.testing.assert_array_equal(got, ref.mask_nms_ref(_strips(M), scores[:M]))
        np.testing.assert_array_equal(got, want)
    # M = 2 and M = 1 with passing scores
    np.testing.assert_array_equal(_nms(_strips(2), [0.5, 0.9]), [1, 0])
    np.testing.assert_array_equal(_nms(_strips(1), [0.5]), [0])
    np.testing.assert_array_equal(_nms(_strips(1), [0.05]), [0])
    # two empty masks: the lower-scored one is dropped (0 / 0 union), the other kept; an empty mask forms no inner entry
    masks = np.zeros((4, 4, 8), bool)
    masks[0, :2] = True
    masks[3] = True
    scores = np.asarray([0.9, 0.5, 0.7, 0.6], np.float32)
    got = _nms(masks, scores)
    np.testing.assert_array_equal(got, ref.mask_nms_ref(masks, scores))
    np.testing.assert_array_equal(got, [0, 2, 3])
    # ties: a stable sort keeps the earlier mask first
    np.testing.assert_array_equal(_nms(_strips(4), [0.5, 0.9, 0.5, 0.9]), [1, 3, 0, 2])


def test_mask_nms_boundaries_with_representable_thresholds():
    row = lambda *px: np.isin(np.arange(16), px).reshape(1, 16)
    # IoU exactly 0.5 (2 of 4 pixels; I / a = 2/3 forms no inner entry): kept at iou_thr = 0.5, dropped just below
    masks = np.stack([row(0, 1, 2), row(1, 2, 3)])
    scores = [0.9, 0.8]
    np.testing.assert_array_equal(_nms(masks, scores, 0.5), [0, 1])
    np.testing.assert_array_equal(_nms(masks, scores, 0.4375), [0])
    for thr in (0.5, 0.4375):
        np.testing.assert_array_equal(_nms(masks, scores, thr), ref.mask_nms_ref(masks, scores, thr))
    # I / a_i exactly 0.5 (4 of 8) is not < 0.5: no inner entry, the part is kept at inner_thr = 0.5 (t = 0.5); 4 of 9 forms one,
    # v = 1 - 4/9 > 0.5, and the part is dropped; with the part scored higher it is the lower test that drops it
    part = row(0, 1, 2, 3)
    for big, want_part_kept in ((row(*range(8)), True), (row(*range(9)), False)):
        masks = np.stack([big, part])
        for scores, want in (([0.9, 0.8], [0, 1] if want_part_kept else [0]), ([0.8, 0.9], [1, 0] if want_part_kept else [0])):
            got = _nms(masks, scores, 0.7, 0.1, 0.5)
            np.testing.assert_array_equal(got, ref.mask_nms_ref(masks, scores, 0.7, 0.1, 0.5))
            np.testing.assert_array_equal(got, want)
    # I / a_j at 0.85: 17 of 20 pixels is f32(0.85), the constant as the reference's float32 comparison rounds it; 16 of 20 is below
    flat = lambda *ranges: np.isin(np.arange(128), np.concatenate([np.arange(*r) for r in ranges])).reshape(8, 16)
    for inside, want in ((17, [0]), (16, [0, 1])):
        masks = np.stack([flat((0, 64)), flat((0, inside), (64, 64 + 20 - inside))])
        scores = [0.9, 0.8]
        got = _nms(masks, scores, 0.7, 0.1, 0.5)
        np.testing.assert_array_equal(got, ref.mask_nms_ref(masks, scores, 0.7, 0.1, 0.5))
        np.testing.assert_array_equal(got, want)


def test_mask_nms_superdiagonal_pair():
    """The pair (c-1, c) also enters the LOWER inner maximum of column c (torch.tril(..., diagonal=1), sam_utils.py:164).  The same
    entry is in the upper maximum of that column, so a selection alone cannot isolate it; the restatement's four tests show it
    (tests/test_sam_masks_host.py) and the kernel must agree with the restatement with the pair adjacent in the order and apart."""
    big = np.ones((10, 10), bool)
    part = np.zeros((10, 10), bool)
    part[:2, :5] = True
    other = np.zeros((10, 10), bool)
    other[9, 9] = True
    for masks, scores in ((np.stack([big, part]), [0.9, 0.8]), (np.stack([big, other, part]), [0.9, 0.85, 0.8]),
                          (np.stack([other, big, part]), [0.95, 0.9, 0.8])):
        got = _nms(masks, scores)
        np.testing.assert_array_equal(got, ref.mask_nms_ref(masks, scores))
        assert len(masks) - 1 not in got   # the part is rejected (v = 0.9 > 0.8)


def test_masks_update_filters_sam_lists():
    rng = np.random.default_rng(3)
    def level(n):
        out = []
        for i in range(n):
            seg = np.zeros((6, 16), bool)
            seg[:, 2 * (i % 4): 2 * (i % 4) + 2 + (i // 4)] = True
            out.append({"segmentation": seg, "predicted_iou": float(rng.uniform(0.6, 1)), "stability_score": float(rng.uniform(0.6, 1)), "id": i})
        return out
    a, b = level(8), level(3)
    kwargs = dict(iou_thr=0.8, score_thr=0.5, inner_thr=0.5)
    got = sam_masks.masks_update(a, b, [], **kwargs)
    want = ref.masks_update_ref(a, b, [], **kwargs)
    assert [[m["id"] for m in lvl] for lvl in got] == [[m["id"] for m in lvl] for lvl in want]
    assert 0 < len(got[0]) < len(a) and got[2] == []


@functools.lru_cache(maxsize=None)
def score_case(shape, K):
    M = shape[0]
    scores = np.random.default_rng(K + M).standard_normal((M, K)).astype(np.float32)
    images, count, mag = ref.score_images_ref(scores, make_masks(*shape))
    return scores, images, count, mag


@pytest.mark.parametrize("K", [1, 3, 64])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_score_images_within_the_sequential_f32_bound(shape, K):
    M, h, w = shape
    scores, images, count, mag = score_case(shape, K)
    s = torch.from_numpy(scores).to(DEV)
    packed = packed_masks(*shape)
    n = count[None].astype(np.float64)
    for mode in ("sum", "mean", "max"):
        got_t = sam_masks.mask_score_images(s, packed, mode=mode)
        assert got_t.shape == (K, h, w) and got_t.dtype == torch.float32 and got_t.is_contiguous()
        assert torch.equal(got_t, sam_masks.mask_score_images(s, packed, mode=mode)), f"{mode}: two runs differ"
        got = got_t.cpu().numpy().astype(np.float64)
        assert (got[:, count == 0] == 0).all(), f"{mode}: an uncovered pixel is not exactly 0"
        if mode == "max":
            np.testing.assert_array_equal(got, images["max"])
            continue
        bound = n * U * mag if mode == "sum" else (n * U * mag / np.maximum(n, 1)) * (1 + U)
        err = np.abs(got - images[mode])
        worst = float((err / np.maximum(bound, 1e-300)).max()) if bound.max() > 0 else 0.0
        print(f"{mode} {shape} K={K}: max err {err.max():.3e}, worst err / bound {worst:.3f}")
        assert (err <= bound).all(), f"{mode}: max err / bound {worst}"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_score_images_count_inputs_and_out(shape):
    M, h, w = shape
    masks = make_masks(*shape)
    count = masks.sum(axis=0)
    ones = torch.ones(M, device=DEV)
    # the covering count, exactly: the "sum" of ones; from a bool tensor on the CPU, 1-D scores
    got = sam_masks.mask_score_images(ones, torch.from_numpy(masks.copy()), mode="sum")
    assert got.shape == (1, h, w)
    np.testing.assert_array_equal(got[0].cpu().numpy(), count.astype(np.float32))
    np.testing.assert_array_equal(sam_masks.mask_score_images(ones, packed_masks(*shape)).cpu().numpy()[0], (count > 0).astype(np.float32))
    # out=, and a column view of a wider score matrix
    scores, images, _, _ = score_case(shape, 3)
    out = torch.full((1, h, w), 7.0, device=DEV)
    col = torch.from_numpy(scores).to(DEV)[:, 1]
    assert sam_masks.mask_score_images(col, packed_masks(*shape), mode="max", out=out) is out
    np.testing.assert_array_equal(out.cpu().numpy()[0].astype(np.float64), images["max"][1])
    with pytest.raises(ValueError, match="out must be"):
        sam_masks.mask_score_images(col, packed_masks(*shape), out=torch.empty((2, h, w), device=DEV))
    with pytest.raises(ValueError, match="score rows"):
        sam_masks.mask_score_images(torch.ones(M + 1, device=DEV), packed_masks(*shape))


def test_score_images_feed_lift_scores():
    """masks -> score images -> 3-D votes: the kernel's image is the torch-built one bit for bit when every sum is exact (scores that
    are multiples of 1/8), and lift_scores takes it as it is.  The two lifts then differ by the order of the float atomics alone:
    at most 2 n 2^-24 of the lift of |image|, n = h w terms at most per vote."""
    M, h, w = 65, 24, 130
    masks = make_masks(M, h, w)
    scores = torch.from_numpy((np.random.default_rng(5).integers(-16, 17, (M, 3)) / 8).astype(np.float32)).to(DEV)
    mf = torch.from_numpy(masks.copy()).to(DEV).float()
    want = torch.einsum("kp,khw->kphw", scores, mf).sum(dim=0) / (mf.sum(dim=0, keepdim=True) + 1e-9)   # clip_utils/__init__.py:282
    image = sam_masks.mask_score_images(scores, packed_masks(M, h, w), mode="mean")
    assert torch.equal(image, want)
    g = hp.GpuRun(hp.make_inputs(600, w, h, 3, seed=2))
    geometry = dict(scales=g.scales, rotations=g.rots, viewmatrix=g.view, projmatrix=g.proj, tanfovx=g.inp.tanfovx, tanfovy=g.inp.tanfovy)
    votes = lifting.lift_scores(image, g.means3D, g.opac, **geometry)
    votes_want = lifting.lift_scores(want, g.means3D, g.opac, **geometry)
    votes_abs = lifting.lift_scores(want.abs(), g.means3D, g.opac, **geometry)
    assert votes.shape == (600, 3) and float(votes.abs().max()) > 0
    assert bool(((votes - votes_want).abs() <= 2 * h * w * U * 1.01 * votes_abs).all())
