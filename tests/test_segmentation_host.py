"""CPU checks of the segmentation queries: the float64 restatement (tests/segmentation_ref.py) against the reference's own float32
lines, the share of decisions the band excuses for exactly the seeds and shapes the GPU test uses, the argument checks of
seganygaussians_amd/segmentation.py before any launch, and the exports.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

from seganygaussians_amd import _lib, build
from seganygaussians_amd import segmentation as seg
from tests import segmentation_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 0.01


def test_gui_frame_lines_match_restatement():
    feats, queries, gates = ref.make_case("image", (9, 21), 32, 3, seed=21)
    feats[:, 2, 5] = 0.0                                   # a background pixel of a zero-background render
    thres = 0.55
    binary, score_map, pca = ref.literal32_gui_frame(feats, gates, queries.t().contiguous(), thres, proj_mat=queries.t().contiguous())
    mask, score, t = ref.select64(feats, queries, thres, gates, pre="eps", half_shift=True)
    band = ((t - thres).abs() <= 2 * ref.value_bound(32, queries)[:, None, None]).any(0)
    assert torch.equal(binary[~band], mask[~band])
    assert (score_map.double() - score)[~band].abs().max() <= ref.value_bound(32, queries).max()
    assert not mask[2, 5] and score[2, 5] == 0.0 and (t[:, 2, 5] == 0.5).all()
    want_pca = ref.scores64(feats, queries, None, pre="eps", post=False)
    assert (pca.permute(2, 0, 1).double() - want_pca).abs().max() <= ref.value_bound(32, queries).max()


def test_segment3d_and_similarity_map_lines_match_restatement():
    feats, queries, gates = ref.make_case("points", (700,), 32, 2, seed=22)
    thres = 0.6
    binary, score_pts = ref.literal32_segment3d(feats, gates, queries.t().contiguous(), thres)
    mask, _, t = ref.select64(feats, queries, thres, gates, pre="none", half_shift=True)
    b = ref.value_bound(32, queries)
    band = ((t - thres).abs() <= 2 * b[:, None]).any(0)
    assert torch.equal(binary[~band], mask[~band])
    assert ((score_pts.t().double() - t).abs() <= b[:, None]).all()
    sim = ref.literal32_get_similarity_map(feats, gates, queries[0])
    assert ((sim.double() - ref.scores64(feats, queries[:1], gates)[0]).abs() <= b[0]).all()
    img, q2, g2 = ref.make_case("image", (5, 13), 16, 1, seed=23)
    sim2 = ref.literal32_point_prompt_2d(img, g2, q2[0])
    assert ((sim2.double() - ref.scores64(img, q2, g2)[0]).abs() <= ref.value_bound(16, q2)[0]).all()


def test_cluster_lines_match_restatement():
    feats, centers, gates = ref.make_case("points", (900,), 32, 20, seed=24)
    centers = ref.unit_centers(centers)
    seg_score, lit_labels = ref.literal32_cluster_in_3d(feats, gates, centers)
    labels, best, gap, _ = ref.assign64(feats, centers, gates, pre="l2")
    b = ref.value_bound(32, centers).max()
    differ = lit_labels != labels
    assert not differ[gap > 2 * b].any()
    assert ((seg_score.max(dim=-1).values.double() - best).abs() <= b).all()
    img, c2, g2 = ref.make_case("image", (6, 11), 16, 7, seed=25)
    res, idx = ref.literal32_cluster_2d(img, g2, c2)
    l2, best2, gap2, _ = ref.assign64(img, c2, g2, pre="none")
    b2 = ref.value_bound(16, c2).max()
    assert not (idx != l2)[gap2 > 2 * b2].any()
    assert ((res.max(dim=-1).values.double() - best2).abs() <= b2).all()


def test_restatement_exact_cases():
    C = 8
    feats = torch.zeros(4, C)
    centers = torch.eye(C)[:3].clone()
    feats[1] = 3.0 * centers[2]
    feats[2] = centers[1]
    labels, best, gap, _ = ref.assign64(feats, centers, None, pre="l2")
    assert labels.tolist() == [0, 2, 1, 0] and best.tolist() == [0.0, 1.0, 1.0, 0.0]
    dup = torch.stack([centers[1], centers[1], centers[0]])
    assert ref.assign64(feats, dup, None)[0].tolist() == [0, 0, 0, 0]
    mask, score, t = ref.select64(feats, centers, 0.5, None, half_shift=True)
    assert not mask[0] and score[0] == 0.0 and (t[:, 0] == 0.5).all()


@pytest.mark.parametrize("case", ref.CAP_CASES, ids=lambda c: f"{c[0]}-{c[1]}-C{c[2]}-Q{c[3]}")
def test_select_band_share_of_the_gpu_cases(case):
    """For the seeds and shapes of the GPU test: the reference's float32 lines disagree with the yardstick only inside the band, and
    the band holds less than 1 % of the rows."""
    layout, shape, C, Q, seed = case
    feats, queries, gates = ref.make_case(layout, shape, C, Q, seed)
    b = ref.value_bound(C, queries)
    for half_shift, thres in ((True, 0.6), (False, 0.2)):
        mask, score, t = ref.select64(feats, queries, thres, gates, pre="none", half_shift=half_shift)
        band = ((t - thres).abs() <= 2 * b.reshape((-1,) + (1,) * (t.dim() - 1))).any(0)
        assert band.float().mean() <= CAP
        rows, _ = ref.rows_of(feats)
        lit = ref.literal32_get_similarity_map(rows, gates, queries[0]) if Q == 1 else None
        lit_t = ref.literal32_segment3d(rows, gates, queries.t().contiguous(), thres)[1] if half_shift else \
            torch.nn.functional.normalize(rows * gates, dim=-1) @ queries.t()
        lit_mask = (lit_t > thres).any(-1).reshape(mask.shape)
        assert not (lit_mask != mask)[~band].any()
        if lit is not None and not half_shift:
            assert ((lit.double().reshape(mask.shape) - t[0]).abs() <= b[0]).all()


@pytest.mark.parametrize("case", ref.ASSIGN_CASES, ids=lambda c: f"{c[0]}-{c[1]}-C{c[2]}-K{c[3]}")
def test_assign_band_share_of_the_gpu_cases(case):
    layout, shape, C, K, seed = case
    feats, centers, gates = ref.make_case(layout, shape, C, K, seed)
    labels, best, gap, second = ref.assign64(feats, centers, gates, pre="l2")
    b = ref.value_bound(C, centers)
    band = gap <= 2 * torch.maximum(b[labels], b[second])
    assert band.float().mean() <= CAP
    rows, _ = ref.rows_of(feats)
    lit_labels = ref.literal32_cluster_in_3d(rows, gates, centers)[1].reshape(labels.shape)
    assert not (lit_labels != labels)[~band].any()


def test_bad_inputs_refused_before_any_launch():
    f = torch.zeros(10, 8)
    q = torch.zeros(2, 8)
    for fn in (lambda *a, **k: seg.similarity_scores(*a, **k), lambda f_, q_, **k: seg.select_by_similarity(f_, q_, 0.5, **k),
               lambda *a, **k: seg.assign_clusters(*a, **k)):
        with pytest.raises(ValueError, match="GPU"):
            fn(f, q)
        with pytest.raises(ValueError, match="float32"):
            fn(f.double(), q)
        with pytest.raises(ValueError, match="float32"):
            fn(f, q.half())
        with pytest.raises(ValueError, match="float32"):
            fn(f.numpy(), q)
        with pytest.raises(ValueError, match=r"\(C, H, W\) or \(P, C\)"):
            fn(torch.zeros(8), q)
        with pytest.raises(ValueError, match=r"\(C, H, W\) or \(P, C\)"):
            fn(torch.zeros(1, 2, 3, 8), q)
        with pytest.raises(ValueError, match="must be"):
            fn(f, torch.zeros(2, 7))
        with pytest.raises(ValueError, match="must be"):
            fn(torch.zeros(8, 4, 4), torch.zeros(2, 4))       # image: C is the first axis
        with pytest.raises(ValueError, match="256"):
            fn(torch.zeros(3, 257), torch.zeros(1, 257))
        with pytest.raises(ValueError, match="rows"):
            fn(torch.zeros(0, 8), q)
        with pytest.raises(ValueError, match="gates"):
            fn(f, q, gates=torch.zeros(7))
        with pytest.raises(ValueError, match="gates"):
            fn(f, q, gates=torch.zeros(8, dtype=torch.float64))
        with pytest.raises(ValueError, match="pre"):
            fn(f, q, pre="L2")
        with pytest.raises(ValueError, match="requires grad"):
            fn(f.clone().requires_grad_(), q)
        with torch.no_grad(), pytest.raises(ValueError, match="GPU"):   # allowed with grad mode off; then the device check
            fn(f.clone().requires_grad_(), q)
    with pytest.raises(ValueError, match="16"):
        seg.similarity_scores(f, torch.zeros(17, 8))
    with pytest.raises(ValueError, match="16"):
        seg.select_by_similarity(f, torch.zeros(17, 8), 0.5)
    with pytest.raises(ValueError, match="4096"):
        seg.assign_clusters(f, torch.zeros(4097, 8))
    with pytest.raises(ValueError, match="queries"):
        seg.similarity_scores(f, torch.zeros(0, 8))


def test_abi_exported_and_checks_arguments():
    build.build_library()
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "mi_segment.h")).read()
    declared = set(re.findall(r"\b(mi_segment_[a-z_0-9]+)\s*\(", hdr))
    assert declared == {"mi_segment_scores", "mi_segment_select", "mi_segment_assign", "mi_segment_assign_block"} <= set(_lib.ALL_EXPORTS)
    assert _lib.DECLARED["mi_segment.h"] == ["mi_segment_scores", "mi_segment_select", "mi_segment_assign", "mi_segment_assign_block"]
    assert (seg.MAX_CHANNELS, seg.MAX_QUERIES, seg.MAX_CENTERS) == (_lib.MI_SEGMENT_MAX_CHANNELS, _lib.MI_SEGMENT_MAX_QUERIES, _lib.MI_SEGMENT_MAX_CENTERS)
    assert seg.PRE_MODES == _lib.MI_SEGMENT_PRE == {"none": _lib.MI_SEGMENT_PRE_NONE, "l2": _lib.MI_SEGMENT_PRE_L2, "eps": _lib.MI_SEGMENT_PRE_EPS}
    for name in declared:
        assert ctypes.cast(getattr(L, name), ctypes.c_void_p).value
    assert os.path.join(ROOT, "include", "mi_segment.h") in build.HEADERS and "segment.h" in build.SOURCES
    # centres per LDS block: a multiple of 32 that fits 16000 floats at an odd row stride
    for C, steps in ((1, 16), (32, 16), (33, 32), (64, 32), (100, 64), (256, 128)):
        kb = L.mi_segment_assign_block(C)
        assert kb % 32 == 0 and 32 <= kb <= 512 and kb * (2 * steps + 1) <= 16000 < (kb + 32) * (2 * steps + 1)
    assert L.mi_segment_assign_block(0) == 0 and L.mi_segment_assign_block(257) == 0
    # argument checks run before any launch: no device needed
    assert L.mi_segment_scores(2, 4, 4, 1, 8, 8, None, 0, 1, 8, None) != 0 and "layout" in _lib.last_error()
    assert L.mi_segment_scores(0, 0, 4, 1, 8, 8, None, 0, 1, 8, None) != 0 and "N >= 1" in _lib.last_error()
    assert L.mi_segment_scores(0, 4, 257, 1, 8, 8, None, 0, 1, 8, None) != 0 and "256" in _lib.last_error()
    assert L.mi_segment_scores(0, 4, 4, 17, 8, 8, None, 0, 1, 8, None) != 0 and "16" in _lib.last_error()
    assert L.mi_segment_scores(0, 4, 4, 1, 8, 8, None, 3, 1, 8, None) != 0 and "pre" in _lib.last_error()
    assert L.mi_segment_scores(0, 4, 4, 1, None, 8, None, 0, 1, 8, None) != 0 and "null" in _lib.last_error()
    assert L.mi_segment_scores(0, 4, 4, 1, 8, 8, None, 0, 1, None, None) != 0 and "null" in _lib.last_error()
    assert L.mi_segment_select(1, 4, 4, 0, 8, 8, None, 0, 1, 0.5, 8, 8, None) != 0 and "16" in _lib.last_error()
    assert L.mi_segment_select(1, 4, 4, 1, 8, 8, None, 0, 1, float("nan"), 8, 8, None) != 0 and "NaN" in _lib.last_error()
    assert L.mi_segment_select(1, 4, 4, 1, 8, 8, None, 0, 1, 0.5, None, 8, None) != 0 and "null" in _lib.last_error()
    assert L.mi_segment_assign(1, 4, 4, 4097, 8, 8, None, 1, 8, 8, None) != 0 and "4096" in _lib.last_error()
    assert L.mi_segment_assign(1, 4, 4, 20, 8, 8, None, 1, None, 8, None) != 0 and "null" in _lib.last_error()


def test_module_exports():
    assert callable(seg.similarity_scores) and callable(seg.select_by_similarity) and callable(seg.assign_clusters)
    assert seg.MAX_CHANNELS == 256 and seg.MAX_QUERIES == 16 and seg.MAX_CENTERS == 4096
    assert seg.PRE_MODES == _lib.MI_SEGMENT_PRE == {"none": 0, "l2": 1, "eps": 2}
