"""CPU-side checks of the vote graph (seganygaussians_amd/vote_graph.py): every refusal that needs no device,
the plain-torch cluster selection against hand-made labels, the C-ABI's own refusals, and the restatement against itself (the
factorised forms the kernels evaluate equal the literal ones in float64).  No GPU."""
import pytest
import torch

from seganygaussians_amd import _lib, build
from seganygaussians_amd import vote_graph as vg
from seganygaussians_amd.mask_scales import erode_sam_masks
from tests import vote_graph_ref as R


class OnGpu(torch.Tensor):
    """A CPU tensor that says it is on a GPU, for the checks that come after the device check; nothing may read its memory."""
    is_cuda = True

    @staticmethod
    def of(t):
        return t.as_subclass(OnGpu)


F = lambda *shape: torch.zeros(*shape, dtype=torch.float32)


# ---- sam_mask_features ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rendered,masks,gates,kw,msg", [
    (F(4, 8, 8).double(), torch.zeros(2, 8, 8, dtype=torch.bool), F(2, 4), {}, "rendered must be a float32"),
    (F(8, 8), torch.zeros(2, 8, 8, dtype=torch.bool), F(2, 4), {}, r"rendered must be \(C, H, W\)"),
    (F(0, 8, 8), torch.zeros(2, 8, 8, dtype=torch.bool), F(2, 0), {}, "1 <= C <= 256"),
    (F(257, 8, 8), torch.zeros(2, 8, 8, dtype=torch.bool), F(2, 257), {}, "1 <= C <= 256"),
    (F(4, 8, 8), torch.zeros(2, 8, 8), F(2, 4), {}, "masks must be a bool"),
    (F(4, 8, 8), torch.zeros(8, 8, dtype=torch.bool), F(2, 4), {}, "masks must be a bool"),
    (F(4, 8, 8), torch.zeros(0, 8, 8, dtype=torch.bool), F(0, 4), {}, "1 <= M <= 1024"),
    (F(4, 8, 8), torch.zeros(1025, 2, 2, dtype=torch.bool), F(1025, 4), {}, "1 <= M <= 1024"),
    (F(4, 8, 8), torch.zeros(2, 8, 8, dtype=torch.bool), F(3, 4), {}, r"gates must be \(2, 4\)"),
    (F(4, 8, 8), torch.zeros(2, 8, 8, dtype=torch.bool), F(2, 5), {}, r"gates must be \(2, 4\)"),
    (F(4, 8, 8), torch.zeros(2, 8, 8, dtype=torch.bool), F(2, 4).half(), {}, "gates must be a float32"),
    (F(4, 8, 8), torch.zeros(2, 8, 8, dtype=torch.bool), F(2, 4), dict(size=(0, 2)), "size must be positive"),
    (F(4, 3, 8), torch.zeros(2, 8, 8, dtype=torch.bool), F(2, 4), {}, "size must be positive"),   # H // 4 = 0
    (F(4, 8, 8), torch.zeros(2, 8, 8, dtype=torch.bool), F(2, 4), dict(size=5), "size must be"),
    (F(4, 8, 8), torch.zeros(2, 8, 8, dtype=torch.bool), F(2, 4), dict(min_sum=float("nan")), "min_sum is NaN"),
    (F(4, 8, 8), torch.zeros(2, 8, 8, dtype=torch.bool), F(2, 4), {}, "rendered must be on a GPU"),
    (OnGpu.of(F(4, 8, 8)), torch.zeros(2, 8, 8, dtype=torch.bool), F(2, 4), {}, "gates must be on a GPU"),
])
def test_sam_mask_features_refusals(rendered, masks, gates, kw, msg):
    with pytest.raises(ValueError, match=msg):
        vg.sam_mask_features(rendered, masks, gates, **kw)


def test_inputs_requiring_grad_are_refused_unless_no_grad():
    r, m, g = F(4, 8, 8), torch.zeros(2, 8, 8, dtype=torch.bool), F(2, 4).requires_grad_()
    with pytest.raises(ValueError, match="gates requires grad"):
        vg.sam_mask_features(r, m, g)
    with torch.no_grad(), pytest.raises(ValueError, match="rendered must be on a GPU"):   # past the grad check
        vg.sam_mask_features(r, m, g)
    with pytest.raises(ValueError, match="anchor_features requires grad"):
        vg.anchor_bits(F(2, 4), F(2, 4), F(5, 4).requires_grad_())
    with torch.no_grad(), pytest.raises(ValueError, match="mask_features must be on a GPU"):
        vg.anchor_bits(F(2, 4), F(2, 4), F(5, 4).requires_grad_())
    with pytest.raises(ValueError, match="embeds requires grad"):
        vg.clip_relevancy(F(3, 8).requires_grad_(), F(1, 8), F(1, 8))
    with pytest.raises(ValueError, match="embeds must be on a GPU"):
        vg.clip_relevancy(F(3, 8).requires_grad_().detach(), F(1, 8), F(1, 8))


def test_erode_min_sum_is_checked():
    with pytest.raises(ValueError, match="min_sum must be a number"):
        erode_sam_masks(torch.zeros(1, 4, 4, dtype=torch.bool), (4, 4), min_sum="two")
    with pytest.raises(ValueError, match="min_sum is NaN"):
        erode_sam_masks(torch.zeros(1, 4, 4, dtype=torch.bool), (4, 4), min_sum=float("nan"))


# ---- anchor_bits ---------------------------------------------------------------------------------------------------------------------
G = lambda *shape: OnGpu.of(F(*shape))


@pytest.mark.parametrize("args,kw,msg", [
    ((F(2, 4).double(), F(2, 4), F(5, 4)), {}, "mask_features must be a float32"),
    ((F(2, 4, 1), F(2, 4), F(5, 4)), {}, "mask_features must be"),
    ((F(2, 0), F(2, 0), F(5, 0)), {}, "1 <= C <= 256"),
    ((F(2, 257), F(2, 257), F(5, 257)), {}, "1 <= C <= 256"),
    ((F(0, 4), F(0, 4), F(5, 4)), {}, "1 <= M <="),
    ((F(2, 4), F(3, 4), F(5, 4)), {}, r"gates must be \(2, 4\)"),
    ((F(2, 4), F(2, 4), F(5, 3)), {}, r"anchor_features must be \(rows, 4\)"),
    ((F(2, 4), F(2, 4), F(5, 4).to(torch.int32)), {}, "anchor_features must be a float32"),
    ((F(2, 4), F(2, 4), F(0, 4)), {}, "1 <= A <= 32768"),
    ((F(2, 4), F(2, 4), F(32769, 4)), {}, "1 <= A <= 32768"),
    ((F(2, 4), F(2, 4), F(5, 4)), dict(threshold=float("nan")), "threshold is NaN"),
    ((F(2, 4), F(2, 4), F(5, 4)), dict(threshold="x"), "threshold must be a number"),
    ((F(2, 4), F(2, 4), F(5, 4)), dict(row_offset=1), "row_offset without out"),
    ((F(2, 4), F(2, 4), F(40, 4)), dict(out=torch.zeros(4, 1, dtype=torch.int32)), r"out must be int32 \(M_total, 2\)"),
    ((F(2, 4), F(2, 4), F(40, 4)), dict(out=torch.zeros(4, 2, dtype=torch.int64)), r"out must be int32 \(M_total, 2\)"),
    ((F(2, 4), F(2, 4), F(40, 4)), dict(out=torch.zeros(2, dtype=torch.int32)), r"out must be int32 \(M_total, 2\)"),
    ((F(2, 4), F(2, 4), F(40, 4)), dict(out=torch.zeros(4, 4, dtype=torch.int32)[:, :2]), "out must be contiguous"),
    ((F(2, 4), F(2, 4), F(40, 4)), dict(out=torch.zeros(4, 2, dtype=torch.int32), row_offset=3), "do not lie in out's 4 rows"),
    ((F(2, 4), F(2, 4), F(40, 4)), dict(out=torch.zeros(4, 2, dtype=torch.int32), row_offset=-1), "do not lie in out's 4 rows"),
    ((F(2, 4), F(2, 4), F(40, 4)), dict(out=torch.zeros(1, 2, dtype=torch.int32)), "do not lie in out's 1 rows"),
    ((F(2, 4), F(2, 4), F(40, 4)), dict(out=torch.zeros(4, 2, dtype=torch.int32), row_offset=1.0), "row_offset must be an integer"),
    ((F(2, 4), F(2, 4), F(5, 4)), {}, "mask_features must be on a GPU"),
    ((G(2, 4), G(2, 4), F(5, 4)), {}, "anchor_features must be on a GPU"),
    ((G(2, 4), G(2, 4), G(40, 4)), dict(out=torch.zeros(4, 2, dtype=torch.int32)), "out must be on a GPU"),
])
def test_anchor_bits_refusals(args, kw, msg):
    with pytest.raises(ValueError, match=msg):
        vg.anchor_bits(*args, **kw)


# ---- clip_relevancy ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,msg", [
    ((F(3, 8).double(), F(1, 8), F(1, 8)), "embeds must be a float32 or float16"),
    ((F(3, 8, 1), F(1, 8), F(1, 8)), r"embeds must be \(N, D\)"),
    ((F(3, 0), F(1, 0), F(1, 0)), "1 <= D <= 1024"),
    ((F(3, 1025), F(1, 1025), F(1, 1025)), "1 <= D <= 1024"),
    ((F(0, 8), F(1, 8), F(1, 8)), "1 <= N"),
    ((F(3, 8), F(1, 8).half(), F(1, 8)), "pos_embeds must be a float32"),
    ((F(3, 8), F(1, 7), F(1, 8)), r"pos_embeds must be \(rows, 8\)"),
    ((F(3, 8), F(1, 8), F(8)), r"neg_embeds must be \(rows, 8\)"),
    ((F(3, 8), F(17, 8), F(1, 8)), "1 <= P, Q <= 16"),
    ((F(3, 8), F(1, 8), F(17, 8)), "1 <= P, Q <= 16"),
    ((F(3, 8), F(0, 8), F(1, 8)), "1 <= P, Q <= 16"),
    ((F(3, 8), F(1, 8), F(1, 8)), "embeds must be on a GPU"),
    ((F(3, 8).half(), F(1, 8), F(1, 8)), "embeds must be on a GPU"),
    ((G(3, 8), F(1, 8), G(1, 8)), "pos_embeds must be on a GPU"),
])
def test_clip_relevancy_refusals(args, msg):
    with pytest.raises(ValueError, match=msg):
        vg.clip_relevancy(*args)


# ---- the C-ABI's own refusals (no launch: the pointers are never read) ---------------------------------------------------------------
def test_c_abi_refuses_before_any_launch():
    build.build_library()
    L = _lib.load()
    names = ["mi_vote_mask_features_workspace_bytes", "mi_vote_mask_features", "mi_vote_anchor_bits", "mi_vote_relevancy"]
    assert _lib.DECLARED["mi_vote_graph.h"] == names
    for name in names + ["mi_mask_erode_min_sum"]:
        assert name in _lib.ALL_EXPORTS and hasattr(L, name), name
    assert (vg.MAX_ANCHORS, vg.MAX_EMBED_DIM, vg.MAX_PROMPTS) == (32768, 1024, 16) == tuple(_lib.CONSTANTS["MI_VOTE_MAX_" + n] for n in ("ANCHORS", "EMBED_DIM", "PROMPTS"))
    assert L.mi_vote_mask_features_workspace_bytes(0, 4, 8, 8) == 0 and L.mi_vote_mask_features_workspace_bytes(2, 257, 8, 8) == 0
    T = 2 * 2   # ceil(17 / 16) * ceil(65 / 64) tiles
    assert L.mi_vote_mask_features_workspace_bytes(3, 4, 17, 65) >= 4 * 4 * 17 * 65 + 8 * 3 * T * (4 + 1)
    assert L.mi_vote_mask_features(2, 257, 8, 8, 4096, 2, 2, 4096, 4096, 4096, 1 << 20, 4096, None, None) != 0
    assert "1 <= C <= 256" in _lib.last_error()
    assert L.mi_vote_mask_features(2, 4, 8, 8, None, 2, 2, 4096, 4096, 4096, 1 << 20, 4096, None, None) != 0 and "null" in _lib.last_error()
    assert L.mi_vote_mask_features(2, 4, 8, 8, 4096, 2, 2, 4096, 4096, 4096, 8, 4096, None, None) != 0 and "workspace" in _lib.last_error()
    assert L.mi_vote_anchor_bits(2, 32769, 4, 4096, 4096, 4096, 0.5, 4096, None, None) != 0 and "32768" in _lib.last_error()
    assert L.mi_vote_anchor_bits(2, 8, 0, 4096, 4096, 4096, 0.5, 4096, None, None) != 0 and "1 <= C <= 256" in _lib.last_error()
    assert L.mi_vote_anchor_bits(2, 8, 4, 4096, 4096, 4096, float("nan"), 4096, None, None) != 0 and "NaN" in _lib.last_error()
    assert L.mi_vote_anchor_bits(2, 8, 4, 4096, None, 4096, 0.5, 4096, None, None) != 0 and "null" in _lib.last_error()
    assert L.mi_vote_relevancy(3, 1025, 1, 1, 4096, 0, 4096, 4096, 1, 4096, None) != 0 and "D <= 1024" in _lib.last_error()
    assert L.mi_vote_relevancy(3, 8, 17, 1, 4096, 0, 4096, 4096, 1, 4096, None) != 0 and "P, Q <= 16" in _lib.last_error()
    assert L.mi_vote_relevancy(3, 8, 1, 1, 4096, 0, 4096, None, 1, 4096, None) != 0 and "null" in _lib.last_error()
    assert L.mi_mask_erode_min_sum(2, 4, 4, 4096, 4, 4, float("nan"), 8192, None) != 0 and "min_sum is NaN" in _lib.last_error()
    assert L.mi_mask_erode_min_sum(0, 4, 4, 4096, 4, 4, 2.0, 8192, None) != 0 and "1024" in _lib.last_error()


# ---- cluster_scores / cluster_queries ----------------------------------------------------------------------------------------------
def hand_made():
    labels = torch.tensor([0, 1, -1, 1, 0, 2, -1, 2, 2])
    scores = torch.tensor([0.2, 0.9, 0.1, 0.5, 0.4, 0.6, 0.3, 0.6, 0.3])
    feats = torch.arange(9 * 3, dtype=torch.float32).reshape(9, 3) + 1
    scales = torch.arange(9, dtype=torch.float32) / 10
    return scores, labels, feats, scales


def test_cluster_scores_noise_first():
    scores, labels, _, _ = hand_made()
    got = vg.cluster_scores(scores, labels)
    assert torch.allclose(got, torch.tensor([0.2, 0.3, 0.7, 0.5]))
    assert torch.allclose(got, R.cluster_scores(scores, labels))
    no_noise = vg.cluster_scores(scores[:2], labels[:2])
    assert no_noise.shape == (3,) and torch.isnan(no_noise[0]) and torch.equal(no_noise[1:], scores[:2])
    all_noise = vg.cluster_scores(scores, torch.full((9,), -1))
    assert all_noise.shape == (1,) and torch.allclose(all_noise, scores.mean())
    with pytest.raises(ValueError, match="labels must be int64"):
        vg.cluster_scores(scores, labels.int())
    with pytest.raises(ValueError, match="labels must be int64"):
        vg.cluster_scores(scores, labels[:3])
    with pytest.raises(ValueError, match="scores must be a floating"):
        vg.cluster_scores(labels, labels)
    with pytest.raises(ValueError, match=">= -1"):
        vg.cluster_scores(scores, labels - 1)


def test_cluster_queries_selection():
    scores, labels, feats, scales = hand_made()
    q, s, ids, means = vg.cluster_queries(scores, labels, feats, scales)   # clusters 1 (0.7) and 2 (0.5) exceed 0.45
    assert ids.tolist() == [1, 2] and torch.allclose(means, torch.tensor([0.7, 0.5]))
    # cluster 1: row 1 (0.9); cluster 2: rows 5 and 7 tie at 0.6, the first wins
    assert torch.allclose(q, torch.nn.functional.normalize(feats[[1, 5]], dim=-1)) and torch.allclose(s, scales[[1, 5]])
    want = R.cluster_queries(scores, labels, feats, scales)
    for a, b in zip((q, s, ids, means), want):
        assert torch.allclose(a.double(), b.double())
    # none above min_score: the single best
    q, s, ids, means = vg.cluster_queries(scores, labels, feats, scales.reshape(9, 1), min_score=0.95)
    assert ids.tolist() == [1] and torch.allclose(s, scales[[1]]) and q.shape == (1, 3)
    # the noise rows are a group of their own, as in the notebook
    q, s, ids, means = vg.cluster_queries(scores, labels, feats, scales, min_score=0.15)
    assert ids.tolist() == [-1, 0, 1, 2] and torch.allclose(s, scales[[6, 4, 1, 5]])
    # all noise
    q, s, ids, means = vg.cluster_queries(scores, torch.full((9,), -1), feats, scales)
    assert ids.tolist() == [-1] and torch.allclose(s, scales[[1]]) and torch.allclose(means, scores.mean())
    # no noise and nothing above min_score: the absent noise group (NaN mean) is never chosen
    q, s, ids, means = vg.cluster_queries(scores[:2], labels[:2], feats[:2], scales[:2], min_score=2.0)
    assert ids.tolist() == [1]
    with pytest.raises(ValueError, match="mask_features must be a floating"):
        vg.cluster_queries(scores, labels, feats[:4], scales)
    with pytest.raises(ValueError, match="mask_scales must hold 9 values"):
        vg.cluster_queries(scores, labels, feats, scales[:4])


# ---- the restatement against itself ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W,size,M,mask_hw", [(7, 37, 53, (9, 13), 5, None), (64, 12, 130, (3, 33), 17, (9, 50)), (5, 16, 70, (16, 70), 6, None)])
def test_factorised_mask_features_equal_the_literal_form(C, H, W, size, M, mask_hw):
    r, m, g = R.feature_case(C, H, W, M, mask_hw)
    lit, n = R.mask_features(r, m, g, size)
    fac, n2 = R.mask_features_factorised(r, m, g, size)
    assert torch.equal(n, n2) and (lit - fac).abs().max() < 1e-13
    assert (n == 0).any() and (n > 0).any() and not lit[n == 0].any()            # an empty mask gives a zero row
    assert torch.allclose(lit[n > 0].norm(dim=1), torch.ones((n > 0).sum(), dtype=torch.float64))
    # the resampling is F.interpolate's
    want = torch.nn.functional.interpolate(r[None].double(), size, mode="bilinear", align_corners=False)[0]
    assert (R.bilinear(r, size, torch.float64) - want).abs().max() < 1e-12


def test_factorised_anchor_values_and_relevancy_equal_the_literal_forms():
    p, g, a = R.anchor_case(9, 70, 12)
    assert (R.anchor_values(p, g, a) - R.anchor_values_factorised(p, g, a)).abs().max() < 1e-13
    z = a.clone()
    z[3] = 0
    assert not (R.anchor_values(p, g, z)[:, 3] != 0).any() and not (R.anchor_values_factorised(p, g, z)[:, 3] != 0).any()
    for nm in (True, False):
        e, pos, neg = R.relevancy_case(40, 33, 3, 5)
        lit, fac = R.relevancy(e, pos, neg, nm), R.relevancy_factorised(e, pos, neg, nm)
        assert (lit - fac).abs().max() < 1e-13
        assert lit[20].sub(0.5).abs().max() == 0                                  # the zero row
        assert (R.relevancy(e.half(), pos, neg, nm) - R.relevancy(e.half().float(), pos, neg, nm)).abs().max() == 0
