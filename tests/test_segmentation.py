"""GPU tests of the segmentation queries (seganygaussians_amd/segmentation.py) against the float64
restatement of tests/segmentation_ref.py.

Values (scores, score, best): |got - want| <= (2 C + 16) 2^-24 max(1, |q_k|), derived in segmentation_ref.value_bound.
Decisions (mask, label): equal to the restatement's except where the float64 margin -- |t_k - threshold| for the mask, the gap
between the two largest s_k for the label -- is at most twice that bound; the rows excused this way may be at most 1 % of N, and a
test fails on that cap alone.  The image and the points kernels do not share their summation order (a lane walks the C planes of its
pixel in order; eight lanes split a point's row and meet in a butterfly), so image == points holds within the value bound on each
side, not bit for bit.  select and assign with K <= 16 run the kernel of scores and are compared with its output exactly."""
import ctypes

import numpy as np
import pytest
import torch

from seganygaussians_amd import _lib
from seganygaussians_amd.segmentation import assign_clusters, select_by_similarity, similarity_scores
from tests import segmentation_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CAP = 0.01


def dev(t):
    return None if t is None else t.to(DEV)


def bshape(b, like):
    return b.reshape((-1,) + (1,) * (like.dim() - 1))


def check_scores(feats, queries, gates, pre, post):
    got = similarity_scores(dev(feats), dev(queries), dev(gates), pre=pre, post=post).cpu()
    want = ref.scores64(feats, queries, gates, pre, post)
    assert got.shape == want.shape and got.dtype == torch.float32
    b = ref.value_bound(feats.shape[0] if feats.dim() == 3 else feats.shape[1], queries)
    if not post:   # rows are not unit rows: the bound scales with |v|
        rows, shape = ref.rows_of(feats)
        v = ref._unit_rows64(rows, gates, pre, False).norm(dim=-1).clamp_min(1.0).reshape(shape)
        err = (got.double() - want).abs() / v
    else:
        err = (got.double() - want).abs()
    worst = (err / bshape(b, err)).max().item()
    print(f"scores {tuple(feats.shape)} Q={queries.shape[0]} pre={pre} post={post}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0
    return got


def check_select(feats, queries, thres, gates, pre, half_shift, cap=CAP):
    mask, score = select_by_similarity(dev(feats), dev(queries), thres, dev(gates), pre=pre, half_shift=half_shift)
    mask, score = mask.cpu(), score.cpu()
    wmask, wscore, t = ref.select64(feats, queries, thres, gates, pre, half_shift)
    assert mask.shape == wmask.shape and mask.dtype == torch.bool and score.dtype == torch.float32
    C = feats.shape[0] if feats.dim() == 3 else feats.shape[1]
    b = bshape(ref.value_bound(C, queries), t)
    near = (t - thres).abs() <= 2 * b
    band = near.any(0)
    share = band.double().mean().item()
    bmax = b.max().item()
    # admissible scores of a row: its in-band queries taken as not selected / as selected
    sel = t > thres
    zero = torch.zeros_like(t)
    lo = torch.where(sel & ~near, t, zero).max(0).values
    hi = torch.where(sel | near, t, zero).max(0).values
    wrong = (mask != wmask) & ~band
    worst = torch.maximum(lo - score.double(), score.double() - hi).max().item() / bmax
    print(f"select {tuple(feats.shape)} Q={queries.shape[0]} pre={pre} hs={half_shift}: excused {share:.5f}, wrong outside band "
          f"{int(wrong.sum())}, worst score error / bound = {worst:.3f}")
    assert not wrong.any()
    assert worst <= 1.0
    assert share <= cap
    return mask, score


def check_assign(feats, centers, gates, pre, cap=CAP):
    labels, best = assign_clusters(dev(feats), dev(centers), dev(gates), pre=pre)
    labels, best = labels.cpu(), best.cpu()
    wl, wb, gap, second = ref.assign64(feats, centers, gates, pre)
    assert labels.shape == wl.shape and labels.dtype == torch.int32 and best.dtype == torch.float32
    assert int(labels.min()) >= 0 and int(labels.max()) < centers.shape[0]
    C = feats.shape[0] if feats.dim() == 3 else feats.shape[1]
    b = ref.value_bound(C, centers)
    band = gap <= 2 * torch.maximum(b[wl], b[second])
    share = band.double().mean().item()
    wrong = (labels.long() != wl) & ~band
    worst = ((best.double() - wb).abs() / torch.maximum(b[wl], b[labels.long()])).max().item()
    print(f"assign {tuple(feats.shape)} K={centers.shape[0]} pre={pre}: excused {share:.5f}, wrong outside band {int(wrong.sum())}, "
          f"worst best error / bound = {worst:.3f}")
    assert not wrong.any()
    assert worst <= 1.0
    assert share <= cap
    return labels, best


# ---- shapes and modes -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 3, 16, 31, 32, 33, 64, 100, 256])
@pytest.mark.parametrize("layout", ["image", "points"])
def test_values_over_channels_and_modes(layout, C):
    shape = (5, 66) if layout == "image" else (333,)
    for i, (pre, gated, post) in enumerate([("none", True, True), ("l2", True, True), ("eps", True, True), ("eps", False, False),
                                            ("none", False, True), ("l2", True, False)]):
        feats, queries, gates = ref.make_case(layout, shape, C, (1, 4, 16, 3, 2, 5)[i], seed=100 + C + i, gated=gated)
        check_scores(feats, queries, gates, pre, post)
    feats, queries, gates = ref.make_case(layout, shape, C, 3, seed=250 + C)
    check_select(feats, queries, 0.6, gates, "none", True)
    check_select(feats, queries, 0.1, None, "eps", False)
    feats, centers, gates = ref.make_case(layout, shape, C, 40, seed=300 + C)
    check_assign(feats, centers, gates, "l2")
    check_assign(feats, centers[:7], None, "none")


@pytest.mark.parametrize("W", [1, 63, 64, 65, 1920])
def test_image_widths(W):
    for H in (1, 3):
        feats, queries, gates = ref.make_case("image", (H, W), 32, 4, seed=W + H)
        check_scores(feats, queries, gates, "eps", True)
        check_select(feats, queries, 0.6, gates, "eps", True)
        check_assign(feats, ref.make_case("points", (1,), 32, 33, seed=W)[1], gates, "l2")


@pytest.mark.parametrize("P", [1, 255, 256, 257, 1_000_003])
def test_point_counts(P):
    feats, queries, gates = ref.make_case("points", (P,), 32, 4, seed=P)
    check_scores(feats, queries, gates, "none", True)
    check_select(feats, queries, 0.6, gates, "none", True)
    check_assign(feats, ref.make_case("points", (1,), 32, 38, seed=P + 1)[1], gates, "l2")
    check_assign(feats, queries, gates, "l2")


def test_full_frame_1080p():
    feats, queries, gates = ref.make_case("image", (1080, 1920), 32, 1, seed=1080)
    check_scores(feats, queries, gates, "eps", True)
    check_select(feats, queries, 0.6, gates, "eps", True)
    check_assign(feats, ref.make_case("points", (1,), 32, 17, seed=17)[1], gates, "l2")


@pytest.mark.parametrize("case", ref.CAP_CASES, ids=lambda c: f"{c[0]}-{c[1]}-C{c[2]}-Q{c[3]}")
def test_select_decisions(case):
    layout, shape, C, Q, seed = case
    feats, queries, gates = ref.make_case(layout, shape, C, Q, seed)
    check_select(feats, queries, 0.6, gates, "none", True)
    check_select(feats, queries, 0.2, gates, "none", False)


@pytest.mark.parametrize("case", ref.ASSIGN_CASES, ids=lambda c: f"{c[0]}-{c[1]}-C{c[2]}-K{c[3]}")
def test_assign_decisions(case):
    layout, shape, C, K, seed = case
    feats, centers, gates = ref.make_case(layout, shape, C, K, seed)
    check_assign(feats, centers, gates, "l2")


# ---- exact cases ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["image", "points"])
def test_zero_rows(layout):
    C = 32
    feats = torch.zeros((C, 4, 9) if layout == "image" else (36, C))
    _, queries, gates = ref.make_case("points", (1,), C, 16, seed=5)
    for pre in ("none", "l2", "eps"):
        s = similarity_scores(dev(feats), dev(queries), dev(gates), pre=pre).cpu()
        assert (s == 0).all()
        mask, score = select_by_similarity(dev(feats), dev(queries), 0.5, dev(gates), pre=pre, half_shift=True)
        assert not mask.any() and (score == 0).all()          # t = 0.5 is not > 0.5
        mask, score = select_by_similarity(dev(feats), dev(queries), 0.25, dev(gates), pre=pre, half_shift=True)
        assert mask.all() and (score == 0.5).all()
        for K in (1, 16, 17, 600):
            centers = ref.make_case("points", (1,), C, K, seed=K)[1]
            labels, best = assign_clusters(dev(feats), dev(centers), dev(gates), pre=pre)
            assert (labels == 0).all() and (best == 0).all()


def seam_counts(C):
    kb = _lib.load().mi_segment_assign_block(C)
    assert kb > 0 and kb % 32 == 0
    return sorted({1, 2, 16, 17, 31, 32, 33, kb - 1, kb, kb + 1, 2 * kb - 1, 2 * kb, 2 * kb + 1, 4096})


@pytest.mark.parametrize("C", [32, 64, 100, 256])
@pytest.mark.parametrize("layout", ["image", "points"])
def test_row_equal_to_one_centre_and_duplicates(layout, C):
    """Centres on coordinate axes (K <= C) or rows of +-1 sign patterns: a row equal to centre j beats every other centre by a wide
    margin, wherever j falls in the LDS blocks; a duplicate of the winning centre at a higher index never wins."""
    g = torch.Generator().manual_seed(C)
    for K in seam_counts(C):
        if K <= C:
            centers = torch.eye(C)[:K].clone()
        else:
            centers = torch.nn.functional.normalize(torch.randn(K, C, generator=g), dim=-1)
        N = 200
        want = torch.cat([torch.tensor([0, K - 1, K // 2]), torch.randint(0, K, (N - 3,), generator=g)])
        rows = centers[want] * (0.5 + torch.rand(N, 1, generator=g))
        # a later duplicate of each row's centre: put copies of the first half of the centres at the end
        dup = torch.cat([centers, centers[: max(1, K // 2)]])[:4096]
        feats = rows.t().reshape(C, 10, 20).contiguous() if layout == "image" else rows
        if K <= C:
            labels, best = assign_clusters(dev(feats), dev(centers), None, pre="l2")
            assert torch.equal(labels.cpu().reshape(-1).long(), want)
            assert (best.cpu().reshape(-1) - 1).abs().max() <= (2 * C + 16) * 2.0 ** -24
        else:   # random unit centres: the restatement decides (gaps are wide, checked there)
            wl, _, gap, _ = ref.assign64(feats, centers, None, pre="l2")
            assert (gap > 1e-3).all() and torch.equal(wl.reshape(-1), want)
            labels, _ = assign_clusters(dev(feats), dev(centers), None, pre="l2")
            assert torch.equal(labels.cpu().reshape(-1).long(), want)
        labels, _ = assign_clusters(dev(feats), dev(dup), None, pre="l2")
        assert torch.equal(labels.cpu().reshape(-1).long(), want)


def test_duplicated_centres_take_the_lower_index():
    feats, centers, gates = ref.make_case("points", (3000,), 32, 50, seed=9)
    l1, b1 = assign_clusters(dev(feats), dev(centers), dev(gates))
    l2, b2 = assign_clusters(dev(feats), dev(torch.cat([centers, centers, centers])), dev(gates))
    assert torch.equal(l1, l2) and torch.equal(b1, b2)
    l3, _ = assign_clusters(dev(feats), dev(torch.cat([centers[:5], centers[:5]])), dev(gates))   # K <= 16 path
    assert int(l3.max()) < 5


def test_rows_past_n_untouched():
    L = _lib.load()
    C, pad, canary = 32, 64, -123.0
    stream = torch.cuda.current_stream(DEV).cuda_stream
    for layout, N in ((0, 5 * 65), (0, 4 * 64), (1, 257), (1, 1)):
        feats = dev(torch.randn(C * N))
        for Q in (1, 4, 16):
            q = dev(torch.randn(Q, C))
            out = torch.full((Q * N + pad,), canary, device=DEV)
            assert L.mi_segment_scores(layout, N, C, Q, feats.data_ptr(), q.data_ptr(), None, 0, 1, out.data_ptr(), stream) == 0
            assert (out[Q * N:] == canary).all() and (out[:Q * N] != canary).all()
            mask = torch.full((N + pad,), 77, device=DEV, dtype=torch.uint8)
            score = torch.full((N + pad,), canary, device=DEV)
            assert L.mi_segment_select(layout, N, C, Q, feats.data_ptr(), q.data_ptr(), None, 0, 1, 0.5, mask.data_ptr(), score.data_ptr(),
                                       stream) == 0
            assert (mask[N:] == 77).all() and (mask[:N] <= 1).all() and (score[N:] == canary).all() and (score[:N] != canary).all()
        for K in (3, 17, 600):
            c = dev(torch.randn(K, C))
            labels = torch.full((N + pad,), -5, device=DEV, dtype=torch.int32)
            best = torch.full((N + pad,), canary, device=DEV)
            assert L.mi_segment_assign(layout, N, C, K, feats.data_ptr(), c.data_ptr(), None, 1, labels.data_ptr(), best.data_ptr(), stream) == 0
            assert (labels[N:] == -5).all() and (labels[:N] >= 0).all() and (best[N:] == canary).all() and (best[:N] != canary).all()


# ---- equivalences ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,Q", [(32, 1), (64, 4), (33, 16), (256, 2)])
def test_image_equals_points_within_the_value_bound(C, Q):
    feats, queries, gates = ref.make_case("image", (7, 65), C, Q, seed=C + Q)
    rows = feats.reshape(C, -1).t().contiguous()
    a = similarity_scores(dev(feats), dev(queries), dev(gates), pre="l2").cpu().reshape(Q, -1).double()
    p = similarity_scores(dev(rows), dev(queries), dev(gates), pre="l2").cpu().double()
    want = ref.scores64(rows, queries, gates, "l2")
    b = ref.value_bound(C, queries)[:, None]
    assert ((a - want).abs() <= b).all() and ((p - want).abs() <= b).all()
    # a transposed view of the points is copied, documented: the same numbers as the image kernel then
    v = similarity_scores(dev(feats).reshape(C, -1).t(), dev(queries), dev(gates), pre="l2").cpu().double()
    assert torch.equal(v, p)


@pytest.mark.parametrize("layout,shape", [("image", (9, 130)), ("points", (2049,))])
@pytest.mark.parametrize("Q", [1, 3, 16])
def test_select_and_small_assign_equal_scores_output(layout, shape, Q):
    feats, queries, gates = ref.make_case(layout, shape, 32, Q, seed=Q)
    for pre in ("none", "l2", "eps"):
        s = similarity_scores(dev(feats), dev(queries), dev(gates), pre=pre)
        for hs, thres in ((True, 0.55), (False, 0.1), (False, -0.2)):
            t = (s + 1.0) / 2 if hs else s
            b = t > thres
            mask, score = select_by_similarity(dev(feats), dev(queries), thres, dev(gates), pre=pre, half_shift=hs)
            assert torch.equal(mask, b.any(0))
            assert torch.equal(score, torch.where(b, t, torch.zeros_like(t)).max(0).values)
        labels, best = assign_clusters(dev(feats), dev(queries), dev(gates), pre=pre)
        assert torch.equal(labels.cpu().long(), s.cpu().argmax(0)) and torch.equal(best, s.max(0).values)


def test_two_runs_bit_identical():
    feats, queries, gates = ref.make_case("points", (100_003,), 64, 4, seed=77)
    centers = ref.make_case("points", (1,), 64, 300, seed=78)[1]
    f, q, g, c = dev(feats), dev(queries), dev(gates), dev(centers)
    runs = []
    for _ in range(2):
        runs.append((similarity_scores(f, q, g), *select_by_similarity(f, q, 0.6, g), *assign_clusters(f, c, g)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_inputs_checked_on_the_device_too():
    f, q = torch.zeros(10, 8, device=DEV), torch.zeros(2, 8, device=DEV)
    with pytest.raises(ValueError, match="GPU"):
        similarity_scores(f, q.cpu())
    with pytest.raises(ValueError, match="requires grad"):
        assign_clusters(f.clone().requires_grad_(), q)
    with torch.no_grad():
        labels, _ = assign_clusters(f.clone().requires_grad_(), q)
    assert not labels.requires_grad and (labels == 0).all()
    s = similarity_scores(f, q[0])      # (C,) query
    assert s.shape == (1, 10)


# ---- end to end -----------------------------------------------------------------------------------------------------------------

def test_render_then_select_on_image_and_gaussians():
    """saga_gui.py:590-599, 633-652, 673-679 on a rendered synthetic scene: the query is the gated, normalised feature of a clicked
    pixel (:637), the selection runs on the render and on the Gaussians' own features."""
    from seganygaussians_amd import install_dropin
    from tests import helpers as hp
    install_dropin()
    from diff_gaussian_rasterization_contrastive_f import GaussianRasterizationSettings, GaussianRasterizer
    inp = hp.make_inputs(4000, 192, 128, 32, seed=0)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(DEV)
    settings = GaussianRasterizationSettings(
        image_height=inp.image_height, image_width=inp.image_width, tanfovx=inp.tanfovx, tanfovy=inp.tanfovy,
        bg=torch.zeros(32, device=DEV), scale_modifier=1.0, viewmatrix=t(inp.viewmatrix), projmatrix=t(inp.projmatrix), sh_degree=0,
        campos=t(inp.campos), prefiltered=False, debug=False)
    point_feats = t(inp.colors_precomp) - 0.5      # signed, as trained features are
    means3D = t(inp.means3D)
    with torch.no_grad():
        rendered, _ = GaussianRasterizer(settings)(means3D=means3D, means2D=torch.zeros_like(means3D), shs=None,
                                                   colors_precomp=point_feats, opacities=t(inp.opacities), scales=t(inp.scales),
                                                   rotations=t(inp.rotations), cov3D_precomp=None)
    C, H, W = rendered.shape
    gates = torch.rand(C, generator=torch.Generator().manual_seed(3)) * 0.9 + 0.05
    norms = rendered.norm(dim=0)
    y, x = divmod(int(norms.argmax()), W)
    # :637 -- the clicked pixel of the gated, normalised feature map
    full = similarity_scores(rendered, torch.eye(C, device=DEV)[:16], dev(gates), pre="eps")      # w itself, 16 channels at a time
    full = torch.cat([full, similarity_scores(rendered, torch.eye(C, device=DEV)[16:], dev(gates), pre="eps")])
    query = full[:, y, x].contiguous()
    # a threshold that splits the frame: the median of t over the render (neighbouring pixels blend the same Gaussians, so a fixed
    # 0.7 would take all of this small scene)
    t_img = (similarity_scores(rendered, query, dev(gates), pre="eps") + 1.0) / 2
    thres = round(float(t_img.median()), 3)
    mask, score = select_by_similarity(rendered, query, thres, dev(gates), pre="eps", half_shift=True)
    assert mask[y, x] and abs(float(score[y, x]) - 1.0) < 1e-5
    r, qc, pf = rendered.cpu(), query.cpu(), point_feats.cpu()
    wmask, wscore, tt = ref.select64(r, qc[None], thres, gates, "eps", True)
    b = ref.value_bound(C, qc[None])[0]
    band = ((tt - thres).abs() <= 2 * b).any(0)
    assert not (mask.cpu() != wmask)[~band].any() and band.double().mean() <= CAP
    assert ((score.cpu().double() - wscore)[~band].abs() <= b).all()
    assert wmask.any() and not wmask.all()
    pmask, pscore = select_by_similarity(point_feats, query, thres, dev(gates), pre="none", half_shift=True)
    wpm, wps, pt = ref.select64(pf, qc[None], thres, gates, "none", True)
    pband = ((pt - thres).abs() <= 2 * b).any(0)
    assert not (pmask.cpu() != wpm)[~pband].any() and pband.double().mean() <= CAP
    assert ((pscore.cpu().double() - wps)[~pband].abs() <= b).all()
