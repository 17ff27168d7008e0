"""The contrastive-loss kernels (csrc/contrastive_loss.h) at the shapes where they branch, against the float64 reference of
tests/contrastive_ref.py (itself checked by tests/test_contrastive_ref.py).

Stages go through the C-ABI (include/mi_contrastive.h) and must match exactly: pack at every word / byte alignment, cover
(areas, the strict `ray_rand < rate`), targets + classes with the scale index at every 64-mask word edge.  The loss goes
through the public API with dyadic features, so every selection is the reference's and only rounding is left; the tolerances
are the summation-error bounds of the kernels' f32 arithmetic, with u = 2^-24:

  loss      |L - L64| <= 8 u A_L + u |L64|,     A_L = mean |positive terms| + mean |negative terms|  (float64)
  gradient  |g - g64| <= (S + 8) u A_g,         A_g[n, h, c] = sum_j |dcorr_hj| |f_jc|               (float64)

(each f32 term carries two roundings, the per-row sums in f64 are exact to far below u, one rounding per mean and one for
their sum; the gradient adds at most S - 1 fused multiply-adds per element after two roundings of the pair's factor)."""
import math

import pytest
import torch

from seganygaussians_amd import _lib
from seganygaussians_amd.contrastive_loss import contrastive_loss, sample_contrastive_targets
from tests.contrastive_ref import classes_ref, loss_ref64, pack_ref, targets_ref, weight_ref32

DEV = "cuda:0"
U = 2.0 ** -24
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _ok(rc):
    assert rc == 0, _lib.last_error()


def _masks(M, H, W, seed, cover_all=True):
    """Random overlapping masks, per-mask densities from sparse (2 %) to dense (52 %); cover_all: every pixel in some mask."""
    g = torch.Generator().manual_seed(seed)
    p = 0.02 + 0.5 * torch.rand(M, 1, 1, generator=g)
    masks = torch.rand(M, H, W, generator=g) < p
    if cover_all:
        masks[torch.randint(0, M, (H * W,), generator=g), torch.arange(H * W) // W, torch.arange(H * W) % W] = True
    return masks


def _word_edges(M):
    edges = {-1, M - 2, M - 1}
    for k in range(17):
        edges |= {64 * k - 1, 64 * k, 64 * k + 1}
    return sorted(si for si in edges if -1 <= si <= M - 1)


def _dyadic(N, S, C, seed):
    """Integers in [-4, 4] over a power of two d ~ (11 sqrt(C))^(1/2): corr = (sum of integer products) / d^2 is exact in f32
    and lands on 0, 0.5 and 0.75 often enough for ties to occur."""
    d = 2 ** round(math.log2(math.sqrt(11 * math.sqrt(C))))
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-4, 5, (N, S, C), generator=g).float() / d).to(DEV)


# ---- checks with the bounds of the module docstring ------------------------------------------------------------------------------

def _check_loss(loss, r):
    L, L64 = float(loss.detach()), float(r.loss)
    if math.isnan(L64):
        assert math.isnan(L), (L, L64)
    else:
        assert abs(L - L64) <= 8 * U * float(r.A_L) + U * abs(L64), (L, L64, float(r.A_L))


def _check_grad(g, g64, bound):
    g = g.double()
    assert torch.equal(g.isnan(), g64.isnan()), f"NaN pattern: {int(g.isnan().sum())} kernel, {int(g64.isnan().sum())} reference"
    fin = ~g64.isnan()
    err = (g - g64).abs()
    bad = fin & ~(err <= bound)
    if bad.any():
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{int(bad.sum())} gradient elements outside the bound; first {i}: kernel {float(g[tuple(i)])!r}, "
                             f"float64 {float(g64[tuple(i)])!r}, bound {float(bound[tuple(i)])!r}")


def _check_rel(x, x64, rtol):
    x, x64 = float(x), float(x64)
    if math.isnan(x64):
        assert math.isnan(x)
    else:
        assert abs(x - x64) <= rtol * abs(x64), (x, x64)


# ---- C-ABI stages: exact ---------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("W", [1, 7, 8, 63, 64, 65, 127, 128, 129, 1921])
def test_pack_every_width_and_byte_offset(W):
    """Rows of W bytes at storage offsets 0..7: the aligned 8-byte path, the byte loop for partial and misaligned words.  The
    bytes around the view are 0xFF, so a read past a row sets bits; the words past the output must stay untouched."""
    L = _lib.load()
    Wq = (W + 63) // 64
    for H in (1, 3, 17):
        for M in (1, 2, 65):
            masks = _masks(M, H, W, seed=W * 10007 + H * 101 + M, cover_all=False)
            want = pack_ref(masks).to(DEV)
            n, nw = M * H * W, M * H * Wq
            src = masks.reshape(-1).view(torch.uint8).to(DEV)
            for k in range(8):
                big = torch.full((n + 16,), 0xFF, dtype=torch.uint8, device=DEV)
                big[k:k + n] = src
                view = big[k:k + n].view(M, H, W)
                out = torch.full((nw + 4,), SENTINEL, dtype=torch.int64, device=DEV)
                _ok(L.mi_contrastive_pack_masks(M, H, W, view.data_ptr(), out.data_ptr(), _stream()))
                torch.cuda.synchronize()
                assert torch.equal(out[:nw].view(M, H, Wq), want), (M, H, W, k)
                assert bool((out[nw:] == SENTINEL).all()), (M, H, W, k)


@pytest.mark.gpu
@pytest.mark.parametrize("M,H,W", [(1, 1, 1), (3, 3, 100), (65, 17, 129), (1024, 40, 130), (7, 300, 200), (2, 1, 20000)])
def test_cover_areas_and_strict_rate(M, H, W):
    """Areas = masks.sum((1, 2)) in int64 and sampled_ray = any & (ray_rand < rate), with pixels at exactly the rate and one
    ulp either side; H * Wq from one word to more than one workgroup."""
    L = _lib.load()
    masks = _masks(M, H, W, seed=M + H + W, cover_all=False)
    masks[0, 0, 0] = True
    packed = pack_ref(masks).to(DEV)
    g = torch.Generator().manual_seed(M * H)
    rate = torch.tensor(0.37, dtype=torch.float32)
    ray_rand = torch.rand(H, W, generator=g)
    pick = torch.rand(H, W, generator=g)
    ray_rand[pick < 0.3] = rate
    ray_rand[(pick >= 0.3) & (pick < 0.4)] = torch.nextafter(rate, torch.tensor(0.0))
    ray_rand[(pick >= 0.4) & (pick < 0.5)] = torch.nextafter(rate, torch.tensor(1.0))
    ray_rand[0, 0] = rate
    acc = torch.zeros((5 + M + 4,), dtype=torch.int64, device=DEV)
    acc[5 + M:] = SENTINEL
    sampled = torch.full((H * W + 64,), 7, dtype=torch.uint8, device=DEV)
    rr = ray_rand.to(DEV)
    _ok(L.mi_contrastive_cover(M, H, W, packed.data_ptr(), rr.data_ptr(), float(rate), sampled.data_ptr(), acc.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(acc[5:5 + M].cpu(), masks.sum((1, 2), dtype=torch.int64))
    assert bool((acc[:5] == 0).all()) and bool((acc[5 + M:] == SENTINEL).all())
    want = masks.any(0) & (ray_rand < rate)
    assert torch.equal(sampled[:H * W].cpu().view(H, W), want.to(torch.uint8))
    assert bool((sampled[H * W:] == 7).all())
    assert bool((masks.any(0) & (ray_rand == rate)).any())


_TARGET_M = [1, 63, 64, 65, 128, 129, 1000, 1024]


@pytest.mark.gpu
@pytest.mark.parametrize("M", _TARGET_M)
@pytest.mark.parametrize("N", [1, 2, 10, 32])
def test_targets_and_classes_at_word_edges(M, N):
    """The scale index at every word edge (64 k - 1, 64 k, 64 k + 1, -1, M - 2, M - 1), upper bound off and on, N scales per
    launch until every edge has run: the gt words, the class counts, a bit-equal to the sequential f32 contract and within
    cnt u of float64, the max / ~min bits of a, and nothing written past the outputs."""
    L = _lib.load()
    H, W = 9, 70
    masks = _masks(M, H, W, seed=M)
    areas = masks.sum((1, 2), dtype=torch.int64)
    packed = pack_ref(masks).to(DEV)
    sort_idx = torch.randperm(M, generator=torch.Generator().manual_seed(M + 1)).to(DEV)
    yx = torch.nonzero(masks.any(0)).to(torch.int32).to(DEV).contiguous()
    S, Wd = int(yx.shape[0]), (M + 63) // 64
    edges = _word_edges(M)
    pairs = [(si, 0) for si in edges] + [(si, 1) for si in edges[::3]]
    ref = targets_ref(masks.to(DEV), sort_idx, yx, [p[0] for p in pairs], [p[1] for p in pairs])
    if M > 64:
        # several words per ray, and the highest covering mask <= si found in an earlier word than si's
        cov = masks.to(DEV)[sort_idx][:, yx[:, 0].long(), yx[:, 1].long()].T                # (S, M) sorted-mask cover
        per_word = torch.stack([cov[:, 64 * w:64 * (w + 1)].any(1) for w in range(Wd)], 1).sum(1)
        assert float((per_word >= 2).float().mean()) > (0.9 if M >= 128 else 0.1)
        cross = 0
        order = torch.arange(M, device=DEV)
        for si, ub in pairs:
            if ub or si < 0 or si % 64 == 63:
                continue
            hi = torch.where(cov & (order <= si), order, torch.full_like(order, -1)).max(1).values
            cross += int(((hi >= 0) & (hi // 64 < si // 64)).sum())
        assert cross > 0
    a_bits = ref.a.view(torch.int32).long() & 0xFFFFFFFF
    for start in range(0, len(pairs), N):
        chunk = [pairs[(start + i) % len(pairs)] for i in range(N)]
        cols = [(start + i) % len(pairs) for i in range(N)]
        si = torch.tensor([c[0] for c in chunk], dtype=torch.int32, device=DEV)
        ub = torch.tensor([c[1] for c in chunk], dtype=torch.int32, device=DEV)
        acc = torch.zeros((5 + M + 4,), dtype=torch.int64, device=DEV)
        acc[5:5 + M] = areas.to(DEV)
        acc[5 + M:] = SENTINEL
        gt = torch.full((S * N * Wd + 4,), SENTINEL, dtype=torch.int64, device=DEV)
        a = torch.full((S + 4,), -1.0, dtype=torch.float32, device=DEV)
        _ok(L.mi_contrastive_targets(M, H, W, packed.data_ptr(), sort_idx.data_ptr(), S, yx.data_ptr(), N, si.data_ptr(), ub.data_ptr(),
                                     gt.data_ptr(), a.data_ptr(), acc.data_ptr(), _stream()))
        torch.cuda.synchronize()
        want_gt = ref.gt[:, cols].contiguous()
        assert torch.equal(gt[:S * N * Wd].view(S, N, Wd), want_gt), chunk
        assert bool((gt[S * N * Wd:] == SENTINEL).all())
        _, counts = classes_ref(want_gt, M)
        assert torch.equal(acc[:3], counts), chunk
        assert torch.equal(a[:S].view(torch.int32), ref.a.view(torch.int32))
        assert bool((a[S:] == -1.0).all())
        assert int(acc[3]) == int(a_bits.max()) and int(acc[4]) == (~int(a_bits.min())) & 0xFFFFFFFF
        assert torch.equal(acc[5:5 + M].cpu(), areas) and bool((acc[5 + M:] == SENTINEL).all())
    assert bool(((ref.a.double() - ref.a64).abs() <= ref.cnt * U * ref.a64).all())


# ---- loss through the public API, dyadic features ---------------------------------------------------------------------------------

def _exact_s_masks(S, M, W, seed):
    """M bool masks on an (H, W) image whose union is exactly S pixels, chosen at random, each covered by one mask or more."""
    H = S // W + 2
    g = torch.Generator().manual_seed(seed)
    pix = torch.randperm(H * W, generator=g)[:S]
    covered = torch.zeros(H * W, dtype=torch.bool)
    covered[pix] = True
    masks = (torch.rand(M, H * W, generator=g) < 0.05 + 0.55 * torch.rand(M, 1, generator=g)) & covered
    masks[torch.randint(0, M, (S,), generator=g), pix] = True
    scales = torch.randperm(M, generator=g).float() / M + 0.01                       # distinct: one sort order
    return masks.view(M, H, W), scales


def _reference(tg, masks, scales, f, rand):
    """The float64 reference from the targets' rays and scales, after checking the kernels' targets against targets_ref."""
    sort_idx = torch.sort(scales.to(DEV), descending=True)[1]                          # distinct scales: the one order
    rt = targets_ref(masks.to(DEV), sort_idx, tg.ray_yx, tg.scale_index, tg.upper_bound)
    gt_corrs, counts = classes_ref(rt.gt, masks.shape[0])
    assert torch.equal(tg.gt, rt.gt)
    assert torch.equal(tg.mean_size.view(torch.int32), rt.a.view(torch.int32))
    assert torch.equal(tg.class_counts, counts)
    r = loss_ref64(f.detach(), gt_corrs, weight_ref32(rt.a), rand)
    assert torch.equal(counts, r.counts)
    return r


def _run(masks, scales, ub, N, feats, seed, rate=1.0):
    """contrastive_loss through the public API and the float64 reference from the same targets and the same device draw."""
    torch.manual_seed(seed)
    tg = sample_contrastive_targets(masks, scales, ub, ray_sample_rate=rate, num_sampled_scales=N - 2)
    S = tg.num_rays
    f = feats(N, S).requires_grad_(True)
    state = torch.cuda.get_rng_state(DEV)
    loss, stats = contrastive_loss(f, tg)
    (g,) = torch.autograd.grad(loss, f)
    torch.cuda.set_rng_state(state, DEV)
    rand = torch.rand((S, S), device=DEV, dtype=torch.float32)                          # the draw contrastive_loss made
    r = _reference(tg, masks, scales, f, rand)
    assert (int(stats.n_pos), int(stats.n_neg)) == (r.n_pos, r.n_neg)
    return tg, f, loss, stats, g, r


def _check_all(tg, f, loss, stats, g, r):
    S = tg.num_rays
    _check_loss(loss, r)
    _check_rel(stats.cosine_pos, r.cosine_pos, 1e-6)
    _check_rel(stats.cosine_neg, r.cosine_neg, 1e-6)
    _check_grad(g, r.grad, (S + 8) * U * r.A_g)


_S = [1, 2, 63, 64, 255, 256, 257, 513]
_C = [1, 3, 4, 5, 33, 255, 256]
_N = [2, 3, 10, 32]
_M = [2, 3, 63, 64, 65, 129, 300]
# every (S, C) pair once; N = _N[(i + k) % 4] covers every (S, N) and (C, N) pair too; N = 32 with M = 1024 (the largest LDS
# carve of the forward, 52 KiB) at S >= 255
_SWEEP = [(S, C, _N[(i + k) % 4], 1024 if _N[(i + k) % 4] == 32 and S >= 255 else _M[(i + 2 * k) % 7], (7, 64, 100)[(i + k) % 3])
          for i, S in enumerate(_S) for k, C in enumerate(_C)]


@pytest.mark.gpu
@pytest.mark.parametrize("S,C,N,M,W", _SWEEP)
def test_loss_sweep(S, C, N, M, W):
    seed = S * 7919 + C * 31 + N
    masks, scales = _exact_s_masks(S, M, W, seed)
    tg, f, loss, stats, g, r = _run(masks, scales, float(scales.max()), N, lambda n, s: _dyadic(n, s, C, seed), seed)
    assert tg.num_rays == S
    _check_all(tg, f, loss, stats, g, r)


@pytest.mark.gpu
def test_loss_large():
    """S = 4096: the f32 restatement of the reference would itself be off by more than the bound here."""
    S, C, N, M = 4096, 32, 10, 300
    masks, scales = _exact_s_masks(S, M, 64, seed=4096)
    tg, f, loss, stats, g, r = _run(masks, scales, float(scales.max()), N, lambda n, s: _dyadic(n, s, C, 1), 4096)
    assert tg.num_rays == S and r.n_pos > 0 and r.n_neg > 0
    _check_all(tg, f, loss, stats, g, r)


@pytest.mark.gpu
def test_upstream_gradient():
    """(2.5 loss + sum f^2).backward() gives 2.5 times the float64 gradient plus 2 f (one more rounding for autograd's sum),
    and 2.5 times the kernel's own unit-g gradient plus 2 f within twice that bound."""
    S, C, N, M = 300, 32, 10, 65
    masks, scales = _exact_s_masks(S, M, 64, seed=25)
    torch.manual_seed(25)
    tg = sample_contrastive_targets(masks, scales, float(scales.max()), ray_sample_rate=1.0, num_sampled_scales=N - 2)
    assert tg.num_rays == S
    f = _dyadic(N, S, C, 25)
    state = torch.cuda.get_rng_state(DEV)
    f1 = f.clone().requires_grad_(True)
    loss1, _ = contrastive_loss(f1, tg)
    (g1,) = torch.autograd.grad(loss1, f1)
    torch.cuda.set_rng_state(state, DEV)
    f2 = f.clone().requires_grad_(True)
    loss2, _ = contrastive_loss(f2, tg)
    (2.5 * loss2 + (f2 ** 2).sum()).backward()
    torch.cuda.set_rng_state(state, DEV)
    r = _reference(tg, masks, scales, f, torch.rand((S, S), device=DEV, dtype=torch.float32))
    assert torch.equal(loss1.view(torch.int32), loss2.view(torch.int32))
    _check_loss(loss2, r)
    want = 2.5 * r.grad + 2 * f.double()
    bound = 2.5 * (S + 8) * U * r.A_g + U * want.abs()
    _check_grad(f2.grad, want, bound)
    _check_grad(f2.grad, 2.5 * g1.double() + 2 * f.double(), 2 * bound)
    assert float(r.A_g.max()) > 0


# ---- C-ABI loss with chosen draws: the strict `rand < t`, ties of corr, g != 1 -------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("C", [5, 8])
def test_loss_ties_through_c_abi(C):
    """rand set to exactly t_pos / t_neg (and one ulp below) on pairs of those classes, corr exactly 0, 0.5 and 0.75 on
    pairs where they decide, g_loss = 2.5: forward and backward against the float64 reference with the same rand."""
    L = _lib.load()
    # 40 region masks of 8 pixels each partition the image; 10 group masks cover two regions each and sort first (larger
    # scale).  Rays of one region: consistent positive; of two regions in one group: positive at si = -1 and 5, negative at
    # si = 49 (each ray's highest covering mask is its region); the rest: consistent negative.  So 0 < t_pos, t_neg < 1.
    M, H, W, N = 50, 8, 40, 4
    region = torch.arange(H * W) // 8
    masks = torch.zeros(M, H * W, dtype=torch.bool)
    masks[region, torch.arange(H * W)] = True
    for grp in range(10):
        masks[40 + grp] = (region == 4 * grp) | (region == 4 * grp + 1)
    masks = masks.view(M, H, W)
    areas = masks.sum((1, 2), dtype=torch.int64)
    packed = pack_ref(masks).to(DEV)
    sort_idx = torch.cat([torch.arange(40, 50), torch.arange(40)]).to(DEV)
    yx = torch.nonzero(masks.any(0)).to(torch.int32).to(DEV).contiguous()
    S, Wd = int(yx.shape[0]), (M + 63) // 64
    si = torch.tensor([-1, 5, 20, 49], dtype=torch.int32, device=DEV)
    ub = torch.tensor([1, 0, 0, 0], dtype=torch.int32, device=DEV)
    acc = torch.zeros((5 + M,), dtype=torch.int64, device=DEV)
    acc[5:] = areas.to(DEV)
    gt = torch.empty((S, N, Wd), dtype=torch.int64, device=DEV)
    a = torch.empty((S,), dtype=torch.float32, device=DEV)
    _ok(L.mi_contrastive_targets(M, H, W, packed.data_ptr(), sort_idx.data_ptr(), S, yx.data_ptr(), N, si.data_ptr(), ub.data_ptr(),
                                 gt.data_ptr(), a.data_ptr(), acc.data_ptr(), _stream()))
    torch.cuda.synchronize()
    rt = targets_ref(masks.to(DEV), sort_idx, yx, si.tolist(), ub.tolist())
    assert torch.equal(gt, rt.gt) and torch.equal(a.view(torch.int32), rt.a.view(torch.int32))
    gt_corrs, counts = classes_ref(gt, M)
    assert torch.equal(acc[:3], counts)
    # :262-270 in f32 from the integer counts
    sampled_num = counts[2] / 2
    t_pos, t_neg = sampled_num / counts[0], sampled_num / counts[1]
    assert 0 < float(t_pos) < 1 and 0 < float(t_neg) < 1, (float(t_pos), float(t_neg))
    g = torch.Generator(device=DEV).manual_seed(C)
    rand = torch.rand((S, S), device=DEV, generator=g)
    sum_0 = gt_corrs.sum(0)
    pick = torch.rand((S, S), device=DEV, generator=g)
    cpos, cneg = sum_0 == N, sum_0 == 0
    rand = torch.where(cpos & (pick < 0.3), t_pos, rand)
    rand = torch.where(cpos & (pick >= 0.3) & (pick < 0.4), torch.nextafter(t_pos, torch.zeros_like(t_pos)), rand)
    rand = torch.where(cneg & (pick < 0.3), t_neg, rand)
    rand = torch.where(cneg & (pick >= 0.3) & (pick < 0.4), torch.nextafter(t_neg, torch.zeros_like(t_neg)), rand)
    rand = rand.contiguous()
    feats = _dyadic(N, S, C, seed=C).contiguous()
    partials = torch.empty((S, 8), dtype=torch.float64, device=DEV)
    out_f32 = torch.empty((3,), dtype=torch.float32, device=DEV)
    out_i64 = torch.empty((2,), dtype=torch.int64, device=DEV)
    _ok(L.mi_contrastive_loss_forward(S, N, C, M, feats.data_ptr(), gt.data_ptr(), a.data_ptr(), acc.data_ptr(), rand.data_ptr(),
                                      partials.data_ptr(), out_f32.data_ptr(), out_i64.data_ptr(), _stream()))
    g_loss = torch.tensor([2.5], dtype=torch.float32, device=DEV)
    d = torch.full((N, S, C), float("nan"), dtype=torch.float32, device=DEV)
    _ok(L.mi_contrastive_loss_backward(S, N, C, M, feats.data_ptr(), gt.data_ptr(), a.data_ptr(), acc.data_ptr(), rand.data_ptr(),
                                       out_i64.data_ptr(), g_loss.data_ptr(), d.data_ptr(), _stream()))
    torch.cuda.synchronize()
    r = loss_ref64(feats, gt_corrs, weight_ref32(a), rand)
    # the ties are there: rand == t on pairs of each class, corr == 0.75 / 0.5 / 0 where each decides
    triu = torch.ones((S, S), dtype=torch.bool, device=DEV).triu(1)
    assert bool((triu & cpos & (rand == t_pos)).any()) and bool((triu & cneg & (rand == t_neg)).any())
    corr = torch.einsum('nhc,njc->nhj', feats.double(), feats.double())
    assert bool((gt_corrs & (corr == 0.75)).any()) and bool((~gt_corrs & (corr == 0.5)).any())
    assert bool((r.neg.unsqueeze(0) & ~gt_corrs & (corr == 0)).any())
    assert (int(out_i64[0]), int(out_i64[1])) == (r.n_pos, r.n_neg)
    _check_loss(out_f32[0], r)
    _check_rel(out_f32[1], r.cosine_pos, 1e-6)
    _check_rel(out_f32[2], r.cosine_neg, 1e-6)
    _check_grad(d, 2.5 * r.grad, 2.5 * (S + 8) * U * r.A_g)


# ---- degenerate cases: values and NaN patterns -----------------------------------------------------------------------------------

@pytest.mark.gpu
def test_single_ray():
    """S = 1: no pair, loss NaN (0 / 0 means), gradient exactly 0 as in float64."""
    masks = torch.zeros(3, 4, 5, dtype=torch.bool)
    masks[:, 2, 3] = True
    masks[1, 0, :] = False
    scales = torch.tensor([0.3, 0.2, 0.1])
    tg, f, loss, stats, g, r = _run(masks, scales, 0.3, 10, lambda n, s: _dyadic(n, s, 8, 0), 1)
    assert tg.num_rays == 1
    assert math.isnan(float(loss)) and math.isnan(float(r.loss))
    assert torch.equal(g, torch.zeros_like(g)) and bool((r.grad == 0).all())
    assert (r.n_pos, r.n_neg) == (0, 0)


@pytest.mark.gpu
def test_every_ray_in_one_mask():
    """One mask under every ray with the smallest scale (last in sorted order, so in every ray's gt at every scale) and
    nested masks above it: every pair consistent positive, n_neg = 0 and t_neg = 0 / 0.  Loss NaN, gradient finite."""
    S, M, W = 200, 12, 20
    masks, scales = _exact_s_masks(S, M, W, seed=12)
    masks[0] = masks.any(0)
    scales[0] = 0.001
    tg, f, loss, stats, g, r = _run(masks, scales, float(scales.max()), 10, lambda n, s: _dyadic(n, s, 8, 12), 12)
    assert int(stats.class_counts[0]) == S * S and r.n_neg == 0 and r.n_pos > 0
    assert math.isnan(float(loss)) and math.isnan(float(r.loss))
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(r.grad).all())
    _check_grad(g, r.grad, (S + 8) * U * r.A_g)


@pytest.mark.gpu
def test_disjoint_masks():
    """Each mask holds exactly one sampled ray (the CPU draw of ray_rand replayed to place them), areas 1..5: every
    off-diagonal pair consistent negative, n_pos = 0, finite weights; loss NaN, gradient finite and bounded."""
    M, H, W, seed, rate = 40, 12, 32, 5, 0.25
    torch.manual_seed(seed)
    torch.randperm(M)                                                                   # the draws sample_contrastive_targets makes
    ray_rand = torch.rand(H, W)
    hits = (ray_rand.reshape(-1) < rate).nonzero()[:, 0]
    assert hits.numel() > M
    masks = torch.zeros(M, H * W, dtype=torch.bool)
    for m in range(M):
        start, stop = int(hits[m]), int(hits[m + 1])
        masks[m, start:min(stop, start + 1 + m % 5)] = True
    scales = torch.randperm(M, generator=torch.Generator().manual_seed(6)).float() / M + 0.01
    tg, f, loss, stats, g, r = _run(masks.view(M, H, W), scales, float(scales.max()), 10,
                                    lambda n, s: _dyadic(n, s, 4, 5), seed, rate=rate)
    assert tg.num_rays == M
    assert stats.class_counts.tolist() == [M, M * M - M, 0]
    assert r.n_pos == 0 and r.n_neg > 0
    assert math.isnan(float(loss)) and math.isnan(float(r.loss))
    assert bool(torch.isfinite(g).all())
    _check_grad(g, r.grad, (M + 8) * U * r.A_g)
    assert float(r.A_g.max()) > 0


@pytest.mark.gpu
def test_all_weights_equal_nan_pattern():
    """Two disjoint masks of equal area: every mean mask size equal, so every weight is 0 / 0.  The rays of mask A share one
    feature (corr 1: no positive hint) with corr <= 0.5 to every ray of B (no negative hint): their gradient rows are 0, while
    B's rows carry NaN.  The NaN pattern and the finite values must be the reference's."""
    S2, C, N = 60, 4, 10
    M, H, W = 2, 4, 30
    masks = torch.zeros(M, H, W, dtype=torch.bool)
    masks[0, :2] = True
    masks[1, 2:] = True
    scales = torch.tensor([0.5, 0.25])

    def feats(n, s):
        f = _dyadic(n, s, C, 3)
        f[..., 0] = f[..., 0].clamp(max=0.5)
        in_a = masks[0].reshape(-1)[masks.any(0).reshape(-1)].to(DEV)
        f[:, in_a] = torch.tensor([1.0, 0.0, 0.0, 0.0], device=DEV)
        return f

    tg, f, loss, stats, g, r = _run(masks, scales, 0.5, N, feats, 3)
    assert tg.num_rays == S2 * 2 and bool(torch.isnan(weight_ref32(tg.mean_size)).all())
    assert math.isnan(float(loss)) and math.isnan(float(r.loss))
    assert bool(g.isnan().any()) and bool((~g.isnan()).any())
    _check_grad(g, r.grad, (tg.num_rays + 8) * U * r.A_g)


# ---- feature alignment ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_misaligned_features_match_aligned_copy():
    """A contiguous (N, S, C) view at a 4-byte storage offset (C % 4 == 0: the float4 path of cl_pair_corr) gives the loss and
    gradient of an aligned copy, bit for bit."""
    S, C, N, M = 200, 32, 10, 40
    masks, scales = _exact_s_masks(S, M, 64, seed=9)
    torch.manual_seed(9)
    tg = sample_contrastive_targets(masks, scales, float(scales.max()), ray_sample_rate=1.0, num_sampled_scales=N - 2)
    f = _dyadic(N, S, C, 9) * 0.75
    buf = torch.zeros(N * S * C + 1, device=DEV)
    buf[1:] = f.reshape(-1)
    fv = buf[1:].view(N, S, C).detach().requires_grad_(True)
    assert fv.data_ptr() % 16 != 0 and fv.is_contiguous()
    fa = f.clone().requires_grad_(True)
    assert fa.data_ptr() % 16 == 0
    state = torch.cuda.get_rng_state(DEV)
    loss_v, _ = contrastive_loss(fv, tg)
    (gv,) = torch.autograd.grad(loss_v, fv)
    torch.cuda.set_rng_state(state, DEV)
    loss_a, _ = contrastive_loss(fa, tg)
    (ga,) = torch.autograd.grad(loss_a, fa)
    assert torch.equal(loss_v.view(torch.int32), loss_a.view(torch.int32))
    assert torch.equal(gv.view(torch.int32), ga.view(torch.int32))
    assert not math.isnan(float(loss_a))
