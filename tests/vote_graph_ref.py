"""Restatement of the language-segmentation vote graph (seganygaussians_amd/vote_graph.py) in torch on the CPU,
written from the definitions: it forms the (M, C, h, w), (M, A, C) and (N, P, Q, 2) tensors literally.  `dtype=torch.float64` is the
reference; `dtype=torch.float32` evaluates the same expressions in the arithmetic the notebook has and supplies the tests'
yardstick (the error a float32 evaluation makes).  The `*_factorised` forms are what the kernels evaluate; the host tests check them
against the literal ones in float64.

The mask bits are decisions, not arithmetic: both dtypes take them from the float64 box sums (tests/mask_scales_ref.box_sums64)."""
import torch

from tests.mask_scales_ref import box_sums64


def src_index(n_out: int, n_in: int, dtype):
    """Lower tap, upper tap and upper weight of bilinear resampling with align_corners=False: src = max((dst + 0.5) n_in / n_out - 0.5, 0)."""
    dst = torch.arange(n_out, dtype=dtype)
    src = torch.clamp((dst + 0.5) * (float(n_in) / float(n_out)) - 0.5, min=0.0)
    i0 = src.floor().long().clamp(max=n_in - 1)
    i1 = torch.clamp(i0 + 1, max=n_in - 1)
    return i0, i1, src - i0.to(dtype)


def bilinear(x: torch.Tensor, size, dtype) -> torch.Tensor:
    """(..., H, W) -> (..., h, w), no antialiasing."""
    h, w = size
    x = x.to(dtype)
    y0, y1, ly = src_index(h, x.shape[-2], dtype)
    x0, x1, lx = src_index(w, x.shape[-1], dtype)
    top = x[..., y0, :][..., x0] * (1 - lx) + x[..., y0, :][..., x1] * lx
    bot = x[..., y1, :][..., x0] * (1 - lx) + x[..., y1, :][..., x1] * lx
    return top * (1 - ly)[:, None] + bot * ly[:, None]


def normalize(x: torch.Tensor, dim: int) -> torch.Tensor:
    return x / x.norm(dim=dim, keepdim=True).clamp_min(1e-12)


def mask_bits(masks: torch.Tensor, size, min_sum: float = 2.0):
    """(bits bool (M, h, w), box float64 (M, h, w)): the 3x3 zero-padded box sum of the bilinearly resampled masks, >= min_sum."""
    box = box_sums64(masks, size)
    return box >= min_sum, box


def mask_features(rendered, masks, gates, size=None, min_sum: float = 2.0, dtype=torch.float64):
    """(features (M, C), counts int64 (M,)), the literal form."""
    C, H, W = rendered.shape
    size = (H // 4, W // 4) if size is None else size
    bits, _ = mask_bits(masks, size, min_sum)
    f = bilinear(rendered, size, dtype)                                      # (C, h, w)
    u = normalize(gates.to(dtype)[:, :, None, None] * f[None], dim=1)        # (M, C, h, w)
    n = bits.sum(dim=(1, 2))
    s = (u * bits[:, None].to(dtype)).sum(dim=(2, 3)) / (n.to(dtype)[:, None] + 1e-9)
    return normalize(s, dim=1), n


def mask_features_factorised(rendered, masks, gates, size=None, min_sum: float = 2.0, dtype=torch.float64):
    """The same through the scalar w_mp = 1 / max(|g_m * f_p|, 1e-12): s_m = g_m * sum_p f_p w_mp / (n_m + 1e-9)."""
    C, H, W = rendered.shape
    size = (H // 4, W // 4) if size is None else size
    bits, _ = mask_bits(masks, size, min_sum)
    f = bilinear(rendered, size, dtype).reshape(C, -1)                       # (C, P)
    g = gates.to(dtype)
    wgt = bits.reshape(bits.shape[0], -1).to(dtype) / ((g * g) @ (f * f)).sqrt().clamp_min(1e-12)   # (M, P)
    n = bits.sum(dim=(1, 2))
    s = g * (wgt @ f.T) / (n.to(dtype)[:, None] + 1e-9)
    return normalize(s, dim=1), n


def anchor_values(phi, gates, anchors, dtype=torch.float64):
    """v (M, A) = <normalize(g_m * a_a), phi_m>, the literal form; the bit is v > threshold."""
    sa = normalize(gates.to(dtype)[:, None, :] * anchors.to(dtype)[None], dim=-1)   # (M, A, C)
    return (sa * phi.to(dtype)[:, None, :]).sum(-1)


def anchor_values_factorised(phi, gates, anchors, dtype=torch.float64):
    g, p, a = gates.to(dtype), phi.to(dtype), anchors.to(dtype)
    return ((g * p) @ a.T) / ((g * g) @ (a * a).T).sqrt().clamp_min(1e-12)


def relevancy(embeds, pos, neg, normalize_rows: bool = True, dtype=torch.float64):
    """(N, P): min over the negatives of softmax(10 [e . pos_p, e . neg_q])[0], the literal form."""
    e = embeds.float().to(dtype)
    if normalize_rows:
        e = normalize(e, dim=-1)
    p = e @ pos.to(dtype).T                                                  # (N, P)
    q = e @ neg.to(dtype).T                                                  # (N, Q)
    pairs = torch.stack([p[:, :, None].expand(-1, -1, q.shape[1]), q[:, None, :].expand(-1, p.shape[1], -1)], dim=-1)   # (N, P, Q, 2)
    return torch.softmax(10 * pairs, dim=-1)[..., 0].min(dim=2).values


def relevancy_factorised(embeds, pos, neg, normalize_rows: bool = True, dtype=torch.float64):
    e = embeds.float().to(dtype)
    if normalize_rows:
        e = normalize(e, dim=-1)
    return 1 / (1 + torch.exp(10 * ((e @ neg.to(dtype).T).max(dim=1, keepdim=True).values - e @ pos.to(dtype).T)))


def cluster_scores(scores, labels):
    """Mean score per label, noise first; K + 1 entries, NaN where a label has no rows."""
    K = int(labels.max()) + 1 if labels.numel() else 0
    out = torch.full((K + 1,), float("nan"), dtype=scores.dtype)
    for k in range(-1, K):
        if (labels == k).any():
            out[k + 1] = scores[labels == k].mean()
    return out


def cluster_queries(scores, labels, features, scales, min_score: float = 0.45):
    means = cluster_scores(scores, labels)
    present = [k for k in range(-1, len(means) - 1) if (labels == k).any()]
    good = [k for k in present if means[k + 1] > min_score]
    if not good:
        good = [max(present, key=lambda k: float(means[k + 1]))]
    queries, out_scales = [], []
    for k in good:
        rows = torch.nonzero(labels == k).flatten()
        row = rows[scores[rows].argmax()]
        queries.append(normalize(features[row], dim=-1))
        out_scales.append(scales.reshape(-1)[row])
    return torch.stack(queries), torch.stack(out_scales), torch.tensor(good), torch.stack([means[k + 1] for k in good])


# ---- inputs the host and GPU tests share ----------------------------------------------------------------------------------------
def mask_set(M: int, hm: int, wm: int, seed: int) -> torch.Tensor:
    """bool (M, hm, wm): a rectangle across the word seam (column 64, where the image has one), the full image, two diagonal pixels
    (one eroded pixel at the same size and min_sum = 2), an empty mask, a single pixel, then rectangles that overlap one another and
    touch the border, and random blobs; the first M of that list."""
    g = torch.Generator().manual_seed(seed)
    ms = []

    def rect(y0, y1, x0, x1):
        m = torch.zeros(hm, wm, dtype=torch.bool)
        m[max(y0, 0):max(y1, 1), max(x0, 0):max(x1, 1)] = True
        return m
    ms.append(rect(hm // 8, hm - hm // 8, min(wm // 8, 60), max(2 * wm // 3, min(wm, 70))))
    ms.append(torch.ones(hm, wm, dtype=torch.bool))
    diag = torch.zeros(hm, wm, dtype=torch.bool)
    diag[0, 0] = True
    diag[min(2, hm - 1), min(2, wm - 1)] = True
    ms.append(diag)
    ms.append(torch.zeros(hm, wm, dtype=torch.bool))
    one = torch.zeros(hm, wm, dtype=torch.bool)
    one[hm // 2, wm // 2] = True
    ms.append(one)
    k = 0
    while len(ms) < M:
        if k % 3 == 2:
            ms.append(torch.rand(hm, wm, generator=g) < 0.3 + 0.1 * (k % 5))
        else:
            y0, x0 = int(torch.randint(0, hm, (1,), generator=g)), int(torch.randint(0, wm, (1,), generator=g))
            dy, dx = int(torch.randint(1, hm + 1, (1,), generator=g)), int(torch.randint(1, wm + 1, (1,), generator=g))
            ms.append(rect(y0 - dy // 2, y0 + dy // 2 + 1, x0 - dx // 2, x0 + dx // 2 + 1))
        k += 1
    return torch.stack(ms[:M])


def feature_case(C, H, W, M, mask_hw=None, seed=0):
    """(rendered (C, H, W) with unit pixels, as norm_point_features renders are near, masks bool (M, hm, wm), gates (M, C) in (0, 1))."""
    g = torch.Generator().manual_seed(1000 + seed)
    rendered = normalize(torch.randn(C, H, W, generator=g) + torch.randn(C, 1, 1, generator=g), dim=0).float()
    hm, wm = (H, W) if mask_hw is None else mask_hw
    gates = torch.sigmoid(2 * torch.randn(M, C, generator=g)).float()
    return rendered, mask_set(M, hm, wm, seed), gates


def anchor_case(M, A, C, seed=0, centres=4):
    """(phi (M, C), gates (M, C), anchors (A, C)): a few cluster centres plus noise scaled with 1 / sqrt(C), so that a mask selects
    the anchors of its own centre and a sizeable share of the bits is set (random unit vectors would leave nearly every bit 0)."""
    g = torch.Generator().manual_seed(2000 + seed)
    ctr = normalize(torch.randn(centres, C, generator=g), dim=-1)
    gates = (0.3 + 0.7 * torch.rand(M, C, generator=g)).float()
    own_a = torch.arange(A) % centres
    own_m = torch.arange(M) % centres
    anchors = ((1 + torch.rand(A, 1, generator=g)) * (ctr[own_a] + 0.4 * torch.randn(A, C, generator=g) / C ** 0.5)).float()
    phi = normalize(gates * (ctr[own_m] + 0.4 * torch.randn(M, C, generator=g) / C ** 0.5), dim=-1).float()
    return phi, gates, anchors


def relevancy_case(N, D, P, Q, seed=0):
    g = torch.Generator().manual_seed(3000 + seed)
    pos = normalize(torch.randn(P, D, generator=g), dim=-1).float()
    neg = normalize(torch.randn(Q, D, generator=g), dim=-1).float()
    mix = torch.rand(N, 1, generator=g)
    embeds = (3 * torch.rand(N, 1, generator=g) * (mix * pos[torch.arange(N) % P] + (1 - mix) * neg[torch.arange(N) % Q]
                                                     + torch.randn(N, D, generator=g) / D ** 0.5)).float()
    embeds[N // 2] = 0          # a zero row: relevancy 1/2
    return embeds, pos, neg


def chain_case(seed=0, C=16, H=96, W=128):
    """A render of three regions with distinct unit features plus noise; 24 masks over the regions and parts of them at two scales
    (two gate vectors); 600 anchors drawn from the per-pixel features; made-up embeddings in which the masks of region 1 match the
    prompt.  Returns a dict."""
    g = torch.Generator().manual_seed(4000 + seed)
    region = torch.zeros(H, W, dtype=torch.long)
    region[:, W // 2:] = 1
    region[H // 2:, : W // 2] = 2
    ctr = normalize(torch.randn(3, C, generator=g), dim=-1)
    rendered = normalize(ctr[region].permute(2, 0, 1) + 0.05 * torch.randn(C, H, W, generator=g), dim=0).float()
    two_gates = (0.4 + 0.6 * torch.rand(2, C, generator=g)).float()
    masks, owner, scale_id = [], [], []
    for k in range(3):
        ys, xs = torch.nonzero(region == k, as_tuple=True)
        y0, y1, x0, x1 = int(ys.min()), int(ys.max()) + 1, int(xs.min()), int(xs.max()) + 1
        for j in range(8):
            m = torch.zeros(H, W, dtype=torch.bool)
            if j < 4:      # the region less a margin that grows with j
                m[y0 + 2 * j: y1 - 2 * j, x0 + 2 * j: x1 - 2 * j] = True
            else:          # a part of it
                cy, cx = (y0 + y1) // 2, (x0 + x1) // 2
                m[(y0 if j % 2 else cy): (cy if j % 2 else y1), (x0 if j < 6 else cx): (cx if j < 6 else x1)] = True
            masks.append(m)
            owner.append(k)
            scale_id.append(j % 2)
    owner, scale_id = torch.tensor(owner), torch.tensor(scale_id)
    pix = torch.randperm(H * W, generator=g)[:600]
    anchors = (rendered.reshape(C, -1).T[pix] * (0.5 + torch.rand(600, 1, generator=g))).float()
    D = 64
    prompt = normalize(torch.randn(1, D, generator=g), dim=-1).float()
    negs = normalize(torch.randn(4, D, generator=g), dim=-1).float()
    embeds = torch.where((owner == 1)[:, None], prompt, negs[owner]) + 0.05 * torch.randn(24, D, generator=g)
    return dict(rendered=rendered, region=region, masks=torch.stack(masks), owner=owner, scale_id=scale_id, two_gates=two_gates,
                gates=two_gates[scale_id], scales=(0.25 + 0.5 * scale_id).float(), anchors=anchors, embeds=embeds.float(),
                pos=prompt, neg=negs)
