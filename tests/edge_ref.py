"""References and the tolerance rule of the edge-case tests of the side kernels that feed SAGA's feature training:
the KNN feature smoothing (tests/test_knn_smooth_edges.py), its multi-resolution form (tests/test_multi_res_smooth_edges.py) and
the contrastive front end (tests/test_contrastive_frontend_edges.py).

The rule is the one of tests/photometric_ref.py (FACTOR, FLOOR), applied per GROUP of equal scale, never per whole tensor:

    E32   = max over the group of |float32 reference expression on the CPU - float64 restatement|      (on that very input)
    bound = max(FACTOR * E32, FLOOR * magnitude of the terms summed into the group)
    every element of the group:  |product - float64| <= bound

The floor takes the magnitude of the TERMS, not of the result, so that a group whose terms cancel keeps a bound.  No element
is excused."""
from __future__ import annotations

import numpy as np
import torch

from oracle import knn_smooth_oracle as ko
from tests.photometric_ref import FACTOR, FLOOR


KNN_GRAD_FLOOR = 2.0 ** -21   # floor of a dL/dF_j row of the smoothing (see tests/test_knn_smooth_edges.py for the measurement)
OUT_ROW_FLOOR = 2.0 ** -21    # floor of an out row (n, s, :) of the front end (tests/test_contrastive_frontend_edges.py)


def ratios(product, f64, f32, magnitude, rows: bool = False, floor: float = FLOOR) -> np.ndarray:
    """error / bound per group: one group per leading index (the last axis is the group) when `rows`, else one group."""
    product, f64, f32 = (np.asarray(a, np.float64) for a in (product, f64, f32))
    assert product.shape == f64.shape == f32.shape, (product.shape, f64.shape, f32.shape)
    if f64.size == 0:
        return np.zeros(1)
    ax = -1 if rows else None
    with np.errstate(invalid="ignore"):
        err = np.abs(product - f64).max(axis=ax)          # NaN / inf in the product stay NaN / inf: never <= 1
    e32 = np.abs(f32 - f64).max(axis=ax)
    bound = np.maximum(FACTOR * e32, floor * np.asarray(magnitude, np.float64))
    return np.atleast_1d(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)))


# ---- KNN feature smoothing ----------------------------------------------------------------------------------------------------

def knn_expression(F, idx, cols, normalize_out, g, dtype, channel_perm=None, reverse_cols=False):
    """scene/gaussian_model_ff.py:354-362 + gaussian_renderer/__init__.py:362-363 by PyTorch autograd on the CPU in `dtype`;
    (out, dL/dF) as float64.  channel_perm / reverse_cols give the same expression another float evaluation order (the channels
    permuted before and restored after, the selected columns gathered last to first)."""
    F, g = np.asarray(F), np.asarray(g)
    cols = list(cols)[::-1] if reverse_cols else list(cols)
    perm = np.arange(F.shape[1]) if channel_perm is None else np.asarray(channel_perm)
    inv = np.argsort(perm)
    f = torch.tensor(F[:, perm], dtype=dtype, requires_grad=True)
    normed = torch.nn.functional.normalize(f, dim=-1, p=2)
    sel = torch.as_tensor(np.asarray(idx))[:, torch.as_tensor(cols)]
    ret = normed[sel, :].mean(dim=1)
    if normalize_out:
        ret = ret / (ret.norm(dim=1, keepdim=True) + 1e-9)
    ret.backward(torch.tensor(g[:, perm], dtype=dtype))
    return ret.detach().double().numpy()[:, inv], f.grad.double().numpy()[:, inv]


def knn_magnitudes(F, idx, cols, g, normalize_out):
    """Magnitude of the terms summed into every output row and every dL/dF row (float64):
    out_i  : mean over the selected columns of |n_j| (largest channel), divided by |m_i| + 1e-9 when normalize_out;
    dL/dF_j: sum over the selected references to j of |dL/dm_i| (largest channel) / max(|F_j|, 1e-12)."""
    F = np.asarray(F, np.float64)
    idx = np.asarray(idx)
    cols = np.asarray(list(cols), np.int64)
    nrm = np.maximum(np.linalg.norm(F, axis=1, keepdims=True), 1e-12)
    n = F / nrm
    mag_out = np.abs(n)[idx[:, cols], :].mean(axis=1).max(axis=1)
    if normalize_out:
        mag_out = mag_out / (np.linalg.norm(n[idx[:, cols], :].mean(axis=1), axis=1) + 1e-9)
    dm = np.abs(ko.dmean(F, idx, cols, g, normalize_out))
    acc = np.zeros_like(F)
    for c in cols:
        np.add.at(acc, idx[:, c], dm)
    return mag_out, acc.max(axis=1) / nrm[:, 0]


def knn_check(name, F, idx, cols, g, normalize_out, out, dF):
    """The rule for one run of the smoothing: prints error / bound per group class, then asserts it for every row."""
    want_o, want_g = ko.forward(F, idx, cols, normalize_out), ko.backward(F, idx, cols, g, normalize_out)
    o32, g32 = knn_expression(F, idx, cols, normalize_out, g, torch.float32)
    mag_o, mag_g = knn_magnitudes(F, idx, cols, g, normalize_out)
    r_o = ratios(out, want_o, o32, mag_o, rows=True)
    r_g = ratios(dF, want_g, g32, mag_g, rows=True, floor=KNN_GRAD_FLOOR)
    print(f"{name}: error / bound  out rows {np.nanmax(r_o):.3f}  dL/dF rows {np.nanmax(r_g):.3f}")
    assert (r_o <= 1.0).all(), (name, "out", int(np.argmax(~(r_o <= 1.0))), float(np.nanmax(r_o)))
    assert (r_g <= 1.0).all(), (name, "dL/dF", int(np.argmax(~(r_g <= 1.0))), float(np.nanmax(r_g)))
    return float(r_o.max()), float(r_g.max())


# ---- multi-resolution KNN feature smoothing ------------------------------------------------------------------------------------

MULTI_OUT_FLOOR = FLOOR            # floor of an out row                     } confirmed by two float32 evaluation orders on every
MULTI_GRAD_FLOOR = KNN_GRAD_FLOOR  # floor of a dL/dF_j row                  } case of tests/test_multi_res_smooth_edges.py (figures
MULTI_DW_FLOOR = FLOOR             # floor of a dL/dw entry / row            } in that module's docstring)


def multi_res_magnitudes(F, levels, w, g, normalize_out):
    """Magnitude of the terms summed into every group of the multi-resolution smoothing (tests/multi_res_smooth_ref.py), float64:
    out_i   : largest channel of sum_l |w_il| (1/k_l) sum_s |n_idx(i,l,s)|, divided by |ret_i| + 1e-9 when normalize_out;
    dL/dF_j : largest channel of sum over the references (i, l, s) to j of (|w_il| / k_l) T_i, divided by max(|F_j|, 1e-12), with
              T_i the terms of dL/dret_i per channel: |g_i|, or |g_i| a + |ret_i| |b| under normalize_out (a = 1 / (r + 1e-9),
              b = (ret_i . g_i) a^2 / r, 0 at r = 0; r = |ret_i|);
    dL/dw   : |T_i| |mean_{l,i}| (Cauchy-Schwarz) per entry (i, l); under normalize_out one value per row i, the largest over l
              (the entries of a row cancel against each other there); summed over i for one shared row of weights.
    Returns (mag_out (P,), mag_dF (P,), mag_dw or None): mag_dw has the shape of dL/dw without normalize_out, and one value per
    row of dL/dw with it."""
    F, g = np.asarray(F, np.float64), np.asarray(g, np.float64)
    P, L = F.shape[0], len(levels)
    nrm = np.maximum(np.linalg.norm(F, axis=1, keepdims=True), 1e-12)
    n = F / nrm
    gidx = [np.flatnonzero(np.asarray(pm, bool))[np.asarray(idx, np.int64)] for pm, idx in levels]      # global indices, (P, k_l)
    W = np.ones((P, L)) if w is None else np.broadcast_to(np.asarray(w, np.float64), (P, L))
    means = [n[gi, :].mean(axis=1) for gi in gidx]
    ret = sum(W[:, l:l + 1] * means[l] for l in range(L))
    mag_out = sum(np.abs(W[:, l:l + 1]) * np.abs(n)[gidx[l], :].mean(axis=1) for l in range(L)).max(axis=1)
    T = np.abs(g)
    if normalize_out:
        r = np.linalg.norm(ret, axis=1, keepdims=True)
        a = 1.0 / (r + 1e-9)
        with np.errstate(divide="ignore", invalid="ignore"):
            b = np.where(r > 0, (ret * g).sum(axis=1, keepdims=True) * a * a / r, 0.0)
        mag_out = mag_out / (r[:, 0] + 1e-9)
        T = T * a + np.abs(ret) * np.abs(b)
    acc = np.zeros_like(F)
    for l, gi in enumerate(gidx):
        contrib = np.abs(W[:, l:l + 1]) / gi.shape[1] * T
        for s in range(gi.shape[1]):
            np.add.at(acc, gi[:, s], contrib)
    mag_dF = acc.max(axis=1) / nrm[:, 0]
    if w is None:
        return mag_out, mag_dF, None
    terms = np.stack([np.linalg.norm(T, axis=1) * np.linalg.norm(m, axis=1) for m in means], axis=1)   # (P, L)
    if np.asarray(w).shape[0] == 1:
        terms = terms.sum(axis=0, keepdims=True)
    return mag_out, mag_dF, terms.max(axis=1) if normalize_out else terms


def multi_res_check(name, F, levels, w, g, normalize_out, out, dF, dw):
    """The rule for one run of the multi-resolution smoothing: truth is multi_res_smooth_ref.forward_backward (float64 autograd),
    E32 comes from multi_res_smooth_ref.expression in float32 on the CPU.  Groups: every out row, every dL/dF row, and of dL/dw
    every entry (without normalize_out) or every row (with it).  Prints error / bound per class, asserts every group, returns the
    worst per class (dL/dw: None without weights)."""
    from tests import multi_res_smooth_ref as mref
    want_o, want_g, want_w = mref.forward_backward(F, levels, w, normalize_out, g)
    o32, g32, w32 = mref.float32_expression(F, levels, w, normalize_out, g)
    mag_o, mag_g, mag_w = multi_res_magnitudes(F, levels, w, g, normalize_out)
    r_o = ratios(out, want_o, o32, mag_o, rows=True, floor=MULTI_OUT_FLOOR)
    r_g = ratios(dF, want_g, g32, mag_g, rows=True, floor=MULTI_GRAD_FLOOR)
    classes = [("out rows", r_o), ("dL/dF rows", r_g)]
    if w is None:
        assert dw is None, (name, "dL/dw without weights")
    else:
        dw = np.asarray(dw, np.float64)
        assert dw.shape == want_w.shape, (name, "dL/dw shape", dw.shape, want_w.shape)
        if normalize_out:
            r_w = ratios(dw, want_w, w32, mag_w, rows=True, floor=MULTI_DW_FLOOR)
        else:
            r_w = ratios(dw[..., None], want_w[..., None], w32[..., None], mag_w, rows=True, floor=MULTI_DW_FLOOR).reshape(-1)
        classes.append(("dL/dw rows" if normalize_out else "dL/dw entries", r_w))
    worst = [float("nan") if np.isnan(r).any() else float(r.max()) for _, r in classes]
    print(f"{name}: error / bound  " + "  ".join(f"{k} {v:.3f}" for (k, _), v in zip(classes, worst)))
    for (k, r), v in zip(classes, worst):
        assert (r <= 1.0).all(), (name, k, int(np.argmax(~(r <= 1.0))), v)
    return tuple(worst) + ((None,) if w is None else ())


# ---- contrastive front end ----------------------------------------------------------------------------------------------------

def taps_f32(n_out: int, n_in: int):
    """Lower tap, upper tap and upper weight of every output index of a bilinear resize n_in -> n_out with align_corners=False, AS
    ATen COMPUTES THEM FOR FLOAT32 INPUT (area_pixel_compute_source_index; bilinear_tap of csrc/contrastive.h, which stays beside
    pm_source_taps of csrc/packed_masks.h: the same source index, lam not clamped):
    scale = float32(n_in) / float32(n_out), src = max(fma(dst + 0.5, scale, -0.5), 0) -- ATen's builds contract the multiply and
    the subtraction into one fused operation -- and lam = src - i0, rounded to float32.  (The product of two float32 numbers, one of
    them a small integer + 0.5, minus 0.5 is exact in float64, so one rounding of the float64 result is the fused operation.)
    A float64 weight differs from these by about n_in * 2^-24, far more than the bound of the tests allows; so does, at a few
    indices, the unfused float32 form."""
    f = np.float32
    scale = f(n_in) / f(n_out)
    dst = np.arange(n_out, dtype=np.float32) + f(0.5)
    src = np.maximum((dst.astype(np.float64) * np.float64(scale) - 0.5).astype(np.float32), f(0.0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    lam = (src - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, lam


def front_end(rendered, out_hw, ray_yx, gates, dtype, up, gn, channel_perm=None, reverse=False):
    """train_contrastive_feature.py:234-254 for the rays `ray_yx` (S, 2) in `dtype` on the CPU: sample_scale_conditioned_features
    (seganygaussians_amd/contrastive_frontend.py) with the float32 taps above, plus rendered.norm(dim=0).mean().  Returns float64
    tensors: out (N, S, C), norm, d_tap = d<out, up>/d rendered, d_gates = d<out, up>/d gates, d_dense = gn d norm / d rendered;
    in float64 also the magnitudes of the terms summed into each group ('mag').  channel_perm / reverse: the same expression in
    another float evaluation order (channels permuted and restored; rays and gates walked last to first)."""
    C, h, w = rendered.shape
    H, W = int(out_hw[0]), int(out_hw[1])
    N, S = gates.shape[0], ray_yx.shape[0]
    perm = torch.arange(C) if channel_perm is None else torch.as_tensor(channel_perm)
    inv = torch.argsort(perm)
    so = torch.arange(S - 1, -1, -1) if reverse else torch.arange(S)
    no = torch.arange(N - 1, -1, -1) if reverse else torch.arange(N)
    r = rendered.detach()[perm].to(dtype).requires_grad_(True)
    gt = gates.detach()[no][:, perm].to(dtype).requires_grad_(True)
    upp = up.detach()[no][:, so][:, :, perm].to(dtype)
    ys, xs = ray_yx[so, 0].long(), ray_yx[so, 1].long()
    y0, y1, ly = taps_f32(H, h)
    x0, x1, lx = taps_f32(W, w)
    y0, y1, x0, x1 = (torch.from_numpy(a)[i] for a, i in ((y0, ys), (y1, ys), (x0, xs), (x1, xs)))
    ly, lx = torch.from_numpy(ly)[ys], torch.from_numpy(lx)[xs]
    if dtype == torch.float32:
        w1y, w0y, w1x, w0x = ly, 1 - ly, lx, 1 - lx                     # 1 - lam rounded to float32, as the kernel does
    else:
        w1y, w0y, w1x, w0x = (a.to(dtype) for a in (ly, 1 - ly.double(), lx, 1 - lx.double()))

    def sample(f):
        top = f[:, y0, x0] * w0x + f[:, y0, x1] * w1x                   # (C, S)
        bot = f[:, y1, x0] * w0x + f[:, y1, x1] * w1x
        return (top * w0y + bot * w1y).transpose(0, 1)                  # (S, C)

    rays = sample(r)
    scaled = rays.unsqueeze(0) * gt.unsqueeze(1)                        # (N, S, C)
    scaled.retain_grad()
    out = torch.nn.functional.normalize(scaled, dim=-1, p=2)
    norm = r.norm(dim=0, p=2).mean()
    d_dense = torch.autograd.grad(norm, r, torch.as_tensor(gn, dtype=dtype), retain_graph=True)[0]
    if S > 0:
        (out * upp).sum().backward()
        d_tap, d_gates = r.grad, gt.grad
    else:
        d_tap, d_gates = torch.zeros_like(r), torch.zeros_like(gt)
    back_n, back_s = torch.argsort(no), torch.argsort(so)
    res = {"out": out.detach()[back_n][:, back_s][:, :, inv].double(), "norm": norm.detach().double(),
           "d_tap": d_tap[inv].double(), "d_gates": d_gates[back_n][:, inv].double(), "d_dense": d_dense[inv].double()}
    if dtype == torch.float64 and channel_perm is None and not reverse:
        with torch.no_grad():
            rd = r.detach()
            absray = sample(rd.abs())                                                           # sum of |tap terms|, (S, C)
            length = scaled.detach().norm(dim=-1).clamp_min(1e-12)                              # (N, S)
            mag = {"out": (absray[None] * gt.detach().abs()[:, None]).amax(dim=-1) / length if S else torch.zeros(N, 0),
                   "norm": float(norm.detach()), "d_dense": abs(float(gn)) / float(h * w)}
            if S > 0:
                dsc = scaled.grad.abs()                                                         # |d (ray * gate)|, (N, S, C)
                mag["d_gates"] = (dsc * rays.detach().abs()[None]).sum(dim=1).amax(dim=-1)      # per gate row (N)
                a = (dsc * gt.detach().abs()[:, None]).sum(dim=0).transpose(0, 1)               # |d ray|, (C, S)
                t = torch.zeros_like(rd)
                for yy, wy in ((y0, w0y), (y1, w1y)):
                    for xx, wx in ((x0, w0x), (x1, w1x)):
                        t.index_put_((torch.arange(C)[:, None], yy[None], xx[None]), a * (wy * wx), accumulate=True)
                mag["d_tap"] = float(t.max())
            else:
                mag["d_gates"], mag["d_tap"] = torch.zeros(N), 0.0
        res["mag"] = mag
    return res


GROUPS = ("out", "norm", "d_tap", "d_gates", "d_dense", "d_both")


def front_end_check(name, product: dict, f64: dict, f32: dict) -> dict:
    """The rule for one run of the front end.  Groups: every out row (n, s, :); the regulariser; the ray-tap part of dL/drendered;
    every dL/dgates row; the dense part of dL/drendered -- and, where the product gives the sum of both parts ('d_both'), that sum
    against the sum of the two parts' bounds.  Prints error / bound per group class, asserts every group, returns the worst."""
    mag = f64["mag"]
    worst, failed = {}, []
    for k in GROUPS:
        if k not in product:
            continue
        if k == "d_both":
            want = f64["d_tap"] + f64["d_dense"]
            b = sum(max(FACTOR * float((f32[p] - f64[p]).abs().max()), FLOOR * mag[p]) for p in ("d_tap", "d_dense"))
            err = float((product[k].double() - want).abs().max())
            r = np.atleast_1d(0.0 if err == 0 else err / max(b, 1e-300))
        else:
            r = ratios(product[k].double().numpy(), f64[k].numpy(), f32[k].numpy(), np.asarray(mag[k]), rows=k in ("out", "d_gates"),
                       floor=OUT_ROW_FLOOR if k == "out" else FLOOR)
        worst[k] = float("nan") if np.isnan(r).any() else float(r.max())
        if not (r <= 1.0).all():
            failed.append(k)
    print(f"{name}: error / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert not failed, (name, failed, worst)
    return worst
