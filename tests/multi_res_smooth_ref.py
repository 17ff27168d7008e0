"""Binary64 restatement of the multi-resolution feature smoothing, the yardstick of tests/test_multi_res_smooth*.py:

    n_j        = F_j / max(|F_j|, 1e-12)                            (torch.nn.functional.normalize, p = 2)
    mean_{l,i} = (1/k_l) * sum_s n[ sub_l[ idx_l[i][s] ] ]          sub_l = nonzero(pm_l)
    ret_i      = sum_l w[i,l] * mean_{l,i}                          w = 1 when absent; (P, L) or one shared row (1, L)
    out_i      = ret_i / (|ret_i| + 1e-9)                           only with normalize_out

(FeatureGaussianModel.get_multi_resolution_smoothed_point_features, scene/gaussian_model_ff.py:391-400, and the renderer's
norm_point_features, gaussian_renderer/__init__.py:362-363; pinned to the reference's own method by the fixture
tests/golden/multi_res_smooth/multi_res_smooth.npz).  Gradients come from autograd.  Runs anywhere: CPU, float64."""
import numpy as np
import torch


def _f64(a, requires_grad=False):
    t = torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a), dtype=torch.float64).clone()
    return t.requires_grad_(requires_grad)


def expression(f, levels, w, normalize_out, channel_perm=None, reverse=False):
    """The expression itself on torch tensors `f` (P, C) and `w` (None, (P, L) or (1, L)) of one dtype, written the way the
    reference writes it (so that it also serves, in float32, as the measure of the reference's own rounding noise).
    channel_perm / reverse give the same expression another float evaluation order, forward and (through autograd) backward:
    the channels permuted before and restored after; the levels walked, and each level's columns gathered, last to first."""
    if channel_perm is not None:
        perm = torch.as_tensor(np.asarray(channel_perm), dtype=torch.int64)
        f = f[:, perm]
    normed = torch.nn.functional.normalize(f, dim=-1, p=2)
    ret = torch.zeros_like(normed)
    order = range(len(levels) - 1, -1, -1) if reverse else range(len(levels))
    for l in order:
        pm, idx = levels[l]
        pm = torch.as_tensor(np.asarray(pm), dtype=torch.bool)
        idx = torch.as_tensor(np.asarray(idx), dtype=torch.int64)
        if reverse:
            idx = idx.flip(1)
        sw = w[:, l:l + 1] if w is not None else 1
        ret = ret + sw * normed[pm][idx, :].mean(dim=1)
    if normalize_out:
        ret = ret / (ret.norm(dim=1, keepdim=True) + 1e-9)
    if channel_perm is not None:
        ret = ret[:, torch.argsort(perm)]
    return ret


def float32_expression(F, levels, w, normalize_out, grad_out, channel_perm=None, reverse=False):
    """(out, dL/dF, dL/dw or None) of `expression` in float32 torch on the CPU, as float64 numpy arrays: the yardstick E32 of
    tests/edge_ref.py, and with channel_perm / reverse the alternative evaluation orders that confirm its floors."""
    f = torch.as_tensor(np.asarray(F), dtype=torch.float32).clone().requires_grad_(True)
    wt = None if w is None else torch.as_tensor(np.asarray(w), dtype=torch.float32).clone().requires_grad_(True)
    out = expression(f, levels, wt, normalize_out, channel_perm, reverse)
    out.backward(torch.as_tensor(np.asarray(grad_out), dtype=torch.float32))
    return (out.detach().double().numpy(), f.grad.double().numpy(), None if wt is None else wt.grad.double().numpy())


def make_levels(xyz, masks, Ks):
    """[(point_mask, idx (P, k) into xyz[point_mask])]: every point's k nearest members of the subset by exhaustive search in
    float64, nearest first.  A subset of fewer than k points (possible only in a hand-built map: the search itself refuses it) is
    cycled through, nearest first, so that every column is a valid member."""
    x = torch.as_tensor(np.asarray(xyz), dtype=torch.float64)
    levels = []
    for pm, k in zip(masks, Ks):
        pm = np.asarray(pm, dtype=bool)
        order = torch.cdist(x, x[torch.as_tensor(pm)]).argsort(dim=1, stable=True).numpy()
        levels.append((pm, order[:, np.arange(k) % order.shape[1]].astype(np.int64)))
    return levels


def make_case(P, C, Ks, rates=None, counts=None, seed=0, zero_rows=()):
    """Seeded inputs of one test: xyz, features of mixed row norms (rows `zero_rows` all zero), the upstream gradient, and the
    levels: level l's subset is a `rand < rates[l]` draw, or exactly counts[l] random points where counts[l] is given; never
    empty."""
    rng = np.random.default_rng(seed)
    xyz = rng.normal(size=(P, 3)).astype(np.float32)
    F = (rng.normal(size=(P, C)) * rng.uniform(0.1, 3.0, size=(P, 1))).astype(np.float32)
    F[list(zero_rows)] = 0.0
    g = rng.normal(size=(P, C)).astype(np.float32)
    masks = []
    for l, k in enumerate(Ks):
        if counts is not None and counts[l] is not None:
            pm = np.zeros(P, dtype=bool)
            pm[rng.choice(P, size=counts[l], replace=False)] = True
        else:
            pm = rng.uniform(size=P) < rates[l]
            if not pm.any():
                pm[rng.integers(P)] = True
        masks.append(pm)
    return xyz, F, g, make_levels(xyz, masks, Ks)


def make_weights(kind, P, L, seed=0):
    """None; "full": (P, L) with negatives and (L > 1) zeros among them, no row all zero (that row has a test of its own: its
    gradients are of the order 1/1e-9 under normalize_out and would set the scale of the whole comparison); "row": one shared
    row (1, L)."""
    if kind is None:
        return None
    rng = np.random.default_rng(1000 + seed)
    w = rng.normal(size=(P if kind == "full" else 1, L)).astype(np.float32)
    if kind == "full" and L > 1:
        w[rng.uniform(size=w.shape) < 0.1] = 0.0
        w[~w.any(axis=1), 0] = -0.75
    return w


def dw_term_scale(F, levels, w, normalize_out, grad_out):
    """max over the levels of |dL/dret_i| * |mean_{l,i}| (summed over i for one shared row of weights): the Cauchy-Schwarz bound
    of the dot products that dL/dw consists of.  The scale of dL/dw's rounding error where dL/dw itself cancels to (nearly) zero:
    under normalize_out the output does not change when the weights of a row are scaled together, so sum_l w_l dL/dw_l = 0, and
    with parallel level means (one level, or a cloud of one point) every dL/dw_l is 0 up to the 1e-9 of the denominator."""
    f, wt = _f64(F), None if w is None else _f64(w)
    normed = torch.nn.functional.normalize(f, dim=-1, p=2)
    means = [normed[torch.as_tensor(np.asarray(pm), dtype=torch.bool)][torch.as_tensor(np.asarray(idx), dtype=torch.int64), :].mean(dim=1)
             for pm, idx in levels]
    ret = sum((wt[:, l:l + 1] if wt is not None else 1) * m for l, m in enumerate(means)).requires_grad_(True)
    out = ret / (ret.norm(dim=1, keepdim=True) + 1e-9) if normalize_out else ret * 1
    out.backward(_f64(grad_out))
    terms = torch.stack([ret.grad.norm(dim=1) * m.norm(dim=1) for m in means], dim=1)      # (P, L)
    if wt is not None and wt.shape[0] == 1:
        terms = terms.sum(dim=0, keepdim=True)
    return float(terms.max())


def fp32_reference_error(F, levels, w, normalize_out, grad_out, want):
    """The reference expression evaluated in float32 torch on the CPU against `want` = forward_backward(...) of the same inputs:
    max |error| / max |want| of out, dL/dF and dL/dw (None without weights) -- the rounding noise of the reference itself."""
    got = float32_expression(F, levels, w, normalize_out, grad_out)
    return tuple(None if b is None else float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(got, want))


def forward_backward(F, levels, w, normalize_out, grad_out):
    """(out, dL/dF, dL/dw or None) as float64 numpy arrays; levels = [(point_mask (P,), idx (P, k_l) into the subset), ...]."""
    f = _f64(F, True)
    wt = None if w is None else _f64(w, True)
    out = expression(f, levels, wt, normalize_out)
    out.backward(_f64(grad_out))
    return out.detach().numpy(), f.grad.numpy(), None if wt is None else wt.grad.numpy()
