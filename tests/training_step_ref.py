"""References of the fused training step (seganygaussians_amd/training_step.py), all on the CPU:

  * adam_restated()      -- the Adam formula as torch.optim.Adam evaluates it (lerp, addcmul, sqrt / bias_correction2_sqrt + eps,
                            addcdiv), dtype-generic; in float64 it is the truth of the GPU tests.
  * torch_adam_step()    -- torch.optim.Adam itself, one step from a given state, in a given dtype: in float32 the yardstick.
  * densify_restated()   -- scene/gaussian_model.py:474-580 (densify_and_prune with densify_and_clone, densify_and_split, N = 2,
                            densification_postfix, cat_tensors_to_optimizer, prune_points, _prune_optimizer) rewritten by hand as one
                            function of tensors; dtype-generic, the normal samples are an argument.
  * densify_case()       -- inputs whose rows fall into chosen classes, every decision quantity away from its threshold.

The tolerance rule is tests/edge_ref.py: ratios (FACTOR 4, FLOOR 2^-22), one group per row."""
from __future__ import annotations

import math

import numpy as np
import torch

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
LOG16 = math.log(1.6)


# ---- Adam --------------------------------------------------------------------------------------------------------------------

def adam_restated(p, g, m, v, step: int, lr: float, beta1: float, beta2: float, eps: float):
    """One step; returns (p, m, v, update magnitude) in the dtype of p.  `step` is the number of this step (1 for the first)."""
    m = m + (g - m) * (1.0 - beta1)
    v = v * beta2 + (1.0 - beta2) * g * g
    step_size = lr / (1.0 - beta1 ** step)
    denom = v.sqrt() / math.sqrt(1.0 - beta2 ** step) + eps
    upd = step_size * (m / denom)
    return p - upd, m, v, upd.abs()


def torch_adam_step(p, g, m, v, step: int, lr: float, beta1: float, beta2: float, eps: float, dtype, cls=torch.optim.Adam):
    """cls (torch.optim.Adam or a subclass) on the CPU in `dtype`: the step number `step` from the state (m, v).  (p, m, v)."""
    q = torch.nn.Parameter(p.detach().to(dtype).clone())
    opt = cls([q], lr=lr, betas=(beta1, beta2), eps=eps)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.detach().to(dtype).clone(), "exp_avg_sq": v.detach().to(dtype).clone()}
    q.grad = g.detach().to(dtype).clone()
    opt.step()
    return q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]


# ---- densify and prune -------------------------------------------------------------------------------------------------------

def f32(x) -> float:
    """A Python number as PyTorch compares it with a float32 tensor: rounded to binary32 once."""
    return float(np.float32(x))


def build_rotation(r):
    """utils/general_utils.py:78-99."""
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3), dtype=r.dtype, device=r.device)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r * z)
    R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y)
    R[:, 2, 1] = 2 * (y * z + r * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def _rep(t, n=2):
    return t.repeat((n,) + (1,) * (t.dim() - 1))


def split_mask(params, accum, denom, max_grad, extent, percent_dense, dtype=torch.float64):
    """The rows densify_and_split selects (of the P originals; a clone row is never selected while max_grad > 0)."""
    g = accum.to(dtype).reshape(-1) / denom.to(dtype).reshape(-1)
    g[g.isnan()] = 0.0
    big = torch.exp(params["scaling"].to(dtype)).max(dim=1).values > f32(percent_dense * extent)
    return (g >= f32(max_grad)) & big


def densify_restated(params: dict, moments: dict, accum, denom, max_grad, min_opacity, extent, percent_dense, max_screen_size, samples,
                     dtype=torch.float64):
    """params: name -> (P, ...) tensor; moments: name -> (exp_avg, exp_avg_sq) or absent; samples: (2 * splits, 3), the draws of
    torch.normal(mean=0, std=exp(scaling[split]).repeat(2, 1)).  Everything is evaluated in `dtype`; thresholds are rounded to
    binary32 once in every dtype.  Returns a dict: 'params', 'moments', 'origin' (source row of every output row), 'kind' (0 original,
    1 clone, 2 first child, 3 second child), 'counts', and for the children rows the magnitudes 'mag_xyz', 'mag_scaling'."""
    T = {k: t.detach().to(dtype) for k, t in params.items()}
    M = {k: tuple(x.detach().to(dtype) for x in mv) for k, mv in moments.items()}
    P, dev = T["xyz"].shape[0], T["xyz"].device          # the CPU in the tests; tools/train_step_time.py times it on the device
    origin, kind = torch.arange(P, device=dev), torch.zeros(P, dtype=torch.long, device=dev)
    mag_xyz, mag_s = torch.zeros(P, dtype=torch.float64, device=dev), torch.zeros(P, dtype=torch.float64, device=dev)

    def postfix(new, new_origin, new_kind, new_mag_xyz, new_mag_s):          # densification_postfix + cat_tensors_to_optimizer
        nonlocal origin, kind, mag_xyz, mag_s
        for k in T:
            if k in M:
                M[k] = tuple(torch.cat((x, torch.zeros_like(new[k])), dim=0) for x in M[k])
            T[k] = torch.cat((T[k], new[k]), dim=0)
        origin, kind = torch.cat((origin, new_origin)), torch.cat((kind, new_kind))
        mag_xyz, mag_s = torch.cat((mag_xyz, new_mag_xyz)), torch.cat((mag_s, new_mag_s))

    def prune(mask):                                                          # prune_points + _prune_optimizer
        nonlocal origin, kind, mag_xyz, mag_s
        keep = ~mask
        for k in T:
            if k in M:
                M[k] = tuple(x[keep] for x in M[k])
            T[k] = T[k][keep]
        origin, kind, mag_xyz, mag_s = origin[keep], kind[keep], mag_xyz[keep], mag_s[keep]

    grads = accum.detach().to(dtype).reshape(-1, 1) / denom.detach().to(dtype).reshape(-1, 1)
    grads[grads.isnan()] = 0.0
    # densify_and_clone
    sel = torch.norm(grads, dim=-1) >= f32(max_grad)
    sel = sel & (torch.exp(T["scaling"]).max(dim=1).values <= f32(percent_dense * extent))
    n_clone = int(sel.sum())
    postfix({k: t[sel] for k, t in T.items()}, origin[sel], torch.ones(n_clone, dtype=torch.long, device=dev), torch.zeros(n_clone, dtype=torch.float64, device=dev),
            torch.zeros(n_clone, dtype=torch.float64, device=dev))
    # densify_and_split
    n_init = T["xyz"].shape[0]
    padded = torch.zeros(n_init, dtype=dtype, device=dev)
    padded[:P] = grads.squeeze(-1)
    sel = padded >= f32(max_grad)
    scal = torch.exp(T["scaling"])
    sel = sel & (scal.max(dim=1).values > f32(percent_dense * extent))
    n_split = int(sel.sum())
    assert not sel[P:].any()
    stds = _rep(scal[sel])
    samples = samples.detach().to(dtype).to(dev)
    assert samples.shape == (stds.shape[0], 3), (samples.shape, stds.shape)
    rots = _rep(build_rotation(T["rotation"][sel]))
    new = {k: _rep(t[sel]) for k, t in T.items()}
    new["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + _rep(T["xyz"][sel])
    new["scaling"] = torch.log(stds / (0.8 * 2))
    m_xyz = (_rep(T["xyz"][sel]).abs().max(dim=1).values + (rots.abs() * samples.abs()[:, None, :]).sum(dim=2).max(dim=1).values).double()
    m_s = (_rep(T["scaling"][sel]).abs().max(dim=1).values + LOG16).double()
    postfix(new, torch.cat((origin[sel], origin[sel])), torch.cat((torch.full((n_split,), 2, device=dev), torch.full((n_split,), 3, device=dev))), m_xyz, m_s)
    prune(torch.cat((sel, torch.zeros(2 * n_split, dtype=torch.bool, device=dev))))
    # the final prune; max_radii2D has been zeroed by densification_postfix
    mask = (torch.sigmoid(T["opacity"]) < f32(min_opacity)).reshape(-1)
    if max_screen_size:
        big_vs = torch.zeros(T["xyz"].shape[0], device=dev) > max_screen_size
        big_ws = torch.exp(T["scaling"]).max(dim=1).values > f32(0.1 * extent)
        mask = mask | big_vs | big_ws
    prune(mask)
    counts = {"clones": n_clone, "splits": n_split, "kept_originals": int((kind == 0).sum()), "kept_clones": int((kind == 1).sum()),
              "kept_children": int((kind == 2).sum())}
    return {"params": T, "moments": M, "origin": origin, "kind": kind, "counts": counts, "mag_xyz": mag_xyz, "mag_scaling": mag_s}


# classes of densify_case(): (selected, size, low opacity, denom == 0).  size: 0 small (clone side), 1 big with children that stay,
# 2 big with children the world-size test deletes
CLASSES = {"kept": (0, 0, 0, 0), "cloned": (1, 0, 0, 0), "split": (1, 1, 0, 0), "split_children_too_big": (1, 2, 0, 0),
           "low_opacity": (0, 0, 1, 0), "too_big": (0, 2, 0, 0), "denom0_nan": (0, 0, 0, 1), "cloned_low_opacity": (1, 0, 1, 0),
           "split_low_opacity": (1, 1, 1, 0), "denom0_inf": (1, 0, 0, 1)}
CLASS_NAMES = tuple(CLASSES)


def densify_case(P: int, sh_degree: int, seed: int, max_grad=0.0002, min_opacity=0.3, extent=8.0, percent_dense=0.0625, classes=None,
                 designated: int = 0):
    """Inputs of P rows (+ `designated` rows with exactly representable activations: s = 0, o = 0, accum / denom = max_grad exactly).
    Row i belongs to class classes[i] (default: the ten CLASSES in turn, starting with 'split', shuffled).  Returns a dict of float32
    CPU tensors: 'params', 'moments', 'accum', 'denom', 'max_radii2D', 'classes'."""
    rng = np.random.default_rng(seed)
    dense, world = percent_dense * extent, 0.1 * extent
    assert 1.1 * dense < 1.5 * world and 1.8 * world > dense
    if classes is None:
        classes = [CLASS_NAMES[(i + 2) % len(CLASS_NAMES)] for i in range(P)]
        classes = [classes[j] for j in rng.permutation(P)]
    spec = np.array([CLASSES[c] for c in classes], np.int64).reshape(P, 4)
    sel, size, low, d0 = spec.T
    u = lambda lo, hi: rng.uniform(lo, hi, P)
    smax = np.where(size == 0, u(0.1, 0.8) * dense, np.where(size == 1, u(1.1 * dense, 1.5 * world), u(1.8, 3.0) * world))
    s = np.log(smax[:, None] * rng.uniform(0.3, 0.9, (P, 3)))
    s[np.arange(P), rng.integers(0, 3, P)] = np.log(smax)
    sig = np.where(low == 1, u(0.2, 0.6) * min_opacity, u(1.2 * min_opacity + 0.02, 0.97))
    o = np.log(sig / (1 - sig))
    den = np.where(d0 == 1, 0, rng.integers(1, 6, P)).astype(np.float64)
    g = np.where(sel == 1, u(1.5, 4.0), u(0.1, 0.7)) * max_grad
    acc = np.where(d0 == 1, np.where(sel == 1, 0.001, 0.0), g * den)
    k = (sh_degree + 1) ** 2
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
    params = {"xyz": t(rng.normal(0, 2, (P, 3))), "f_dc": t(rng.normal(0, 1, (P, 1, 3))), "f_rest": t(rng.normal(0, 0.1, (P, k - 1, 3))),
              "opacity": t(o[:, None]), "scaling": t(s), "rotation": t(rng.normal(0, 1, (P, 4)))}
    accum, denom = t(acc[:, None]), t(den[:, None])
    if designated:
        assert f32(max_grad) == max_grad
        extra = {"xyz": t(rng.normal(0, 2, (designated, 3))), "f_dc": t(rng.normal(0, 1, (designated, 1, 3))),
                 "f_rest": t(rng.normal(0, 0.1, (designated, k - 1, 3))), "opacity": torch.zeros(designated, 1), "scaling": torch.zeros(designated, 3),
                 "rotation": t(rng.normal(0, 1, (designated, 4)))}
        params = {n: torch.cat((params[n], extra[n])) for n in params}
        accum = torch.cat((accum, torch.full((designated, 1), 2 * max_grad)))
        denom = torch.cat((denom, torch.full((designated, 1), 2.0)))
    n = P + designated
    moments = {name: (t(rng.normal(0, 1e-3, tuple(p.shape))), t(rng.uniform(0, 1e-6, tuple(p.shape)))) for name, p in params.items()}
    return {"params": params, "moments": moments, "accum": accum, "denom": denom, "max_radii2D": t(rng.uniform(0, 50, n)),
            "classes": list(classes) + ["designated"] * designated, "designated": designated,
            "args": dict(max_grad=max_grad, min_opacity=min_opacity, extent=extent, percent_dense=percent_dense)}


def decision_margins(case, ulps: float = 16.0):
    """Every decision quantity of every non-designated row, in float64, against its float32-rounded threshold: the smallest
    |q - t| / (ulp of t in binary32).  The tests fail when this is not above `ulps`.  Quantities: accum / denom vs max_grad; max exp(s) vs
    percent_dense extent and vs 0.1 extent; max exp(s) / 1.6 vs 0.1 extent; sigmoid(o) vs min_opacity."""
    a = case["args"]
    n = case["params"]["xyz"].shape[0] - case["designated"]
    s = torch.exp(case["params"]["scaling"][:n].double()).max(dim=1).values
    with np.errstate(all="ignore"):
        g = (case["accum"][:n].double() / case["denom"][:n].double()).reshape(-1)
    g = torch.nan_to_num(g, nan=0.0, posinf=1e30)
    sig = torch.sigmoid(case["params"]["opacity"][:n].double()).reshape(-1)
    worst = float("inf")
    for q, thr in ((g, a["max_grad"]), (s, a["percent_dense"] * a["extent"]), (s, 0.1 * a["extent"]), (s / 1.6, 0.1 * a["extent"]), (sig, a["min_opacity"])):
        thr = f32(thr)
        if q.numel():
            worst = min(worst, float((q - thr).abs().min()) / float(np.spacing(np.float32(thr))))
    return worst
