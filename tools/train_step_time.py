"""Timing of the fused training step at 1 M Gaussians, SH degree 3, every figure from the same run:

  * adam     -- FusedAdam.step() against torch.optim.Adam.step() as scene/gaussian_model.py:187 constructs it (six groups, lr 0,
                eps 1e-15, PyTorch's default implementation for device tensors), and against dst.copy_(src) moving the step's
                algorithmic bytes: 7 x 4 x 59 = 1652 per Gaussian (read p, g, m, v; write p, m, v), half read and half written;
  * stats    -- densification_stats() against train_scene.py:126 + scene/gaussian_model.py:582-584 (five masked index operations);
  * densify  -- densify_and_prune() against the reference method's expression (reference_densify below: the reference's own calls in
                float32 on the device, with both Adam moments), about 5 % of the rows cloned and 5 % split.

Device events, median of --reps (adam, stats) / --densify-reps iterations after a warm-up; peak = extra device memory of one iteration.

    python tools/train_step_time.py [--points 1000000] [--out profiles/train_step_time.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from seganygaussians_amd import _lib  # noqa: E402
from seganygaussians_amd import training_step as ts  # noqa: E402
from tests import training_step_ref as ref  # noqa: E402

DEV = torch.device("cuda:0")
ADAM_BYTES = 7 * 4 * 59
LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 2.5e-3 / 20, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3}


def reference_densify(params, moments, accum, denom, max_grad, min_opacity, extent, percent_dense, max_screen_size):
    """scene/gaussian_model.py:566-578 with the methods it calls (:474-564, :338-373), line for line in float32 on the device of
    the tensors: the reference's own PyTorch calls and host reads, nothing else (no bookkeeping of the tests' restatement)."""
    T = dict(params)
    M = dict(moments)

    def cat(new):                       # densification_postfix -> cat_tensors_to_optimizer
        for k in T:
            M[k] = tuple(torch.cat((x, torch.zeros_like(new[k])), dim=0) for x in M[k])
            T[k] = torch.cat((T[k], new[k]), dim=0)

    def prune(mask):                    # prune_points -> _prune_optimizer
        keep = ~mask
        for k in T:
            M[k] = tuple(x[keep] for x in M[k])
            T[k] = T[k][keep]

    grads = accum / denom
    grads[grads.isnan()] = 0.0
    P = T["xyz"].shape[0]
    sel = torch.where(torch.norm(grads, dim=-1) >= max_grad, True, False)
    sel = torch.logical_and(sel, torch.max(torch.exp(T["scaling"]), dim=1).values <= percent_dense * extent)
    cat({k: t[sel] for k, t in T.items()})
    padded = torch.zeros((T["xyz"].shape[0]), device=DEV)
    padded[:P] = grads.squeeze()
    sel = torch.where(padded >= max_grad, True, False)
    sel = torch.logical_and(sel, torch.max(torch.exp(T["scaling"]), dim=1).values > percent_dense * extent)
    stds = torch.exp(T["scaling"])[sel].repeat(2, 1)
    samples = torch.normal(mean=torch.zeros((stds.size(0), 3), device=DEV), std=stds)
    rots = ref.build_rotation(T["rotation"][sel]).repeat(2, 1, 1)
    new = {k: t[sel].repeat((2,) + (1,) * (t.dim() - 1)) for k, t in T.items()}
    new["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + T["xyz"][sel].repeat(2, 1)
    new["scaling"] = torch.log(torch.exp(T["scaling"])[sel].repeat(2, 1) / (0.8 * 2))
    cat(new)
    prune(torch.cat((sel, torch.zeros(2 * sel.sum(), device=DEV, dtype=bool))))
    mask = (torch.sigmoid(T["opacity"]) < min_opacity).squeeze()
    if max_screen_size:
        big_vs = torch.zeros(T["xyz"].shape[0], device=DEV) > max_screen_size        # max_radii2D, zeroed by densification_postfix
        big_ws = torch.exp(T["scaling"]).max(dim=1).values > 0.1 * extent
        mask = torch.logical_or(torch.logical_or(mask, big_vs), big_ws)
    prune(mask)
    return T, M


def timed(fn, reps, setup=None):
    """(median ms by device events, peak extra MiB of one iteration); setup() runs before every iteration, outside the events."""
    def once():
        state = setup() if setup else None
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        e0.record()
        out = fn(state) if setup else fn()
        e1.record()
        torch.cuda.synchronize()
        peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        del out, state
        return e0.elapsed_time(e1), peak
    once()
    runs = [once() for _ in range(reps)]
    return statistics.median(t for t, _ in runs), max(p for _, p in runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--densify-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "train_step_time.py measures on the GPU"
    P = args.points
    lines = [f"# {_lib.load().mi_rast_version().decode()}; {torch.cuda.get_device_name(0)}; {P} Gaussians, SH degree 3 (59 floats each); median of "
             f"{args.reps} (adam, stats) / {args.densify_reps} (densify) iterations after warm-up, device events; peak = extra device memory of one "
             f"iteration; ref = torch.optim.Adam as scene/gaussian_model.py:187 builds it / the reference's five statistics lines / the reference's "
             f"densify_and_prune calls in float32 on the device with both moments; copy = dst.copy_(src) moving {ADAM_BYTES} bytes per Gaussian (half read, half written) "
             f"in the same run",
             "stage     ref_ms    ref_peak_MiB  new_ms    new_peak_MiB  ref/new  copy_ms  new/copy  rows_out"]

    def report(stage, t_ref, p_ref, t_new, p_new, t_copy=None, rows=""):
        copy = f"{t_copy:7.3f}  {t_new / t_copy:8.2f}" if t_copy else f"{'-':>7}  {'-':>8}"
        line = f"{stage:<8} {t_ref:8.3f}  {p_ref:12.0f}  {t_new:8.3f}  {p_new:12.0f}  {t_ref / t_new:6.1f}x  {copy}  {rows}"
        print(line, flush=True)
        lines.append(line)

    # ---- Adam
    gen = torch.Generator().manual_seed(0)
    shapes = {"xyz": (P, 3), "f_dc": (P, 1, 3), "f_rest": (P, 15, 3), "opacity": (P, 1), "scaling": (P, 3), "rotation": (P, 4)}
    grads = {k: torch.randn(s, generator=gen).to(DEV) for k, s in shapes.items()}

    def optimizer(cls):
        params = {k: torch.nn.Parameter(torch.randn(s, generator=torch.Generator().manual_seed(1)).to(DEV)) for k, s in shapes.items()}
        for k, q in params.items():
            q.grad = grads[k]
        return cls([{"params": [params[k]], "lr": LRS[k], "name": k} for k in shapes], lr=0.0, eps=1e-15)

    src = torch.empty(ADAM_BYTES * P // 8, device=DEV, dtype=torch.float32)
    dst = torch.empty_like(src)
    t_copy, _ = timed(lambda: dst.copy_(src), args.reps)
    del src, dst
    old, new = optimizer(torch.optim.Adam), optimizer(ts.FusedAdam)
    t_ref, p_ref = timed(old.step, args.reps)
    t_new, p_new = timed(new.step, args.reps)
    report("adam", t_ref, p_ref, t_new, p_new, t_copy)
    del old, new

    # ---- statistics
    radii = torch.where(torch.rand(P, generator=gen) < 0.6, torch.randint(1, 40, (P,), generator=gen), torch.zeros(P, dtype=torch.long)).to(torch.int32).to(DEV)
    vgrad = torch.randn(P, 3, generator=gen).to(DEV)
    accum, denom, max_r = torch.zeros(P, 1, device=DEV), torch.zeros(P, 1, device=DEV), torch.zeros(P, device=DEV)

    def ref_stats():
        vis = radii > 0
        max_r[vis] = torch.max(max_r[vis], radii[vis])
        accum[vis] += torch.norm(vgrad[vis, :2], dim=-1, keepdim=True)
        denom[vis] += 1

    t_ref, p_ref = timed(ref_stats, args.reps)
    t_new, p_new = timed(lambda: ts.densification_stats(accum, denom, vgrad, radii, max_r), args.reps)
    report("stats", t_ref, p_ref, t_new, p_new)

    # ---- densify and prune: 5 % cloned, 5 % split, the rest kept
    classes = ["cloned" if i % 20 == 0 else "split" if i % 20 == 1 else "kept" for i in range(P)]
    case = ref.densify_case(P, 3, 0, classes=classes)
    a = case["args"]
    cp = {k: t.to(DEV) for k, t in case["params"].items()}
    cm = {k: (m.to(DEV), v.to(DEV)) for k, (m, v) in case["moments"].items()}
    c_accum, c_denom, c_max = (case[k].to(DEV) for k in ("accum", "denom", "max_radii2D"))
    n_split = classes.count("split")
    rows = []

    def ref_densify():
        return reference_densify(cp, cm, c_accum, c_denom, a["max_grad"], a["min_opacity"], a["extent"], a["percent_dense"], 20)

    def new_setup():
        params = {k: torch.nn.Parameter(t) for k, t in cp.items()}
        opt = ts.FusedAdam([{"params": [params[k]], "lr": LRS[k], "name": k} for k in params], lr=0.0, eps=1e-15)
        for k, q in params.items():
            opt.state[q] = {"step": torch.tensor(3.0), "exp_avg": cm[k][0], "exp_avg_sq": cm[k][1]}
        return params, opt

    def new_densify(state):
        out = ts.densify_and_prune(state[0], state[1], c_accum, c_denom, c_max, a["max_grad"], a["min_opacity"], a["extent"], a["percent_dense"], 20)
        rows.append(out[0]["xyz"].shape[0])
        return out

    t_ref, p_ref = timed(ref_densify, args.densify_reps)
    t_new, p_new = timed(new_densify, args.densify_reps, setup=new_setup)
    report("densify", t_ref, p_ref, t_new, p_new, rows=f"{rows[-1]} ({classes.count('cloned')} clones, {n_split} splits)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
