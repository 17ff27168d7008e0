"""Timing of the 2D-to-3D score lifting on the cfg2 scene (1 M Gaussians, 1920 x 1080), against the two ways
the same numbers could be had before it, on the same build:

  * lift        : lifting.lift_scores with K = 1, 3, 16 score channels, front half (preprocess, binning, per-tile sort) included;
  * lift_reuse  : the same with state= (the lift kernel alone over the buffers of an earlier lift, accumulating into `out`);
  * mask_pair   : K = 1 as mi_rast_mask_forward + mi_rast_mask_backward with dL_dout_mask = the score image;
  * rgb_fwd_bwd : the reference's route (clip_utils/__init__.py:291-330): the 3-channel forward of the mask repeated to three
                  colours + the default backward (blend and geometry) with dL_dpixels = the score image in all three channels.

Device events, median of --reps iterations after a warm-up.  Also: the per-stage times of one K = 1 lift (library events), and the
rows of atomics the lift kernel issues -- (half tile, record) pairs among the entries the forward walks -- against its time.

    python tools/lift_time.py [--reps 20] [--out profiles/lift_time.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from seganygaussians_amd import _lib, lifting  # noqa: E402
from seganygaussians_amd import rasterizer as R  # noqa: E402
from tests import helpers as hp  # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def atomic_rows(g):
    """(entries, half-tile rows, whole-tile rows) among the list entries a forward walks (tile_nsurv of an expf forward): what the
    lift kernel turns into rows of atomics with a wave per half tile / per tile."""
    fw = hp.GpuRun(g.inp).forward(full_lists=False, exact_exp=True)
    im = fw.img_fields()
    ranges = torch.as_tensor(im["ranges"].reshape(-1, 2).astype(np.int64)).to(DEV)
    nsurv = torch.as_tensor(im["tile_nsurv"].astype(np.int64)).to(DEV)
    lens = ranges[:, 1] - ranges[:, 0]
    _, off = _lib.binning_layout(fw.num_rendered)
    n = int(lens.sum())
    bl = fw.binning[off["blend_list"]:off["blend_list"] + 4 * fw.num_rendered].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    tile = torch.repeat_interleave(torch.arange(len(lens), device=DEV), lens)
    pos = torch.arange(n, device=DEV) - torch.repeat_interleave(torch.cumsum(lens, 0) - lens, lens)   # position in its tile's list
    walked = pos < nsurv[tile]
    e = bl[(ranges[tile, 0] + pos)[walked]]
    m = e >> 28
    upper, lower = (m & 3) != 0, (m & 12) != 0
    return int(walked.sum()), int(upper.sum() + lower.sum()), int((m != 0).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "lift_time.py measures on the GPU"
    assert args.reps >= 10
    inp = hp.inputs_from_config(args.config)
    g = hp.GpuRun(inp)
    H, W, P = inp.image_height, inp.image_width, g.P
    geo = dict(scales=g.scales, rotations=g.rots, viewmatrix=g.view, projmatrix=g.proj, tanfovx=inp.tanfovx, tanfovy=inp.tanfovy)
    gen = torch.Generator().manual_seed(0)
    scores = torch.rand((16, H, W), generator=gen).to(DEV)
    lines = [f"# {_lib.load().mi_rast_version().decode()}; {torch.cuda.get_device_name(0)}; {args.config}: P = {P}, {W} x {H}; median of "
             f"{args.reps} iterations after warm-up, device events, product flags (lean lists)",
             "case          K    ms"]

    def emit(case, K, ms):
        line = f"{case:<13} {K:<4} {ms:8.3f}"
        print(line, flush=True)
        lines.append(line)
        return ms

    for _ in range(50):   # clocks and allocator in steady state before the first timed case
        lifting.lift_scores(scores[:1].contiguous(), g.means3D, g.opac, **geo)
    t_lift, t_reuse = {}, {}
    for K in (1, 3, 16):
        s = scores[:K].contiguous()
        t_lift[K] = emit("lift", K, timed(lambda: lifting.lift_scores(s, g.means3D, g.opac, **geo), args.reps))
        _, st = lifting.lift_scores(s, g.means3D, g.opac, return_state=True, **geo)
        acc = torch.zeros((P, K), device=DEV)
        t_reuse[K] = emit("lift_reuse", K, timed(lambda: lifting.lift_scores(s, g.means3D, g.opac, state=st, out=acc), args.reps))

    target = scores[:1].contiguous()
    mask_vals = torch.zeros(P, device=DEV)

    def mask_pair():
        nr, _, _, geom, binning, img = R.rasterize_mask_gaussians_native(
            g.means3D, g.opac, mask_vals, g.scales, g.rots, 1.0, g.cov, g.view, g.proj, inp.tanfovx, inp.tanfovy, H, W, False, False)
        return R.rasterize_mask_gaussians_backward_native(g.means3D, target, geom, nr, binning, img, False)
    t_pair = emit("mask_pair", 1, timed(mask_pair, args.reps))

    colors = torch.zeros((P, 3), device=DEV)
    target3 = target.repeat(3, 1, 1).contiguous()
    bg = torch.zeros(3, device=DEV)
    empty = torch.empty(0)

    def rgb_fwd_bwd():
        nr, _, radii, geom, binning, img = R.rasterize_gaussians_native(
            3, False, bg, g.means3D, colors, g.opac, empty, g.scales, g.rots, 1.0, g.cov, g.view, g.proj, inp.tanfovx, inp.tanfovy,
            H, W, empty, 0, g.campos, False, False)
        return R.rasterize_gaussians_backward_native(
            3, False, bg, g.means3D, radii, colors, g.scales, g.rots, 1.0, g.cov, g.view, g.proj, inp.tanfovx, inp.tanfovy, target3,
            None, empty, 0, g.campos, geom, nr, binning, img, False)
    t_rgb = emit("rgb_fwd_bwd", 3, timed(rgb_fwd_bwd, args.reps))

    _lib.profile_enable(True)
    lifting.lift_scores(target, g.means3D, g.opac, **geo)
    stages = _lib.profile_read()
    _lib.profile_enable(False)
    front = sum(stages[k] for k in ("preprocess", "tile_scan", "emit", "tile_sort"))
    entries, half_rows, tile_rows = atomic_rows(g)
    tail = [
        f"# mask_pair / lift (K = 1): {t_pair / t_lift[1]:.2f}x    rgb_fwd_bwd / lift (K = 1): {t_rgb / t_lift[1]:.2f}x    "
        f"rgb_fwd_bwd / lift (K = 3): {t_rgb / t_lift[3]:.2f}x",
        f"# stages of one K = 1 lift (library events, ms): front half {front:.3f} (" +
        ", ".join(f"{k} {stages[k]:.3f}" for k in ("preprocess", "tile_scan", "emit", "tile_sort")) + f"), lift kernel {stages['blend_fwd']:.3f}",
        f"# walked list entries {entries}; rows of atomics: {half_rows} per half tile ({half_rows / max(entries, 1):.2f} per (tile, record)), "
        f"{tile_rows} per whole tile",
    ] + [f"# K = {K}: {half_rows / (t_reuse[K] * 1e-3) / 1e9:.2f} G rows/s over the lift_reuse time" for K in (1, 3, 16)]
    if t_pair / t_lift[1] < 1.0:
        tail.append(f"# K = 1 lift is SLOWER than the mask-only pair: front half {front:.3f} ms, walk + atomics {stages['blend_fwd']:.3f} ms "
                    f"(atomics alone at 15 G rows/s: {half_rows / 15e9 * 1e3:.3f} ms)")
    for line in tail:
        print(line, flush=True)
    lines += tail
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
