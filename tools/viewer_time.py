"""Timing of the viewer frame at 1080p and of the feature moments behind the PCA basis.

  * frame   : C in {32, 64}, Q in {none, 1, 4}, every non-empty set of the GUI's four render modes (no mode shows what "rgb" shows);
              cluster_rgb is given whenever "cluster" is on.  Per row:
                ref_ms  the reference's own lines on the device (tests/viewer_ref.py:literal32_fetch_data: saga_gui.py:584-599,
                        630-659, 701-724 unchanged, its .cpu().numpy() copies, np.interp colour map and numpy averaging included);
                sep_ms  the separate-call form available before viewer_frame existed: select_by_similarity, similarity_scores(post=False)
                        and torch operations for the clip, the colour map and the average, each only when its mode asks for it;
                new_ms  viewer_frame;
                copy_ms dst.copy_(src) of the feature tensor in the same run.
  * moments : 200 000 sampled rows of a 1 M x 32 table (do_pca) and all rows of 5 M x 64.  ref_ms is saga_gui.py:549-551, 562-567 on
              the device (clone, normalise every row, gather, mean, matmul; the eigen-decomposition is outside both columns);
              new_ms is feature_covariance; there is no separate-call form.

Device events, median of --reps iterations after a warm-up (--ref-reps for the reference's chain, which the host bounds).
of_8TBs = algorithmic bytes / new_ms / 8 TB/s.

    python tools/viewer_time.py [--reps 20] [--ref-reps 3] [--out profiles/viewer_time.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from seganygaussians_amd import _lib  # noqa: E402
from seganygaussians_amd.segmentation import select_by_similarity, similarity_scores  # noqa: E402
from seganygaussians_amd.viewer import feature_covariance, gui_pca_sample, viewer_frame  # noqa: E402
from tests import viewer_ref as vr  # noqa: E402

DEV = torch.device("cuda:0")
H, W = 1080, 1920
PEAK_BW = 8.0e12


def timed(fn, reps):
    """Median ms by device events; the host's share of fn is inside the interval."""
    fn()
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


def jet_torch(score):
    """The colour map as torch operations on the device: (H, W) -> (H, W, 3)."""
    x = score.clamp(0.0, 1.0) * 8
    r = ((x - 3) * 0.5).clamp(0, 1) - ((x - 7) * 0.5).clamp(0, 0.5)
    g = ((x - 1) * 0.5).clamp(0, 1) - ((x - 5) * 0.5).clamp(0, 1)
    b = (x * 0.5 + 0.5).clamp(0.5, 1) - ((x - 3) * 0.5).clamp(0, 1)
    return torch.stack((r, g, b), dim=-1)


def separate_calls(feats, rgb, proj_t, queries, gates, thr, cluster, modes):
    img = rgb.permute(1, 2, 0)
    mask = score = None
    if queries is not None:
        mask, score = select_by_similarity(feats, queries, thr, gates, pre="eps", half_shift=True)
    comps = []
    if "rgb" in modes:
        comps.append(img)
    if "pca" in modes:
        p = similarity_scores(feats, proj_t, pre="eps", post=False)
        comps.append(torch.clip(p.permute(1, 2, 0) * 0.5 + 0.5, 0, 1))
    if "cluster" in modes:
        comps.append(img if cluster is None else cluster.permute(1, 2, 0))
    if "similarity" in modes:
        comps.append(img if score is None else jet_torch(score))
    buf = comps[0]
    for c in comps[1:]:
        buf = buf + c
    return (buf / len(comps)).contiguous(), mask, score


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ref-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "viewer_time.py measures on the GPU"
    assert args.reps >= 10
    torch.set_num_threads(16)
    lines = [f"# {_lib.load().mi_rast_version().decode()}; {torch.cuda.get_device_name(0)}; median of {args.reps} iterations after warm-up "
             f"({args.ref_reps} for ref_ms), device events; ref = the reference's lines on the device with their host copies and numpy "
             f"colour map, {torch.get_num_threads()} torch threads; sep = select_by_similarity + similarity_scores(post=False) + torch "
             f"operations; new = viewer_frame / feature_covariance; copy = dst.copy_(src) of the feature tensor in the same run; "
             f"of_8TBs = algorithmic bytes / new_ms / 8 TB/s",
             "case     N        C    Q     modes                       ref_ms    sep_ms   new_ms  sep/new  copy_ms  new/copy  of_8TBs"]

    def emit(case, N, C, Q, modes, t_ref, t_sep, t_new, t_copy, nbytes):
        sep = "-" if t_sep is None else format(t_sep, "8.3f")
        ratio = "-" if t_sep is None else format(t_sep / t_new, "6.2f") + "x"
        line = (f"{case:<8} {N:<8} {C:<4} {Q:<5} {modes:<26} {t_ref:8.3f}  {sep:>8}  {t_new:7.3f}  {ratio:>7}  {t_copy:7.3f}  "
                f"{t_new / t_copy:8.2f}  {nbytes / (t_new * 1e-3) / PEAK_BW:7.3f}")
        print(line, flush=True)
        lines.append(line)

    g = torch.Generator().manual_seed(0)
    N = H * W
    rgb = torch.rand(3, H, W, generator=g).to(DEV)
    cluster = torch.rand(3, H, W, generator=g).to(DEV)
    out = torch.empty(H, W, 3, device=DEV)
    for C in (32, 64):
        feats = torch.randn(C, H, W, generator=g).to(DEV)
        scratch = torch.empty_like(feats)
        t_copy = timed(lambda: scratch.copy_(feats), args.reps)
        del scratch
        gates = (torch.rand(C, generator=g) * 0.9 + 0.05).to(DEV)
        proj = torch.linalg.qr(torch.randn(C, 3, generator=g))[0].contiguous().to(DEV)
        proj_t = proj.t().contiguous()
        for Q in (0, 1, 4):
            queries = torch.nn.functional.normalize(torch.randn(Q, C, generator=g), dim=-1).to(DEV) if Q else None
            chosen_t = None if queries is None else queries.t().contiguous()
            for modes in vr.ALL_MODE_SUBSETS[1:]:
                clu = cluster if "cluster" in modes else None
                t_ref = timed(lambda: vr.literal32_fetch_data(feats, rgb, proj, gates, chosen_t, 0.7,
                                                              None if clu is None else clu.permute(1, 2, 0), modes, False), args.ref_reps)
                t_sep = timed(lambda: separate_calls(feats, rgb, proj_t, queries, gates, 0.7, clu, modes), args.reps)
                t_new = timed(lambda: viewer_frame(feats, rgb, proj=proj, queries=queries, gates=gates, threshold=0.7, cluster_rgb=clu,
                                                   modes=modes, out=out), args.reps)
                read = (C if (Q or "pca" in modes) else 0) + (6 if clu is not None else 3)
                emit("frame", N, C, Q if Q else "none", "+".join(modes), t_ref, t_sep, t_new, t_copy, 4 * N * read + 12 * N + (5 * N if Q else 0))
        del feats

    def reference_moments(table, index):
        sems = table.clone()                                                                  # saga_gui.py:562
        sems /= (torch.norm(sems, dim=1, keepdim=True) + 1e-6)                                # :566
        X = sems if index is None else sems[index, :]                                         # :567
        n = X.shape[0]                                                                        # :548
        mean = torch.mean(X, dim=0)                                                           # :549
        X = X - mean                                                                          # :550
        return (1 / n) * torch.matmul(X.T, X).float()                                         # :551

    for P, C, sample in ((1_000_000, 32, 200_000), (5_000_000, 64, None)):
        table = torch.randn(P, C, generator=g).to(DEV)
        scratch = torch.empty_like(table)
        t_copy = timed(lambda: scratch.copy_(table), args.reps)
        del scratch
        index = None if sample is None else gui_pca_sample(P, sample).to(DEV)
        n = P if sample is None else sample
        t_ref = timed(lambda: reference_moments(table, index), args.reps)
        t_new = timed(lambda: feature_covariance(table, index, pre="eps"), args.reps)
        emit("moments", n, C, "-", "all rows" if sample is None else f"sampled of {P}", t_ref, None, t_new, t_copy,
             4 * n * C + (8 * n if sample else 0))
        del table
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
