"""Timing of the segmentation queries against the reference's own expressions
(tests/segmentation_ref.py:literal32_*, run on the device unchanged):

  * gui_frame : image 1080 x 1920, C in {32, 64}, Q in {1, 4}: the PCA image (similarity_scores, 3 columns, pre="eps", post=False) and
                the selection (select_by_similarity, pre="eps") against saga_gui.py:590-599, 633, 645-652;
  * segment3d : P = 1 M / C = 32 and 5 M / C = 64, Q in {1, 4}: select_by_similarity against saga_gui.py:674-679;
  * cluster   : the same two point sets and the 1080p image (C = 32), K in {38, 130, 512}: assign_clusters against
                saga_gui.py:526-528, 542-543 on the device (the (N, K) matrix fits there) and, for the points, on the CPU as the
                reference runs it (one run, the .cpu() copies included), and against the notebook's "Cluster in 2D" for the image.

Device events, median of --reps iterations after a warm-up; peak = extra device memory of one iteration.  Each streaming row is
set beside a plain device copy of its feature tensor taken in the same run (copy_ms; new/copy = time per byte read against the
copy's) and its algorithmic bytes / time as a fraction of 8 TB/s; each cluster row with K > 16 gives 2 N K C flops / time.

    python tools/segment_time.py [--reps 10] [--no-cpu] [--out profiles/segment_time.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from seganygaussians_amd import _lib  # noqa: E402
from seganygaussians_amd.segmentation import assign_clusters, select_by_similarity, similarity_scores  # noqa: E402
from tests import segmentation_ref as ref  # noqa: E402

DEV = torch.device("cuda:0")
H, W = 1080, 1920
PEAK_BW = 8.0e12


def timed(fn, reps):
    """(median ms by device events, peak extra MiB of one iteration)."""
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), peak


def cluster_on_device(point_features, gates, cluster_centers):
    """saga_gui.py:526-528, 542-543 with both operands left on the device."""
    scale_conditioned_point_features = torch.nn.functional.normalize(point_features, dim=-1, p=2) * gates.unsqueeze(0)
    normed_point_features = torch.nn.functional.normalize(scale_conditioned_point_features, dim=-1, p=2)
    seg_score = torch.einsum('nc,bc->bn', cluster_centers, normed_point_features)
    return seg_score.argmax(dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "segment_time.py measures on the GPU"
    assert args.reps >= 10
    torch.set_num_threads(16)
    lines = [f"# {_lib.load().mi_rast_version().decode()}; {torch.cuda.get_device_name(0)}; median of {args.reps} iterations after warm-up, "
             f"device events; peak = extra device memory of one iteration; copy = dst.copy_(src) of the feature tensor in the same run; "
             f"of_8TBs = algorithmic bytes / new_ms / 8 TB/s; CPU reference: one run, {torch.get_num_threads()} torch threads",
             "case       layout  N        C    Q/K  ref_ms    ref_peak_MiB  new_ms   new_peak_MiB  speedup  copy_ms  new/copy  of_8TBs  TFLOPs  "
             "ref_cpu_ms"]

    def emit(case, layout, N, C, qk, t_ref, p_ref, t_new, p_new, t_copy, nbytes, flops=None, t_cpu=None):
        line = (f"{case:<10} {layout:<7} {N:<8} {C:<4} {qk:<4} {t_ref:8.3f}  {p_ref:12.0f}  {t_new:7.3f}  {p_new:12.0f}  "
                f"{t_ref / t_new:6.1f}x  {t_copy:7.3f}  {t_new / t_copy:8.2f}  {nbytes / (t_new * 1e-3) / PEAK_BW:7.3f}  "
                f"{'-' if flops is None else format(flops / (t_new * 1e-3) / 1e12, '6.1f'):>6}  "
                f"{'-' if t_cpu is None else format(t_cpu, '10.0f'):>10}")
        print(line, flush=True)
        lines.append(line)

    g = torch.Generator().manual_seed(0)
    sets = {}
    for name, shape, C in (("image", (H, W), 32), ("image", (H, W), 64), ("points", (1_000_000,), 32), ("points", (5_000_000,), 64)):
        feats = (torch.randn((C,) + shape, generator=g) if name == "image" else torch.randn(shape + (C,), generator=g)).to(DEV)
        scratch = torch.empty_like(feats)
        t_copy, _ = timed(lambda: scratch.copy_(feats), args.reps)
        del scratch
        gates = (torch.rand(C, generator=g) * 0.9 + 0.05).to(DEV)
        N = feats.numel() // C
        if name == "image":
            proj = torch.randn(C, 3, generator=g).to(DEV)
            for Q in (1, 4):
                chosen = torch.nn.functional.normalize(torch.randn(Q, C, generator=g), dim=-1).to(DEV)   # (Q, C); the GUI keeps (C, Q)
                chosen_t, proj_t = chosen.t().contiguous(), proj.t().contiguous()
                t_ref, p_ref = timed(lambda: ref.literal32_gui_frame(feats, gates, chosen_t, 0.7, proj_mat=proj), args.reps)

                def new():
                    similarity_scores(feats, proj_t, pre="eps", post=False)
                    select_by_similarity(feats, chosen, 0.7, gates, pre="eps", half_shift=True)
                t_new, p_new = timed(new, args.reps)
                emit("gui_frame", name, N, C, Q, t_ref, p_ref, t_new, p_new, 2 * t_copy, 2 * 4 * N * C + 4 * 3 * N + 5 * N)
        else:
            for Q in (1, 4):
                chosen = torch.nn.functional.normalize(torch.randn(Q, C, generator=g), dim=-1).to(DEV)
                chosen_t = chosen.t().contiguous()
                t_ref, p_ref = timed(lambda: ref.literal32_segment3d(feats, gates, chosen_t, 0.7), args.reps)
                t_new, p_new = timed(lambda: select_by_similarity(feats, chosen, 0.7, gates, pre="none", half_shift=True), args.reps)
                emit("segment3d", name, N, C, Q, t_ref, p_ref, t_new, p_new, t_copy, 4 * N * C + 5 * N)
        sets[(name, C)] = (feats, gates, t_copy, N)
        if (name, C) == ("image", 64):
            del sets[(name, C)]
        del feats
    for (name, C), (feats, gates, t_copy, N) in sets.items():
        for K in (38, 130, 512):
            centers = torch.nn.functional.normalize(torch.randn(K, C, generator=g), dim=-1).to(DEV)
            if name == "image":
                t_ref, p_ref = timed(lambda: ref.literal32_cluster_2d(feats, gates, centers), args.reps)
                t_new, p_new = timed(lambda: assign_clusters(feats, centers, gates, pre="none"), args.reps)
                t_cpu = None
            else:
                t_ref, p_ref = timed(lambda: cluster_on_device(feats, gates, centers), args.reps)
                t_new, p_new = timed(lambda: assign_clusters(feats, centers, gates, pre="l2"), args.reps)
                t_cpu = None
                if not args.no_cpu:
                    t0 = time.perf_counter()
                    ref.literal32_cluster_in_3d(feats, gates, centers)
                    t_cpu = (time.perf_counter() - t0) * 1e3
            emit("cluster", name, N, C, K, t_ref, p_ref, t_new, p_new, t_copy, 4 * N * C + 8 * N, flops=2.0 * N * K * C, t_cpu=t_cpu)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
