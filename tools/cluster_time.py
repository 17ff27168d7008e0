"""Timing of the HDBSCAN* clustering, every figure from the same run:

  * core_ms    -- mi_cluster_core_distances, device events;
  * mst_ms     -- mi_cluster_mst, host clock around the call and a synchronise (the call itself reads 4 bytes per Boruvka round);
                  rounds, and ms_per_round = mst_ms / rounds;
  * tree_ms    -- labels_from_mst on the host (C++), host clock, edges already on the host;
  * total_ms   -- hdbscan_labels end to end (upload excluded, the download of the tree and the upload of the labels included);
  * sklearn_s  -- sklearn.cluster.HDBSCAN.fit_predict on the same rows (CPU, wall clock, one run) where scikit-learn is importable
                  and n <= 20000; "-" otherwise.

Shapes: the planted generator of tests/hdbscan_ref.py at n = 16384, 20000, 51565 x C = 32 (min_cluster_size 10, epsilon 0.01) and
planted bit sets at n = 8192 x 1024 bits (min_cluster_size 30, epsilon 0.25).  Median of --reps runs after one warm-up run.

    python tools/cluster_time.py [--reps 5] [--out profiles/cluster_time.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from seganygaussians_amd import _lib  # noqa: E402
from seganygaussians_amd import clustering as cl  # noqa: E402
from tests import hdbscan_ref as ref  # noqa: E402

DEV = torch.device("cuda:0")
CASES = [("euclidean", 16384, 32, 10, 0.01), ("euclidean", 20000, 32, 10, 0.01), ("euclidean", 51565, 32, 10, 0.01),
         ("jaccard", 8192, 32, 30, 0.25)]


def median_ms(fn, reps, device_events):
    out = []
    for it in range(reps + 1):
        torch.cuda.synchronize()
        if device_events:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1)
        else:
            h0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - h0) * 1e3
        if it:
            out.append(ms)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cluster_time.py needs a GPU: nothing here is measured without one")
    L = _lib.load()
    try:
        from sklearn.cluster import HDBSCAN as SkHDBSCAN
    except ImportError:
        SkHDBSCAN = None
    lines = [f"# {L.mi_rast_version().decode()}; {torch.cuda.get_device_name(0)}; every figure measured in this run: median of {args.reps} runs after one "
             "warm-up; core_ms device events, mst_ms / tree_ms / total_ms host clock ending in a synchronise; sklearn_s one CPU run "
             "'-' = not measured",
             f"{'metric':<10}{'n':>7}{'width':>6}{'mcs':>5}{'core_ms':>9}{'mst_ms':>9}{'rounds':>7}{'ms_per_round':>13}{'tree_ms':>9}"
             f"{'total_ms':>10}{'clusters':>9}{'noise':>7}{'sklearn_s':>10}"]
    for metric, n, width, mcs, eps in CASES:
        pts = ref.planted(n, width, 8, seed=0) if metric == "euclidean" else ref.planted_bits(n, 8, seed=0, bits=32 * width)
        x = torch.from_numpy(pts.view(np.int32) if pts.dtype == np.uint32 else pts).to(DEV)
        x, mid, n, width = cl._prepare("cluster_time", x, mcs, metric)
        ws, nbytes = cl._workspace(L, mid, n, width, mcs, DEV)
        core = cl._core(L, x, mid, n, width, mcs, ws, nbytes)
        core_ms = median_ms(lambda: cl._core(L, x, mid, n, width, mcs, ws, nbytes), args.reps, True)
        mst_ms = median_ms(lambda: cl._mst(L, x, mid, n, width, core, ws, nbytes), args.reps, False)
        rounds = L.mi_cluster_mst_rounds()
        ea, eb, ew = (t.cpu() for t in cl._mst(L, x, mid, n, width, core, ws, nbytes))
        tree_ms = median_ms(lambda: cl.labels_from_mst(ea, eb, ew, n, mcs, eps), args.reps, False)
        total_ms = median_ms(lambda: cl.hdbscan_labels(x, mcs, cluster_selection_epsilon=eps, metric=metric), args.reps, False)
        labels = cl.hdbscan_labels(x, mcs, cluster_selection_epsilon=eps, metric=metric)
        sk = "-"
        if SkHDBSCAN is not None and metric == "euclidean" and n <= 20000:
            h0 = time.perf_counter()
            SkHDBSCAN(min_cluster_size=mcs, cluster_selection_epsilon=eps).fit_predict(pts.astype(np.float64))
            sk = f"{time.perf_counter() - h0:.2f}"
        lines.append(f"{metric:<10}{n:>7}{width:>6}{mcs:>5}{core_ms:>9.3f}{mst_ms:>9.3f}{rounds:>7}{mst_ms / max(rounds, 1):>13.3f}{tree_ms:>9.3f}"
                     f"{total_ms:>10.3f}{int(labels.max()) + 1:>9}{int((labels < 0).sum()):>7}{sk:>10}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
