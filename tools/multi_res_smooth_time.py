"""Timing of the fused multi-resolution KNN feature smoothing (knn_smooth.py: multi_res_smooth_point_features,
include/mi_knn_smooth.h: mi_knn_smooth_multi_*) at the size the reference trains at: P = 1 M Gaussians, C = 32, default rates
(0.1, 0.5, 1.5) and Ks (4, 4, 16), (P, 3) softmax weights that require a gradient -- against the reference's own PyTorch expression
(scene/gaussian_model_ff.py:391-400) on the same device and the same maps.

  * kernels     : the C-ABI calls on preallocated buffers: forward; backward pass B alone (a call that needs no pass A: no
                  normalize_out, no dL/dw); the whole backward; pass A = whole - B (the library launches the two back to back);
  * autograd    : forward and backward through multi_res_smooth_point_features (PyTorch's allocations and bookkeeping included);
  * reference   : forward and backward of the PyTorch expression.

Device events, median of --reps iterations after a warm-up.  Also: the peak memory either route takes beyond its inputs, the bytes
the fused passes have to move (counted as in profiles/r01_knn_smooth.md: gathered rows and their indices, rows read and written), and
the median and maximum length of the inverse lists that pass B walks, one lane group per list.

    python tools/multi_res_smooth_time.py [--reps 10] [--out profiles/multi_res_smooth_time.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from seganygaussians_amd import _lib  # noqa: E402
from seganygaussians_amd import knn_smooth as ks  # noqa: E402
from seganygaussians_amd._ffi import check, stream_ptr  # noqa: E402

DEV = torch.device("cuda:0")
HBM_PEAK_GBPS = 8000.0
RATES, KS = (0.1, 0.5, 1.5), (4, 4, 16)


def timed(fn, reps, marks=2):
    """Medians of the intervals between `marks` events that fn(record) places on the stream."""
    for _ in range(5):
        fn(lambda: None)
    torch.cuda.synchronize()
    ts = [[] for _ in range(marks - 1)]
    for _ in range(reps):
        ev = []

        def record():
            ev.append(torch.cuda.Event(enable_timing=True))
            ev[-1].record()
        fn(record)
        torch.cuda.synchronize()
        assert len(ev) == marks
        for k in range(marks - 1):
            ts[k].append(ev[k].elapsed_time(ev[k + 1]))
    return [statistics.median(t) for t in ts]


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    fn(lambda: None)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(DEV) - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "multi_res_smooth_time.py measures on the GPU"
    P, C, L, Ktot = args.points, 32, len(KS), sum(KS)
    lib = _lib.load()
    gen = torch.Generator().manual_seed(3)
    xyz = (torch.randn(P, 3, generator=gen) * torch.tensor([3.0, 2.0, 1.0])).to(DEV)
    feats = (torch.randn(P, C, generator=gen) * (0.1 + 3 * torch.rand(P, 1, generator=gen))).to(DEV).requires_grad_(True)
    logits = torch.randn(P, L, generator=gen).to(DEV)
    up = torch.randn(P, C, generator=gen).to(DEV)
    masks = ks.draw_point_masks(P, RATES, generator=gen)
    from seganygaussians_amd.knn import KnnIndex
    levels = [(pm, KnnIndex(xyz[pm.to(DEV)]).query(xyz, k)[0]) for pm, k in zip(masks, KS)]
    mr = ks.MultiResNeighbourMap(levels)
    nmap = mr.nmap
    lengths = (nmap.inv_offsets[1:] - nmap.inv_offsets[:-1]).long()
    weights = torch.softmax(logits, dim=1).requires_grad_(True)
    lines = [f"# {lib.mi_rast_version().decode()}; {torch.cuda.get_device_name(0)}; P = {P}, C = {C}, rates {RATES}, Ks {KS}, (P, {L}) weights; "
             f"median of {args.reps} iterations after warm-up, device events",
             f"# subsets: {', '.join(str(int(pm.sum())) for pm in masks)} members",
             "case                                   ms"]

    def emit(case, ms):
        line = f"{case:<38} {ms:8.3f}"
        print(line, flush=True)
        lines.append(line)
        return ms

    # ---- the kernels, through the C-ABI on preallocated buffers
    f, w = feats.detach(), weights.detach()
    out, dret, dF, dw = torch.empty_like(f), torch.empty_like(f), torch.empty_like(f), torch.empty_like(w)
    stream = stream_ptr(DEV)

    def forward(normalize_out):
        def fn(record):
            record()
            check(lib.mi_knn_smooth_multi_forward(P, C, L, mr.level_k_c, nmap.idx.data_ptr(), w.data_ptr(), 0, f.data_ptr(), out.data_ptr(),
                                                  normalize_out, stream))
            record()
        return fn

    def backward(normalize_out, want_dw):
        def fn(record):
            record()
            check(lib.mi_knn_smooth_multi_backward(P, C, L, mr.level_k_c, nmap.idx.data_ptr(), nmap.inv_offsets.data_ptr(),
                                                   nmap.inv_entries.data_ptr(), w.data_ptr(), 0, f.data_ptr(), up.data_ptr(), dret.data_ptr(),
                                                   dF.data_ptr(), dw.data_ptr() if want_dw else None, normalize_out, stream))
            record()
        return fn

    for _ in range(30):     # clocks in steady state before the first timed case
        forward(0)(lambda: None)
    t_fwd = emit("kernel forward", timed(forward(0), args.reps)[0])
    t_b = emit("kernel backward pass B alone", timed(backward(0, False), args.reps)[0])
    t_ab = emit("kernel backward (A: dL/dw, B)", timed(backward(0, True), args.reps)[0])
    emit("  pass A = backward - B", t_ab - t_b)
    t_fwd_n = emit("kernel forward, normalize_out", timed(forward(1), args.reps)[0])
    t_ab_n = emit("kernel backward, normalize_out", timed(backward(1, True), args.reps)[0])
    emit("  pass A = backward - B", t_ab_n - t_b)

    # ---- through autograd, and the reference expression
    def fused(record):
        feats.grad = weights.grad = None
        record()
        o = ks.multi_res_smooth_point_features(feats, mr, weights, normalize_out=False)
        record()
        o.backward(up)
        record()

    idx_dev = [(pm.to(DEV), idx) for pm, idx in levels]

    def reference(record):
        feats.grad = weights.grad = None
        record()
        normed = torch.nn.functional.normalize(feats, dim=-1, p=2)
        ret = torch.zeros_like(normed)
        for i, (pm, idx) in enumerate(idx_dev):
            ret += weights[:, i:i + 1] * normed[pm][idx, :].mean(dim=1)
        record()
        ret.backward(up)
        record()

    tf, tb = timed(fused, args.reps, marks=3)
    emit("autograd forward", tf)
    emit("autograd backward", tb)
    rf, rb = timed(reference, args.reps, marks=3)
    emit("reference expression forward", rf)
    emit("reference expression backward", rb)
    mem = []
    for fn in (fused, reference):
        feats.grad = weights.grad = None          # the gradients count as the route's memory, not as its inputs
        mem.append(peak_extra(fn))
    mem_fused, mem_ref = mem

    # ---- bytes the passes have to move (profiles/r01_knn_smooth.md): gathered rows + their indices, rows read and written
    row = 4 * C
    bytes_fwd = P * (Ktot * (row + 4) + 4 * L + row)
    bytes_a = P * (Ktot * (row + 4) + 4 * L + row + row + 4 * L)            # + dL/dout read, dL/dret and dL/dw written
    bytes_b = P * (Ktot * (row + 4 + 4) + 4 + row + row)                    # per entry: the dL/dret row, the entry, one weight
    tail = [
        f"# fused fwd + bwd: kernels {t_fwd + t_ab:.3f} ms, through autograd {tf + tb:.3f} ms; reference expression {rf + rb:.3f} ms "
        f"({(rf + rb) / (tf + tb):.1f}x the autograd route)",
        f"# peak memory beyond the inputs, one forward + backward: fused {mem_fused / 2**20:.0f} MiB, reference expression {mem_ref / 2**20:.0f} MiB",
        f"# algorithmic bytes: forward {bytes_fwd / 1e9:.3f} GB ({bytes_fwd / (t_fwd * 1e-3) / 1e9:.0f} GB/s), pass A {bytes_a / 1e9:.3f} GB "
        f"({bytes_a / (max(t_ab - t_b, 1e-6) * 1e-3) / 1e9:.0f} GB/s), pass B {bytes_b / 1e9:.3f} GB ({bytes_b / (t_b * 1e-3) / 1e9:.0f} GB/s); "
        f"HBM peak {HBM_PEAK_GBPS:.0f} GB/s (rates over algorithmic bytes: the maps are spatially local, part of the gathers is served by the caches)",
        f"# inverse lists (pass B, one lane group per list): median {int(lengths.median())}, maximum {int(lengths.max())}, mean {Ktot} entries; "
        f"lists longer than 4 x the median: {int((lengths > 4 * lengths.median()).sum())} of {P}",
        f"# single-map path for comparison (profiles/r01_knn_smooth.md): 0.67 ms forward + backward for 8 columns; here {Ktot} columns",
    ]
    for line in tail:
        print(line, flush=True)
    lines += tail
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
