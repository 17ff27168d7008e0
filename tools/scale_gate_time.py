"""Timing of scale conditioning: q_trans followed by scale_gate, as every SAGA stage that takes a scale runs
them, for n = 10 scales (one training iteration, train_contrastive_feature.py:228 and :241), 300 (one view of the notebook's language
loop) and 32 768 (all masks of a scene).

  * ref_ms   the reference's expression in the same run: the scales copied device -> host, the quantile transform on the host, the
             result copied host -> device (torch.Tensor(...).to(device), :58-60), then scale_gate = Linear(1, 32) + Sigmoid on the GPU.
             The host transform is scikit-learn's where it imports, otherwise the numpy restatement of tests/scale_gate_ref.py (much
             slower than the library's compiled code: then ref_ms is an upper bound); the header line says which was used.
  * new_ms   scale_gates(scales, sq, weight, bias): one launch.
  * fwd+bwd  the same with the backward for weight and bias behind it (ref: autograd through Linear + Sigmoid).
  * launches and device-to-host copies per call: counted with torch.profiler in one extra call of each path where the profiler
    gives device events ("-" where it does not).  By construction the fused forward is one launch and no copy.

ref and new alternate call by call; host clock around work that ends in a synchronise, median of --reps calls after a warm-up.
The kernels are latency-bound at these sizes: what is measured is the removed round trip, not bandwidth.

    python tools/scale_gate_time.py [--reps 50] [--sizes 10 300 32768] [--no-profiler] [--out profiles/scale_gate_time.txt]"""
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
from seganygaussians_amd import scale_gate as sg  # noqa: E402

DEV = torch.device("cuda:0")
CHANNELS = 32


def host_transformer(all_scales):
    """(name, transform of an (n, 1) float32 numpy column) fitted on all_scales."""
    try:
        from sklearn.preprocessing import QuantileTransformer
        qt = QuantileTransformer(output_distribution="uniform").fit(all_scales.reshape(-1, 1))
        return "scikit-learn", qt.transform, qt.quantiles_[:, 0], qt.references_
    except ImportError:
        from tests import scale_gate_ref as sr
        quantiles, references = sr.fit_quantiles(all_scales)
        return "the numpy restatement (scikit-learn is not installed)", (lambda x: sr.transform(x, quantiles, references)), quantiles, references


def count_device_events(fn):
    """(kernel launches, device-to-host copies) of one call, or (None, None) without a working profiler."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        if not dev:
            return None, None
        copies = [e for e in dev if "memcpy" in e.name.lower() or "copy" in e.name.lower() and "kernel" not in e.name.lower()]
        d2h = [e for e in copies if "dtoh" in e.name.lower() or "devicetohost" in e.name.lower().replace(" ", "")]
        return len(dev) - len(copies), len(d2h)
    except Exception:
        return None, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sizes", type=int, nargs="+", default=[10, 300, 32768])
    ap.add_argument("--no-profiler", action="store_true", help="do not count launches and device-to-host copies")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "scale_gate_time.py measures on the GPU"
    assert args.reps >= 10
    rng = np.random.default_rng(0)
    all_scales = rng.gamma(2.0, 0.5, 32768).astype(np.float32)
    np.random.seed(0)
    host_name, host_transform, quantiles, references = host_transformer(all_scales)
    np.random.seed(0)
    sq = sg.ScaleQuantile.fit(torch.from_numpy(all_scales).to(DEV))
    same_table = bool(np.array_equal(sq.quantiles.cpu().numpy().view(np.int64), quantiles.view(np.int64)))
    scale_gate = torch.nn.Sequential(torch.nn.Linear(1, CHANNELS, bias=True), torch.nn.Sigmoid()).to(DEV)
    weight, bias = scale_gate[0].weight, scale_gate[0].bias
    lines = [f"# {_lib.load().mi_rast_version().decode()}; {torch.cuda.get_device_name(0)}; q_trans + scale_gate (Linear(1, {CHANNELS}) + Sigmoid) of n "
             f"scales; host transform of ref: {host_name}; the device table equals the host's bit for bit: {same_table}; median of {args.reps} "
             "calls after warm-up, ref and new alternating, host clock around work that ends in a synchronise; ref = device -> host copy, host "
             "transform, host -> device copy, scale_gate; new = scale_gates (one launch); launches / device-to-host copies counted with "
             "torch.profiler in one extra call (- = no device events)",
             "n       pass      ref_ms    new_ms   ref/new  ref_launch ref_d2h  new_launch new_d2h  same_u"]
    for n in args.sizes:
        scales = torch.from_numpy(rng.gamma(2.0, 0.5, n).astype(np.float32)).to(DEV)
        g = torch.randn(n, CHANNELS, device=DEV)

        def q_trans(s):      # train_contrastive_feature.py:54-60
            s = s.reshape(-1, 1)
            return torch.Tensor(host_transform(s.detach().cpu().numpy())).to(s.device)

        def ref(backward):
            gates = scale_gate(q_trans(scales).squeeze().unsqueeze(-1))
            if backward:
                weight.grad = bias.grad = None
                gates.backward(g)
            torch.cuda.synchronize()

        def new(backward):
            gates = sg.scale_gates(scales, sq, weight, bias)
            if backward:
                weight.grad = bias.grad = None
                gates.backward(g)
            torch.cuda.synchronize()

        same_u = bool(torch.equal(q_trans(scales).reshape(-1).view(torch.int32), sq.transform(scales).view(torch.int32)))
        for name, backward in (("forward", False), ("fwd+bwd", True)):
            def interval(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(backward)
                return (time.perf_counter() - t0) * 1e3
            for _ in range(5):
                interval(ref), interval(new)
            t_ref, t_new = [], []
            for _ in range(args.reps):
                t_ref.append(interval(ref))
                t_new.append(interval(new))
            t_ref, t_new = statistics.median(t_ref), statistics.median(t_new)
            ref_counts = (None, None) if args.no_profiler else count_device_events(lambda: ref(backward))
            new_counts = (None, None) if args.no_profiler else count_device_events(lambda: new(backward))
            show = lambda v: "-" if v is None else str(v)
            line = (f"{n:<7} {name:<9} {t_ref:7.3f}  {t_new:8.3f}  {t_ref / t_new:6.2f}x  {show(ref_counts[0]):>10} {show(ref_counts[1]):>7}  "
                    f"{show(new_counts[0]):>10} {show(new_counts[1]):>7}  {same_u}")
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
