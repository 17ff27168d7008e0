"""Timing of the photometric loss against the reference's own expression (tests/photometric_ref.py in
float32, run on the device through autograd: five grouped 11 x 11 conv2d and their backward, as utils/loss_utils.py does):

  * sizes 3 x 540 x 960, 3 x 1080 x 1920 (the BASELINE image), 3 x 2160 x 3840;
  * forward alone (no grad) and forward + backward;
  * beside each: a plain device copy that moves as many bytes as the new path's algorithmic traffic (forward alone: 8 bytes per
    element read; forward + backward: 8 read + 12 written, then 20 read + 4 written = 44), taken in the same run.

Device events, median of --reps iterations after a warm-up; peak = extra device memory of one iteration.  of_8TBs = algorithmic bytes /
new_ms / 8 TB/s.

    python tools/photometric_time.py [--reps 20] [--out profiles/photometric_time.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from seganygaussians_amd import _lib  # noqa: E402
from seganygaussians_amd.photometric import photometric_loss  # noqa: E402
from tests import photometric_ref as ref  # noqa: E402

DEV = torch.device("cuda:0")
PEAK_BW = 8.0e12
SIZES = ((3, 540, 960), (3, 1080, 1920), (3, 2160, 3840))
FWD_BYTES, FWD_BWD_BYTES = 8, 44      # per element


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "photometric_time.py measures on the GPU"
    assert args.reps >= 10
    lines = [f"# {_lib.load().mi_rast_version().decode()}; {torch.cuda.get_device_name(0)}; median of {args.reps} iterations after warm-up, "
             f"device events; peak = extra device memory of one iteration; ref = the float32 restatement of utils/loss_utils.py on the "
             f"device through autograd; copy = dst.copy_(src) moving the new path's algorithmic bytes (half read, half written) in the "
             f"same run; of_8TBs = algorithmic bytes / new_ms / 8 TB/s",
             "pass     C  H     W     ref_ms    ref_peak_MiB  new_ms   new_peak_MiB  ref/new  copy_ms  new/copy  alg_MB   of_8TBs"]

    for C, H, W in SIZES:
        x, g = (t.to(DEV) for t in ref.make_pair("noise", (C, H, W), seed=0))
        n = C * H * W
        xg = x.clone().requires_grad_(True)

        def new_fwd():
            with torch.no_grad():
                photometric_loss(x, g)

        def ref_fwd():
            with torch.no_grad():
                ref.loss(x, g)

        def new_both():
            xg.grad = None
            photometric_loss(xg, g).backward()

        def ref_both():
            xg.grad = None
            ref.loss(xg, g).backward()

        for name, new, old, per_elem in (("fwd", new_fwd, ref_fwd, FWD_BYTES), ("fwd+bwd", new_both, ref_both, FWD_BWD_BYTES)):
            nbytes = per_elem * n
            src = torch.empty(nbytes // 8, device=DEV, dtype=torch.float32)     # nbytes / 2 read + nbytes / 2 written
            dst = torch.empty_like(src)
            t_copy, _ = timed(lambda: dst.copy_(src), args.reps)
            del src, dst
            t_ref, p_ref = timed(old, args.reps)
            t_new, p_new = timed(new, args.reps)
            line = (f"{name:<8} {C:<2} {H:<5} {W:<5} {t_ref:8.3f}  {p_ref:12.0f}  {t_new:7.3f}  {p_new:12.0f}  {t_ref / t_new:6.1f}x  "
                    f"{t_copy:7.3f}  {t_new / t_copy:8.2f}  {nbytes / 1e6:7.1f}  {nbytes / (t_new * 1e-3) / PEAK_BW:7.3f}")
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
