"""Timing of the model cut: one press of the GUI's "segment3d" button, i.e. segment(mask) of the scene model
(SH degree 3: 59 floats per row) and of the feature model (32-D: 43 floats per row) with the same mask.

  * ref_ms     the reference's expression restated in PyTorch on the same GPU in the same run (scene/gaussian_model.py:376-428 and
               scene/gaussian_model_ff.py:257-285 with optimizer None: count_nonzero, one boolean index per tensor, the three masked
               reads and writes of _mask), the two models one after the other;
  * new_ms     segment_models([scene, feature], mask): one plan, one host read, a row map and a gather per model;
  * gather_ms  the two row-map + gather calls of new_ms alone (mi_edit_apply with the plan already made);
  * launches and host reads per press: counted with torch.profiler in one extra press of each path where the profiler gives device
    events ("-" where it does not); device-to-host copies stand for host reads.  By construction the fused press makes 8 launches
    (4 plan, 2 per model) and one 8-byte device-to-host copy; what the profiler adds to that are the allocations' fills, if any.
  * of_8TBs    bytes the cut needs (the mask + kept rows read + kept rows written, both models) / time / 8 TB/s, over new_ms and
               over gather_ms.

P0 = 1 M and 5 M; kept fractions 0.01, 0.3, 0.9; "one cut" of the loaded model and "cut of a cut" (a first cut that keeps half,
outside the interval, then the timed one on what is left).  ref and new alternate iteration by iteration; every iteration starts
from the same state, restored outside the interval.  Device events around work that ends in a synchronise, median of --reps
iterations after a warm-up.

    python tools/model_edit_time.py [--reps 10] [--sizes 1000000 5000000] [--no-profiler] [--out profiles/model_edit_time.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from seganygaussians_amd import _lib  # noqa: E402
from seganygaussians_amd import model_edit as me  # noqa: E402

DEV = torch.device("cuda:0")
PEAK_BW = 8.0e12
LAYOUTS = {"scene": {"_xyz": (3,), "_features_dc": (1, 3), "_features_rest": (15, 3), "_opacity": (1,), "_scaling": (3,), "_rotation": (4,)},
           "feature": {"_xyz": (3,), "_point_features": (32,), "_opacity": (1,), "_scaling": (3,), "_rotation": (4,)}}
FLOATS = {"scene": 59, "feature": 43}


class Model:
    """The attributes the cut works on."""

    def __init__(self, kind, P0, gen):
        self.kind, self.optimizer, self.segment_times = kind, None, 0
        for field, trailing in LAYOUTS[kind].items():
            setattr(self, field, torch.randn((P0,) + trailing, generator=gen, device=DEV))
            setattr(self, "old" + field, [])
        if kind == "scene":
            self.old_mask = []
        self._mask = torch.ones((P0,), dtype=torch.float, device=DEV)

    def snapshot(self):
        return ({f: getattr(self, f) for f in LAYOUTS[self.kind]}, self._mask.clone(), self.segment_times)

    def restore(self, snap):
        tensors, level, times = snap
        for f, t in tensors.items():
            setattr(self, f, t)
            setattr(self, "old" + f, [])
        if self.kind == "scene":
            self.old_mask = []
        self._mask.copy_(level)
        self.segment_times = times


def reference_segment(self, mask):
    """The reference's segment with optimizer None, line for line as PyTorch evaluates it."""
    mask = mask.squeeze()
    if torch.count_nonzero(mask) == 0:
        mask = ~mask
    for f in LAYOUTS[self.kind]:
        getattr(self, "old" + f).append(getattr(self, f))
    if self.kind == "scene":
        self.old_mask.append(self._mask)
    for f in LAYOUTS[self.kind]:
        setattr(self, f, getattr(self, f)[mask])
    self.segment_times += 1
    tmp = self._mask[self._mask == self.segment_times]
    tmp[mask] += 1
    self._mask[self._mask == self.segment_times] = tmp


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 5_000_000])
    ap.add_argument("--no-profiler", action="store_true", help="do not count launches and host reads")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "model_edit_time.py measures on the GPU"
    assert args.reps >= 10
    lines = [f"# {_lib.load().mi_rast_version().decode()}; {torch.cuda.get_device_name(0)}; one press = segment(mask) of the scene model (59 floats per "
             f"row) and the feature model (43) with one mask; median of {args.reps} iterations after warm-up, ref and new alternating, device "
             "events around work that ends in a synchronise; ref = the reference's expression in PyTorch; new = segment_models; gather = its two "
             "mi_edit_apply calls alone; launches / host reads counted with torch.profiler in one extra press (- = no device events); "
             "of_8TBs = (mask + kept rows read + kept rows written) / time / 8 TB/s",
             "P0        stage          rows      kept      ref_ms   new_ms  ref/new  gather_ms  ref_launch ref_reads  new_launch new_reads  "
             "of_8TBs(new)  of_8TBs(gather)"]
    gen = torch.Generator(device=DEV).manual_seed(0)
    for P0 in args.sizes:
        models = [Model("scene", P0, gen), Model("feature", P0, gen)]
        for stage in ("one cut", "cut of a cut"):
            if stage == "cut of a cut":
                first = torch.rand(P0, generator=gen, device=DEV) < 0.5
                me.segment_models(models, first)
            snaps = [m.snapshot() for m in models]
            n = models[0]._xyz.shape[0]
            for fraction in (0.01, 0.3, 0.9):
                mask = torch.rand(n, generator=gen, device=DEV) < fraction
                kept = int(mask.sum())

                def reset():
                    for m, s in zip(models, snaps):
                        m.restore(s)
                    torch.cuda.synchronize()

                def ref():
                    for m in models:
                        reference_segment(m, mask)
                    torch.cuda.synchronize()

                def new():
                    me.segment_models(models, mask)
                    torch.cuda.synchronize()

                def interval(fn):
                    reset()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    return e0.elapsed_time(e1)

                for _ in range(2):
                    interval(ref), interval(new)
                t_ref, t_new = [], []
                for _ in range(args.reps):
                    t_ref.append(interval(ref))
                    t_new.append(interval(new))
                t_ref, t_new = statistics.median(t_ref), statistics.median(t_new)
                # the gather alone: the plan made once, apply without the level update is the same work every time
                reset()
                tensor_lists = [[getattr(m, f) for f in LAYOUTS[m.kind]] for m in models]
                plan = me._Plan("model_edit_time", models[0]._mask, models[0].segment_times, mask.contiguous(), n, DEV)

                def gather():
                    for tensors in tensor_lists:
                        plan.apply(None, tensors)
                    torch.cuda.synchronize()
                t_gather = []
                for k in range(args.reps + 2):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    gather()
                    e1.record()
                    torch.cuda.synchronize()
                    if k >= 2:
                        t_gather.append(e0.elapsed_time(e1))
                t_gather = statistics.median(t_gather)
                reset()
                ref_counts = (None, None) if args.no_profiler else count_device_events(ref)
                reset()
                new_counts = (None, None) if args.no_profiler else count_device_events(new)
                reset()
                show = lambda v: "-" if v is None else str(v)
                nbytes = n + 2 * 4 * kept * (FLOATS["scene"] + FLOATS["feature"])
                line = (f"{P0:<9} {stage:<14} {n:<9} {kept:<9} {t_ref:7.3f}  {t_new:7.3f}  {t_ref / t_new:6.2f}x  {t_gather:9.3f}  "
                        f"{show(ref_counts[0]):>10} {show(ref_counts[1]):>9}  {show(new_counts[0]):>10} {show(new_counts[1]):>9}  "
                        f"{nbytes / (t_new * 1e-3) / PEAK_BW:12.3f}  {nbytes / (t_gather * 1e-3) / PEAK_BW:15.3f}")
                print(line, flush=True)
                lines.append(line)
            for m, s in zip(models, snaps):
                m.restore(s)
        del models
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
