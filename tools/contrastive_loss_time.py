"""Device-event timing of the contrastive loss: sample_contrastive_targets + contrastive_loss forward and
backward against the reference block restated in torch (tests/test_contrastive_loss.py: train_contrastive_feature.py:145-226 and
:255-299), at 1080p, M in {60, 120, 250} nested synthetic masks, S ~ 1000 and 1600 rays, N = 10 scales, C = 32.  Warm-up, then
the median of --reps timed iterations of each; peak extra device memory of one iteration each.  Masks come from the CPU as in the
reference (`original_masks.cuda()`); the new path is also timed with the masks packed once (pack_sam_masks, cached per camera).

    python tools/contrastive_loss_time.py [--reps 10] [--out profiles/contrastive_loss_time.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from seganygaussians_amd.contrastive_loss import contrastive_loss, pack_sam_masks, sample_contrastive_targets  # noqa: E402
from tests.test_contrastive_loss import _reference_loss, _reference_targets, synthetic_masks  # noqa: E402

DEV = "cuda:0"
H, W, N, C = 1080, 1920, 10, 32


def _feats(S):
    g = torch.Generator().manual_seed(S)
    return torch.nn.functional.normalize(torch.randn(N, S, C, generator=g), dim=-1).to(DEV).requires_grad_(True)


def new_iter(masks, scales, ub, rays):
    tg = sample_contrastive_targets(masks, scales, ub, num_sampled_rays=rays)
    loss, _ = contrastive_loss(_feats(tg.num_rays), tg)
    loss.backward()


def ref_iter(masks, scales, ub, rays):
    _, _, gt, w = _reference_targets(masks, scales, ub, num_sampled_rays=rays)
    loss = _reference_loss(_feats(gt.shape[1]), gt, w)[0]
    loss.backward()


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return statistics.median(ms), (torch.cuda.max_memory_allocated() - base) / 2**20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "contrastive_loss_time.py measures on the GPU"
    lines = [f"# {torch.cuda.get_device_name(0)}; 1080x1920, N={N}, C={C}; median of {args.reps} iterations after warm-up, "
             f"device events; peak = extra device memory of one iteration",
             "M     rays  S     reference_ms  ref_peak_MiB  new_ms  new_peak_MiB  new_packed_ms  packed_peak_MiB  speedup  speedup_packed"]
    for M in (60, 120, 250):
        masks, scales = synthetic_masks(M, H, W, seed=M)
        ub = float(scales.max())
        packed = pack_sam_masks(masks, device=DEV)
        for rays in (1000, 1600):
            torch.manual_seed(0)
            S = sample_contrastive_targets(packed, scales, ub, num_sampled_rays=rays).num_rays
            t_ref, p_ref = timed(lambda: ref_iter(masks, scales, ub, rays), args.reps)
            t_new, p_new = timed(lambda: new_iter(masks, scales, ub, rays), args.reps)
            t_pk, p_pk = timed(lambda: new_iter(packed, scales, ub, rays), args.reps)
            line = (f"{M:<5} {rays:<5} {S:<5} {t_ref:12.2f}  {p_ref:12.0f}  {t_new:6.2f}  {p_new:12.0f}  {t_pk:13.2f}  {p_pk:15.0f}  "
                    f"{t_ref / t_new:7.1f}x  {t_ref / t_pk:13.1f}x")
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
