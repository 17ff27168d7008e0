"""Timing of the SAM-mask set operations at 1080p, M in {120, 300} seeded rectangle masks (sides 40 .. 700
pixels, log-uniform: mostly small masks, a few that cover a quarter of the image), K in {1, 3} score columns:

  * overlaps : mask_overlaps from packed masks, against m.flatten(1).float() @ m.flatten(1).float().T on the same GPU (the float
               masks already on the device);
  * boxes    : masks_to_boxes from packed masks, against the any / argmax statement of torchvision's masks_to_boxes in torch;
  * nms      : mask_nms from packed masks, sort and idx[keep] included.  The reference's pair loop (sam_utils.py:146-158) is two
               full-image sums per pair, M (M + 1) / 2 pairs -- minutes per call at these sizes -- and is not timed;
  * images   : mask_score_images from packed masks per mode, against the reference's statements on the float masks:
               einsum('kp,khw->kphw').sum(0) / (masks.sum(0) + 1e-9) (:282), (r[:, :, None, None] * m[:, None]).sum(0) (:380 per
               column), .max(0) (:206).

Host clock around work that ends in a device synchronise; median of --reps runs after one warm-up.  `of_8TBs` is the time the
algorithmic bytes of include/mi_mask_sets.h would take at 8 TB/s over the measured time.  The first line stamps the library build
measured (mi_rast_version).

    python tools/sam_masks_time.py [--reps 10] [--out profiles/sam_masks_time.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from seganygaussians_amd import _lib, sam_masks  # noqa: E402
from seganygaussians_amd.contrastive_loss import pack_sam_masks  # noqa: E402

DEV = torch.device("cuda:0")
H, W = 1080, 1920
WQ = (W + 63) // 64
PEAK = 8e12


def rectangle_masks(M, seed):
    g = torch.Generator().manual_seed(seed)
    side = lambda: (40.0 * (700.0 / 40.0) ** torch.rand(M, generator=g)).long()
    h, w = side().clamp(max=H), side().clamp(max=W)
    y0 = (torch.rand(M, generator=g) * (H - h + 1)).long()
    x0 = (torch.rand(M, generator=g) * (W - w + 1)).long()
    ys, xs = torch.arange(H)[None, :, None], torch.arange(W)[None, None, :]
    return (ys >= y0[:, None, None]) & (ys < (y0 + h)[:, None, None]) & (xs >= x0[:, None, None]) & (xs < (x0 + w)[:, None, None])


def torch_boxes(m):
    rows, cols = m.any(dim=2), m.any(dim=1)
    first = lambda b: b.to(torch.uint8).argmax(dim=1)
    last = lambda b: b.shape[1] - 1 - b.flip(1).to(torch.uint8).argmax(dim=1)
    return torch.stack([first(cols), first(rows), last(cols), last(rows)], dim=1).float()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sam_masks_time.py measures on the GPU"
    lines = [f"# {_lib.load().mi_rast_version().decode()}; {torch.cuda.get_device_name(0)}; {H}x{W}, seeded rectangle masks; median of "
             f"{args.reps} runs after a warm-up, host clock with a device synchronise; of_8TBs = algorithmic bytes at 8 TB/s / new_ms",
             "# the reference's mask_nms pair loop (two full-image sums per pair, M (M + 1) / 2 pairs) takes minutes per call: not timed",
             "op            M    K  torch_ms     new_ms   speedup  alg_MB  of_8TBs  equal"]

    def row(op, M, K, t_ref, t_new, nbytes, equal):
        ref = f"{t_ref:9.3f}" if t_ref is not None else "        -"
        sp = f"{t_ref / t_new:8.1f}x" if t_ref is not None else "        -"
        line = f"{op:<12} {M:>4} {K:>4} {ref}  {t_new:9.3f} {sp} {nbytes / 1e6:7.1f}  {nbytes / PEAK * 1e3 / t_new:7.3f}  {equal}"
        print(line, flush=True)
        lines.append(line)

    for M in (120, 300):
        masks = rectangle_masks(M, seed=M).to(DEV)
        packed = pack_sam_masks(masks, device=DEV)
        mf = masks.float()
        mask_bytes = 8 * M * H * WQ
        flat = mf.flatten(1)
        ref_inter = flat @ flat.T
        inter, areas = sam_masks.mask_overlaps(packed)
        row("overlaps", M, "-", timed(lambda: flat @ flat.T, args.reps), timed(lambda: sam_masks.mask_overlaps(packed), args.reps),
            mask_bytes + 4 * M * M, bool(torch.equal(inter.float(), ref_inter)))
        row("boxes", M, "-", timed(lambda: torch_boxes(masks), args.reps), timed(lambda: sam_masks.masks_to_boxes(packed), args.reps),
            mask_bytes, bool(torch.equal(sam_masks.masks_to_boxes(packed), torch_boxes(masks))))
        scores = torch.rand(M, generator=torch.Generator().manual_seed(M)).to(DEV)
        kept = sam_masks.mask_nms(packed, scores)
        row("nms", M, "-", None, timed(lambda: sam_masks.mask_nms(packed, scores), args.reps), mask_bytes + 12 * M * M, f"kept {kept.numel()}")
        for K in (1, 3):
            s = torch.randn(M, K, generator=torch.Generator().manual_seed(K)).to(DEV)
            statements = {
                "mean": lambda: torch.einsum("kp,khw->kphw", s, mf).sum(dim=0) / (mf.sum(dim=0, keepdim=True) + 1e-9),
                "sum": lambda: (s[:, :, None, None] * mf[:, None]).sum(dim=0),
                "max": lambda: (s[:, :, None, None] * mf[:, None]).max(dim=0)[0],
            }
            for mode, statement in statements.items():
                got, want = sam_masks.mask_score_images(s, packed, mode=mode), statement()
                close = torch.equal(got, want) if mode == "max" else f"max diff {float((got - want).abs().max()):.1e}"
                row("images " + mode, M, K, timed(statement, args.reps),
                    timed(lambda: sam_masks.mask_score_images(s, packed, mode=mode), args.reps), mask_bytes + 4 * K * H * W, close)
                del got, want
        del mf, flat, masks
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
