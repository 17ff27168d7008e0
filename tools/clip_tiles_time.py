"""Timing of the CLIP tiles at 1080p: a seeded uint8 image, M in {120, 300} seeded rectangle masks (sides
40 .. 700 pixels, log-uniform, as tools/sam_masks_time.py draws them), both layouts, antialias on and off, float16 tiles of 224 x 224:

  * new_ms     : clip_tiles from the packed masks and the image on the GPU -- the boxes launch, the rectangle arithmetic in torch and
                 the tiles launch;
  * torch_ms   : the same work as torch operations on the same GPU, per mask: the crop of the image by torch.where with the crop of
                 the mask, (the pad to a square,) F.interpolate, normalise, half.  Its rectangles are read to the host before the
                 clock starts;
  * literal_ms : the reference's formulation as written (clip_utils/__init__.py:108, :166-174; clip_utils/clip_utils.py:60-68) on
                 the GPU: the (M, H, W, 3) float tensor of masked images, then a slice, a resize and a normalisation per mask.  Timed
                 once, at M = 120, layout "crop", antialias on (the tensor is 3 GB there).

Host clock around work that ends in a device synchronise; median of --reps runs after one warm-up.  alg_MB is the sum over the masks
of 8 ch ceil(cw / 64) + 3 ch cw + 6 Sh Sw bytes (include/mi_clip_tiles.h); `of_8TBs` is the time those bytes would take at 8 TB/s
over new_ms.  max_diff is the largest difference between the two results, both float16.  The first line stamps the library build
measured (mi_rast_version).

    python tools/clip_tiles_time.py [--reps 10] [--out profiles/clip_tiles_time.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from seganygaussians_amd import _lib, clip_tiles, sam_masks  # noqa: E402
from seganygaussians_amd.contrastive_loss import pack_sam_masks  # noqa: E402

DEV = torch.device("cuda:0")
H, W = 1080, 1920
SIZE = (224, 224)
PEAK = 8e12


def rectangle_masks(M, seed):
    g = torch.Generator().manual_seed(seed)
    side = lambda: (40.0 * (700.0 / 40.0) ** torch.rand(M, generator=g)).long()
    h, w = side().clamp(max=H), side().clamp(max=W)
    y0 = (torch.rand(M, generator=g) * (H - h + 1)).long()
    x0 = (torch.rand(M, generator=g) * (W - w + 1)).long()
    ys, xs = torch.arange(H)[None, :, None], torch.arange(W)[None, None, :]
    return (ys >= y0[:, None, None]) & (ys < (y0 + h)[:, None, None]) & (xs >= x0[:, None, None]) & (xs < (x0 + w)[:, None, None])


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


def finish(plane, layout, bg, antialias, mean, std):
    """plane (ch, cw, 3) float32 on the GPU -> the (3, 224, 224) float16 tile."""
    ch, cw = plane.shape[:2]
    if layout == "pad_square":
        L = max(ch, cw)
        sq = plane.new_full((L, L, 3), bg)
        if ch > cw:
            sq[:, (L - cw) // 2:(L - cw) // 2 + cw] = plane
        else:
            sq[(L - ch) // 2:(L - ch) // 2 + ch] = plane
        plane = sq
    r = F.interpolate(plane.permute(2, 0, 1)[None], SIZE, mode="bilinear", align_corners=False, antialias=antialias)[0]
    return ((r - mean) / std).half()


def torch_tiles(image, masks, rects, layout, bg, antialias, mean, std, out):
    for m, (x0, y0, x1, y1) in enumerate(rects):
        crop = image[y0:y1, x0:x1].float() / 255.0
        out[m] = finish(torch.where(masks[m, y0:y1, x0:x1, None], crop, crop.new_tensor(bg)), layout, bg, antialias, mean, std)
    return out


def literal_tiles(image, masks, rects, bg, mean, std, out):
    keep = masks.float().unsqueeze(-1)
    full = keep * image.unsqueeze(0) + (1 - keep) * (255.0 * bg)   # (M, H, W, 3) float32: 3 GB at M = 120 and 1080p
    for m, (x0, y0, x1, y1) in enumerate(rects):
        out[m] = finish(full[m, y0:y1, x0:x1] / 255.0, "crop", bg, True, mean, std)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "clip_tiles_time.py measures on the GPU"
    image = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(DEV)
    mean = torch.tensor(clip_tiles.CLIP_MEAN, device=DEV)[:, None, None]
    std = torch.tensor(clip_tiles.CLIP_STD, device=DEV)[:, None, None]
    lines = [f"# {_lib.load().mi_rast_version().decode()}; {torch.cuda.get_device_name(0)}; {H}x{W} uint8 image, seeded rectangle masks, "
             f"float16 tiles {SIZE[0]}x{SIZE[1]}; median of {args.reps} runs after a warm-up, host clock with a device synchronise; "
             f"of_8TBs = algorithmic bytes at 8 TB/s / new_ms"]
    rows = ["layout        aa    M  torch_ms     new_ms   speedup  alg_MB  of_8TBs  max_diff"]
    for M in (120, 300):
        masks = rectangle_masks(M, seed=M).to(DEV)
        packed = pack_sam_masks(masks, device=DEV)
        rects = sam_masks.masks_to_boxes(packed).int().tolist()   # the exclusive slice [x_min, x_max) x [y_min, y_max), as it is
        nbytes = sum(8 * (y1 - y0) * ((x1 - x0 + 63) // 64) + 3 * (y1 - y0) * (x1 - x0) + 6 * SIZE[0] * SIZE[1] for x0, y0, x1, y1 in rects)
        want = torch.empty((M, 3) + SIZE, device=DEV, dtype=torch.float16)
        got = torch.empty_like(want)
        for layout in ("crop", "pad_square"):
            bg = 1.0 if layout == "crop" else 0.0
            for antialias in (True, False):
                new = lambda: clip_tiles.clip_tiles(image, packed, layout=layout, antialias=antialias, out=got)
                ref = lambda: torch_tiles(image, masks, rects, layout, bg, antialias, mean, std, want)
                _, valid = new()
                ref()
                assert bool(valid.all())
                diff = float((got.float() - want.float()).abs().max())
                t_ref, t_new = timed(ref, args.reps), timed(new, args.reps)
                line = (f"{layout:<11} {str(antialias):>5} {M:>4} {t_ref:9.3f}  {t_new:9.3f} {t_ref / t_new:8.1f}x {nbytes / 1e6:7.1f}  "
                        f"{nbytes / PEAK * 1e3 / t_new:7.3f}  {diff:.1e}")
                print(line, flush=True)
                rows.append(line)
        if M == 120:
            literal_tiles(image, masks, rects, 1.0, mean, std, want)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            literal_tiles(image, masks, rects, 1.0, mean, std, want)
            torch.cuda.synchronize()
            t_lit = (time.perf_counter() - t0) * 1e3
            clip_tiles.clip_tiles(image, packed, out=got)
            lines.append(f"# literal_ms at M = 120, layout crop, antialias on: {t_lit:.3f} (the (M, H, W, 3) float tensor of masked images on "
                         f"the GPU, then a slice, a resize and a normalisation per mask; one run after a warm-up); max_diff "
                         f"{float((got.float() - want.float()).abs().max()):.1e}")
            print(lines[-1], flush=True)
        del masks, packed
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines + rows) + "\n")


if __name__ == "__main__":
    main()
