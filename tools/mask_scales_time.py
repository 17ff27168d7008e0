"""Timing of the SAM-mask scales at 1080p, M in {60, 120, 250} nested synthetic masks
(tests/test_contrastive_loss.py:synthetic_masks) and a seeded depth with a zero patch:

  * reference_cpu : get_scale.py:128-159 as written (tests/test_mask_scales_host.py:literal_scales), on the CPU with 16 torch threads,
                    the f32 float masks already in memory as the reference keeps them (images_masks, :107);
  * reference_gpu : the same expression in torch on the GPU, the float masks already on the device;
  * new_bool      : sam_mask_scales from the bool masks on the CPU (host-to-device copy and packing included);
  * new_packed    : sam_mask_scales from masks packed once (pack_sam_masks).

Host clock around work that ends in a device synchronise; median of --reps runs after one warm-up (--cpu-reps for the CPU
reference).  The first line stamps the library build measured (mi_rast_version).

    python tools/mask_scales_time.py [--reps 10] [--cpu-reps 2] [--out profiles/mask_scales_time.txt]"""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from seganygaussians_amd import _lib  # noqa: E402
from seganygaussians_amd.contrastive_loss import pack_sam_masks  # noqa: E402
from seganygaussians_amd.mask_scales import sam_mask_scales  # noqa: E402
from tests.test_contrastive_loss import synthetic_masks  # noqa: E402
from tests.test_mask_scales_host import literal_scales  # noqa: E402

DEV = torch.device("cuda:0")
H, W = 1080, 1920
FOVX, FOVY = 2 * math.atan(W / (2 * 1421.0)), 2 * math.atan(H / (2 * 1421.0))


def literal_on(dev, depth, masks_f):
    """literal_scales with every tensor on `dev` (the reference's expression, run where its inputs are)."""
    d = depth.to(dev)
    grid = torch.stack(torch.meshgrid([torch.arange(H, device=dev), torch.arange(W, device=dev)], indexing="ij"), dim=-1)
    pts = torch.zeros(H, W, 3, device=dev)
    pts[:, :, -1] = d
    cx, cy = W / 2, H / 2
    fx, fy = cx / math.tan(FOVX / 2), cy / math.tan(FOVY / 2)
    pts[:, :, 0] = (grid[:, :, 0] - cx) * d / fx
    pts[:, :, 1] = (grid[:, :, 1] - cy) * d / fy
    up = torch.nn.functional.interpolate(masks_f.unsqueeze(1), mode="bilinear", size=(H, W), align_corners=False)
    er = torch.conv2d(up.float(), torch.full((3, 3), 1.0, device=dev).view(1, 1, 3, 3), padding=1)
    er = (er >= 5).squeeze()
    scale = torch.zeros(len(masks_f), device=dev)
    for m in range(len(masks_f)):
        scale[m] = (pts[er[m] == 1].std(dim=0) * 2).norm()
    return scale


def timed(fn, reps, sync=True):
    fn()
    if sync:
        torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mask_scales_time.py measures on the GPU"
    torch.set_num_threads(16)
    g = torch.Generator().manual_seed(0)
    depth = 1.0 + 4.0 * torch.rand(H, W, generator=g)
    depth[: H // 4, : W // 4] = 0.0
    depth_dev = depth.to(DEV)
    lines = [f"# {_lib.load().mi_rast_version().decode()}; {torch.cuda.get_device_name(0)}; {H}x{W} depth, nested synthetic masks; "
             f"median of {args.reps} GPU / {args.cpu_reps} CPU runs after a warm-up, host clock with a device synchronise; "
             f"CPU reference with {torch.get_num_threads()} torch threads",
             "M     reference_cpu_ms  reference_gpu_ms  new_bool_ms  new_packed_ms  max_rel_diff  vs_cpu_packed  vs_gpu_packed"]
    for M in (60, 120, 250):
        masks, _ = synthetic_masks(M, H, W, seed=M)
        masks_f = masks.float()
        masks_f_dev = masks_f.to(DEV)
        packed = pack_sam_masks(masks, device=DEV)
        t_cpu = timed(lambda: literal_scales(depth, masks_f, FOVX, FOVY), args.cpu_reps, sync=False)
        t_gpu = timed(lambda: literal_on(DEV, depth_dev, masks_f_dev), args.reps)
        t_bool = timed(lambda: sam_mask_scales(depth_dev, masks, FOVX, FOVY), args.reps)
        t_pk = timed(lambda: sam_mask_scales(depth_dev, packed, FOVX, FOVY), args.reps)
        ref = literal_scales(depth, masks_f, FOVX, FOVY)[2].double()
        new = sam_mask_scales(depth_dev, packed, FOVX, FOVY).cpu().double()
        ok = ~torch.isnan(ref) & (ref > 0)
        rel = float(((new[ok] - ref[ok]).abs() / ref[ok]).max())
        line = (f"{M:<5} {t_cpu:16.1f}  {t_gpu:16.2f}  {t_bool:11.2f}  {t_pk:13.3f}  {rel:12.1e}  {t_cpu / t_pk:12.0f}x  "
                f"{t_gpu / t_pk:12.0f}x")
        print(line, flush=True)
        lines.append(line)
        del masks_f_dev
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
