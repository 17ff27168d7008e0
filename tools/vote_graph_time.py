"""Timing of the vote graph at the notebook's shapes, each call beside a torch restatement of the notebook's
own expressions on the same GPU:

  * mask_features : sam_mask_features, M = 110 masks, C = 32, a 1080 x 1920 render down to 270 x 480 (masks packed beforehand);
                    torch: interpolate, conv2d >= 2, the (M, C, h, w) scale-conditioned tensor, normalize, masked mean, normalize.
  * anchor_bits   : anchor_bits, M = 110, A = 21 750, C = 32, with and without counts;
                    torch: the (M, A, C) tensor, normalize, einsum, > 0.5 (bool on the device), and the same followed by pack_bits.
  * scene_bits    : anchor_bits over a whole scene's 32 707 masks in one call (no torch side: it is the per-view one 299 times).
  * relevancy     : clip_relevancy, N = 32 707, D = 512 float16, P = 1, Q = 4; torch: normalize(float()), the (N, P, Q, 2) softmax, min.

Every case runs in a child process of its own under a time limit; the first one that fails ends the run.  A restatement that does
not fit in memory is reported as such, not shrunk.  Device events, median of --reps iterations after a warm-up.  "bytes" are the
algorithmic bytes of the call (inputs read once, outputs written once) and "HBM" the fraction of 8 TB/s they imply.

    python tools/vote_graph_time.py [--reps 20] [--out profiles/vote_graph_time.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ["mask_features", "anchor_bits", "scene_bits", "relevancy"]
CASE_SECONDS = 240
HBM_BYTES_PER_S = 8.0e12
M, C, H, W, A, N, D, P, Q = 110, 32, 1080, 1920, 21750, 32707, 512, 1, 4


def timed(fn, reps):
    import torch
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def row(case, what, ms, nbytes=None):
    tail = "" if nbytes is None else f" {nbytes / 1e6:10.2f} MB {nbytes / (ms * 1e-3) / HBM_BYTES_PER_S:7.3%} HBM"
    print(f"{case:<14} {what:<26} {ms:9.3f} ms{tail}", flush=True)


def torch_side(case, what, fn, reps):
    import torch
    try:
        row(case, what, timed(fn, reps))
    except torch.cuda.OutOfMemoryError:
        print(f"{case:<14} {what:<26} does not fit in memory", flush=True)


def run_case(case, reps):
    import torch
    import torch.nn.functional as F
    from seganygaussians_amd import _lib, vote_graph
    from seganygaussians_amd.clustering import pack_bits
    from seganygaussians_amd.contrastive_loss import pack_sam_masks
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    if case == "mask_features":
        print(f"# {_lib.load().mi_rast_version().decode()}; {torch.cuda.get_device_name(0)}; median of {reps} iterations after warm-up, "
              "device events", flush=True)
        rendered = F.normalize(torch.randn(C, H, W, generator=g), dim=0).to(dev)
        masks = torch.zeros(M, H, W, dtype=torch.bool)
        for m in range(M):   # rectangles from 1/500 to 3/20 of the image: every pixel lies in about four masks
            frac = 0.002 * (75.0 ** torch.rand(1, generator=g).item())
            dy, dx = max(int(H * frac ** 0.5), 2), max(int(W * frac ** 0.5), 2)
            y0, x0 = torch.randint(0, H - dy + 1, (1,), generator=g).item(), torch.randint(0, W - dx + 1, (1,), generator=g).item()
            masks[m, y0:y0 + dy, x0:x0 + dx] = True
        gates = torch.sigmoid(torch.randn(M, C, generator=g)).to(dev)
        packed = pack_sam_masks(masks, device=dev)
        masks_dev = masks.to(dev)
        h, w = H // 4, W // 4
        _, counts = vote_graph.sam_mask_features(rendered, packed, gates, return_counts=True)
        print(f"# masks cover {counts.sum().item() / (h * w):.2f} x the {h} x {w} working image", flush=True)
        nbytes = 4 * C * H * W + 8 * M * H * ((W + 63) // 64) + 8 * M * C
        row(case, "sam_mask_features", timed(lambda: vote_graph.sam_mask_features(rendered, packed, gates), reps), nbytes)

        def notebook():
            f = F.interpolate(rendered[None], (h, w), mode="bilinear")[0]
            sm = F.interpolate(masks_dev[:, None].float(), (h, w), mode="bilinear")
            sm = torch.conv2d(sm, torch.ones(1, 1, 3, 3, device=dev), padding=1) >= 2
            sc = F.normalize(f[None] * gates[:, :, None, None], dim=1)
            feat = (sc * sm).sum(dim=(2, 3)) / (sm.sum(dim=(2, 3)) + 1e-9)
            return F.normalize(feat, dim=-1)
        torch_side(case, "torch (M, C, h, w)", notebook, reps)
    elif case in ("anchor_bits", "scene_bits"):
        rows = M if case == "anchor_bits" else N
        ctr = F.normalize(torch.randn(8, C, generator=g), dim=-1)
        anchors = (ctr[torch.arange(A) % 8] + 0.4 * torch.randn(A, C, generator=g) / C ** 0.5).to(dev)
        gates = torch.sigmoid(torch.randn(rows, C, generator=g)).to(dev)
        phi = F.normalize(gates.cpu() * (ctr[torch.arange(rows) % 8] + 0.4 * torch.randn(rows, C, generator=g) / C ** 0.5), dim=-1).to(dev)
        words = (A + 31) // 32
        out = torch.empty(rows, words, dtype=torch.int32, device=dev)
        nbytes = 4 * C * (A + 2 * rows) + 4 * rows * words
        row(case, f"anchor_bits M = {rows}", timed(lambda: vote_graph.anchor_bits(phi, gates, anchors, out=out), reps), nbytes)
        row(case, "  with counts", timed(lambda: vote_graph.anchor_bits(phi, gates, anchors, out=out, return_counts=True), reps), nbytes + 4 * rows)
        if case == "anchor_bits":
            def notebook():
                sa = F.normalize(gates[:, None, :] * anchors[None], dim=-1)
                return torch.einsum("mac,mc->ma", sa, phi) > 0.5
            torch_side(case, "torch (M, A, C) -> bool", notebook, reps)
            torch_side(case, "torch ... -> pack_bits", lambda: pack_bits(notebook()), reps)
    elif case == "relevancy":
        embeds = torch.randn(N, D, generator=g).half().to(dev)
        pos = F.normalize(torch.randn(P, D, generator=g), dim=-1).to(dev)
        neg = F.normalize(torch.randn(Q, D, generator=g), dim=-1).to(dev)
        nbytes = 2 * N * D + 4 * (P + Q) * D + 4 * N * P
        row(case, "clip_relevancy f16", timed(lambda: vote_graph.clip_relevancy(embeds, pos, neg), reps), nbytes)
        e32 = embeds.float()
        row(case, "clip_relevancy f32", timed(lambda: vote_graph.clip_relevancy(e32, pos, neg), reps), nbytes + 2 * N * D)

        def notebook():
            e = F.normalize(embeds.float(), dim=-1)
            p, q = e @ pos.T, e @ neg.T
            pairs = torch.stack([p[:, :, None].expand(-1, -1, Q), q[:, None, :].expand(-1, P, -1)], dim=-1)
            return torch.softmax(10 * pairs, dim=-1)[..., 0].min(dim=2).values
        torch_side(case, "torch (N, P, Q, 2)", notebook, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", choices=CASES, default=None, help="run one case in this process (what the parent starts)")
    args = ap.parse_args()
    assert args.reps >= 10
    if args.case:
        run_case(args.case, args.reps)
        return 0
    lines = []
    for case in CASES:
        try:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(args.reps)], cwd=ROOT,
                                  stdout=subprocess.PIPE, text=True, timeout=CASE_SECONDS)
        except subprocess.TimeoutExpired as e:
            print(e.stdout or "", f"{case}: no result within {CASE_SECONDS} s; stopping", sep="\n", flush=True)
            return 1
        print(done.stdout, end="", flush=True)
        if done.returncode != 0:
            print(f"{case}: exit status {done.returncode}; stopping", flush=True)
            return 1
        lines += done.stdout.splitlines()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
