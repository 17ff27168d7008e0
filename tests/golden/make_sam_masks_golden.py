"""Writes tests/golden/sam_masks/sam_masks.npz: selections of the reference's own mask_nms (clip_utils/sam_utils.py:123-187) on
seeded mask sets, for tests/test_sam_masks_host.py (the restatement) and tests/test_sam_masks.py (the kernels).

Run where the reference sources are (tests/reference_helpers.py: REF_ROOT); not part of the tests:

    python tests/golden/make_sam_masks_golden.py [--reference <checkout>]

The reference module imports cv2 and segment_anything at its top, so only the one function is taken: the file is parsed, the
mask_nms definition is compiled at run time in a namespace that holds torch, and nothing of its text is kept.

Per case: M in 2 .. 70 masks on a 24 x (70 .. 130) image -- rectangles, near-copies, small parts and supersets of earlier masks,
now and then an empty one --, distinct scores, and one of the reference's two threshold sets (the defaults; 0.8 / 0.7 / 0.5 of
sam_utils.py:210).  A case in which the reference raises (the keep_conf[index, 0] of its fallbacks, :173-181) is left out and
counted.  Asserted here: at most 10 % of the drawn cases left out, at least 60 kept; the restatement (tests/sam_masks_ref.py) agrees
on every kept case; each of the four tests is the sole reason for at least one rejection; at least one mask is kept and one dropped
in at least half the cases."""
import argparse
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import reference_helpers as rh  # noqa: E402
from tests.sam_masks_ref import load_cases, nms_tests_ref, overlaps_ref  # noqa: E402

THRESHOLDS = [(0.7, 0.1, 0.2), (0.8, 0.7, 0.5)]   # (iou_thr, score_thr, inner_thr): the defaults, and sam_utils.py:210
DRAWN = 72
H = 24


def reference_mask_nms(reference_root):
    path = os.path.join(reference_root, "clip_utils", "sam_utils.py")
    tree = ast.parse(open(path).read(), path)
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "mask_nms")
    ns = {"torch": torch}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns["mask_nms"]


def rectangle(rng, W, min_side=2):
    h = int(rng.integers(min_side, H + 1))
    w = int(rng.integers(min_side, W // 2 + 1))
    y0, x0 = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
    m = np.zeros((H, W), bool)
    m[y0:y0 + h, x0:x0 + w] = True
    return m


def draw_case(rng):
    M, W = int(rng.integers(2, 71)), int(rng.integers(70, 131))
    masks = [rectangle(rng, W)]
    while len(masks) < M:
        kind = rng.random()
        src = masks[int(rng.integers(0, len(masks)))]
        if kind < 0.35 or not src.any():
            m = rectangle(rng, W)
        elif kind < 0.55:      # a near-copy: a few pixels flipped
            m = src.copy()
            flips = int(rng.integers(1, max(2, src.sum() // 8)))
            m.reshape(-1)[rng.integers(0, H * W, flips)] ^= True
        elif kind < 0.78:      # a small part of an earlier mask, sometimes with a few pixels outside it
            ys, xs = np.nonzero(src)
            cy, cx = ys[int(rng.integers(0, ys.size))], xs[int(rng.integers(0, xs.size))]
            m = np.zeros((H, W), bool)
            m[max(0, cy - int(rng.integers(0, 4))): cy + int(rng.integers(1, 5)), max(0, cx - int(rng.integers(0, 6))): cx + int(rng.integers(1, 7))] = True
            if rng.random() < 0.6:
                m &= src
            if not m.any():
                m[cy, cx] = True
        elif kind < 0.97:      # a superset of an earlier mask
            m = src | rectangle(rng, W, min_side=4)
        else:
            m = np.zeros((H, W), bool)
        masks.append(m)
    masks = np.stack(masks)[rng.permutation(M)]
    scores = rng.permutation(np.linspace(0.02, 0.99, 97, dtype=np.float32))[:M] + rng.random(M, dtype=np.float32) * np.float32(0.004)
    assert len(np.unique(scores)) == M
    return masks, scores.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=rh.REF_ROOT)
    ap.add_argument("--out", default=os.path.join(HERE, "sam_masks", "sam_masks.npz"))
    args = ap.parse_args()
    ref_nms = reference_mask_nms(args.reference)
    rng = np.random.default_rng(20241)
    bits, shapes, all_scores, thrs, sels, kept_cases, left_out, mixed = [], [], [], [], [], 0, 0, 0
    sole = {"iou": 0, "score": 0, "inner_u": 0, "inner_l": 0}
    for c in range(DRAWN):
        masks, scores = draw_case(rng)
        thr = THRESHOLDS[c % 2]
        try:
            sel = ref_nms(torch.from_numpy(masks), torch.from_numpy(scores), iou_thr=thr[0], score_thr=thr[1], inner_thr=thr[2])
        except (IndexError, RuntimeError):
            left_out += 1
            continue
        sel = sel.numpy().astype(np.int64)
        s, idx = torch.sort(torch.from_numpy(scores), descending=True, stable=True)
        inter, areas = overlaps_ref(masks, idx.numpy())
        tests = np.stack(nms_tests_ref(inter, areas, s.numpy(), *thr))
        assert np.array_equal(idx.numpy()[tests.all(axis=0)], sel), f"case {c}: the restatement differs from the reference"
        for name, row in zip(sole, range(4)):
            sole[name] += int((~tests[row] & np.delete(tests, row, axis=0).all(axis=0)).sum())
        mixed += int(0 < len(sel) < len(scores))
        bits.append(np.packbits(masks.reshape(-1)))
        shapes.append(masks.shape)
        all_scores.append(scores)
        thrs.append(thr)
        sels.append(sel)
        kept_cases += 1
    # few arrays, the cases back to back (tests/sam_masks_ref.py:load_cases cuts them apart): a zip member per case would outweigh its data
    data = dict(mask_bits=np.concatenate(bits), shapes=np.asarray(shapes, np.int32), scores=np.concatenate(all_scores),
                thresholds=np.asarray(thrs, np.float64), selected=np.concatenate(sels).astype(np.int16),
                selected_len=np.asarray([len(x) for x in sels], np.int32))
    print(f"drawn {DRAWN}, kept {kept_cases}, left out (the reference raised) {left_out}; sole reasons {sole}; mixed {mixed}")
    assert left_out * 10 <= DRAWN and kept_cases >= 60
    assert all(v >= 1 for v in sole.values()), sole
    assert mixed * 2 >= kept_cases
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **data)
    back = load_cases(args.out)
    assert len(back) == kept_cases and all(np.array_equal(a[3], b) for a, b in zip(back, sels))
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
