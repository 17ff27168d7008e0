"""Writes tests/golden/clip_tiles/clip_tiles.npz: the crops the reference's own get_features_from_image_and_masks
(clip_utils/__init__.py:91-191) hands to the CLIP encoder on seeded images and masks, for tests/test_clip_tiles_host.py (the
restatement) and tests/test_clip_tiles.py (the kernels).

Run where the reference sources are (tests/reference_helpers.py: REF_ROOT); not part of the tests:

    MPLBACKEND=Agg python tests/golden/make_clip_tiles_golden.py [--reference <checkout>]

The reference module imports open_clip and torchvision at its top, so only the one function is taken: the file is parsed, the
definition of get_features_from_image_and_masks is compiled at run time in a namespace that holds torch, np, a dummy
OpenCLIPNetwork and a torchvision stand-in whose ops.masks_to_boxes is the restatement's, and nothing of its text is kept.  While
it runs Tensor.cuda is the identity (the function moves each crop to the GPU before the encoder), restored afterwards.  The
clip_model is a stub whose encode_image records its argument, the (1, 3, ch, cw) float32 crop / 255.

Per case: a 24 x (70 .. 130) x 3 uint8 image, 2 .. 8 masks (rectangles with holes punched in), at the image's size in the even
cases and at half size in the odd ones, so that the interpolation of :99 does work; backgrounds 1.0, 0.0, 0.5 in turn.  No case is
left out: every mask is drawn again until its resampled version spans at least two rows and two columns (asserted), so the
reference never meets an empty crop.  Asserted too: the restatement (tests/clip_tiles_ref.py) reproduces every crop bit for bit.
The file holds data only: images, mask bits, backgrounds, crops and their shapes."""
import argparse
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import clip_tiles_ref as ref  # noqa: E402
from tests import reference_helpers as rh  # noqa: E402

CASES = 12
H = 24
BACKGROUNDS = (1.0, 0.0, 0.5)


def reference_function(reference_root):
    path = os.path.join(reference_root, "clip_utils", "__init__.py")
    tree = ast.parse(open(path).read(), path)
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "get_features_from_image_and_masks")
    boxes = lambda masks: torch.from_numpy(ref.boxes_ref(masks.numpy() != 0))
    ns = {"torch": torch, "np": np, "OpenCLIPNetwork": type("OpenCLIPNetwork", (), {}),
          "torchvision": types.SimpleNamespace(ops=types.SimpleNamespace(masks_to_boxes=boxes))}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns["get_features_from_image_and_masks"]


class Recorder:
    def __init__(self):
        self.seen = []

    def encode_image(self, x):
        assert x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] == 1 and x.shape[1] == 3
        self.seen.append(x[0].numpy().copy())
        return torch.zeros(1, 4)


def draw_mask(rng, h, w, size):
    """A rectangle with holes at (h, w) whose version resampled to `size` spans at least two rows and two columns."""
    while True:
        mh, mw = int(rng.integers(2, h // 2 + 2)), int(rng.integers(3, w // 2 + 1))
        y0, x0 = int(rng.integers(0, h - mh + 1)), int(rng.integers(0, w - mw + 1))
        m = np.zeros((h, w), bool)
        m[y0:y0 + mh, x0:x0 + mw] = rng.random((mh, mw)) < 0.8
        up = ref.resize_masks_ref(m[None], size)[0]
        ys, xs = np.nonzero(up)
        if ys.size and ys.max() > ys.min() and xs.max() > xs.min():
            return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=rh.REF_ROOT)
    ap.add_argument("--out", default=os.path.join(HERE, "clip_tiles", "clip_tiles.npz"))
    args = ap.parse_args()
    fn = reference_function(args.reference)
    rng = np.random.default_rng(20242)
    images, image_shapes, bits, mask_shapes, backgrounds, crops, crop_shapes = [], [], [], [], [], [], []
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        for c in range(CASES):
            W, M = int(rng.integers(70, 131)), int(rng.integers(2, 9))
            h, w = (H, W) if c % 2 == 0 else (H // 2, W // 2)
            image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            masks = np.stack([draw_mask(rng, h, w, (H, W)) for _ in range(M)])
            background = BACKGROUNDS[c % 3]
            rec = Recorder()
            fn(rec, image, torch.from_numpy(masks), background=background)
            assert len(rec.seen) == M
            up = ref.resize_masks_ref(masks, (H, W))
            rects, valid = ref.rects_ref(up)
            assert valid.all()
            for m in range(M):
                want = ref.plane_ref(image, up[m], rects[m], "crop", background).transpose(2, 0, 1)
                assert want.shape[1] >= 1 and want.shape[2] >= 1
                assert want.shape == rec.seen[m].shape and np.array_equal(want, rec.seen[m]), f"case {c} mask {m}: the restatement differs"
                crops.append(rec.seen[m].reshape(-1))
                crop_shapes.append(rec.seen[m].shape[1:])
            images.append(image.reshape(-1))
            image_shapes.append((H, W))
            bits.append(np.packbits(masks.reshape(-1)))
            mask_shapes.append(masks.shape)
            backgrounds.append(background)
    finally:
        torch.Tensor.cuda = cuda
    # few arrays, the cases back to back (tests/clip_tiles_ref.py:load_cases cuts them apart)
    data = dict(images=np.concatenate(images), image_shapes=np.asarray(image_shapes, np.int32), mask_bits=np.concatenate(bits),
                mask_shapes=np.asarray(mask_shapes, np.int32), backgrounds=np.asarray(backgrounds, np.float64),
                crops=np.concatenate(crops).astype(np.float32), crop_shapes=np.asarray(crop_shapes, np.int32))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **data)
    back = ref.load_cases(args.out)
    assert len(back) == CASES and sum(len(b["crops"]) for b in back) == len(crop_shapes)
    k = 0
    for b in back:
        for crop in b["crops"]:
            assert np.array_equal(crop.reshape(-1), crops[k])
            k += 1
    size = os.path.getsize(args.out)
    print(f"{CASES} cases, {len(crop_shapes)} crops;", args.out, size, "bytes")
    assert size <= 668 * 1024


if __name__ == "__main__":
    main()
