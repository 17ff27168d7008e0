"""Plain numpy / torch restatement of seganygaussians_amd/clip_tiles.py and of resize_sam_masks / mask_index_map
(seganygaussians_amd/sam_masks.py), for the tests.  Runs anywhere.

What it restates, by the reference's lines:
  * clip_utils/__init__.py:99-102  the masks interpolated bilinearly to the image's size as floats; above 0.5 is 1, the rest 0
  * :108        the masked images in float32: the image where the mask is 1, 255 x background where it is 0
  * :115, :157  torchvision's masks_to_boxes, truncated to integers
  * :168        the slice rows y_min .. y_max - 1, columns x_min .. x_max - 1: the box's last row and column are left out
  * :173        the crop, channels first, divided by 255, goes to the encoder; clip_utils/clip_utils.py:60-68 resizes it to
                224 x 224 and normalises it with the CLIP constants
  * clip_utils/sam_utils.py:99-104  get_seg_img: pixels outside the segmentation set to 0, then the bbox (x, y, w, h) cut out
  * :106-114    pad_img: a zero square of side max(w, h); the crop at column (h - w) // 2 if h > w, else at row (w - h) // 2
  * :214, :221  the seg_map starts at -1 and takes i wherever mask i is set, in ascending i; :62 adds the earlier levels' lengths
                to every value but -1

The weight tables are computed in float32, one IEEE operation per step (numpy float32 scalars and arrays round every operation
separately), as include/mi_clip_tiles.h states them; tiles_ref64 contracts the exact float32 planes with those float32 weights in
float64, so what is left between it and the kernel is the kernel's float32 summation alone."""
import os

import numpy as np
import torch

from tests.sam_masks_ref import boxes_ref  # noqa: F401  (torchvision.ops.masks_to_boxes, NaN rows for empty masks)

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_tiles", "clip_tiles.npz")
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)   # clip_utils/clip_utils.py:64
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)   # clip_utils/clip_utils.py:65
MAX_SIDE = 32768


def load_cases(path=GOLDEN):
    """The fixture of tests/golden/make_clip_tiles_golden.py as a list of dicts: image uint8 (H, W, 3), masks bool (M, h, w),
    background float, crops: M float32 arrays (3, ch, cw), what the reference handed to encode_image (without the batch axis)."""
    z = np.load(path)
    cases, i0, b0, c0, k0 = [], 0, 0, 0, 0
    for (H, W), (M, h, w), bg in zip(z["image_shapes"], z["mask_shapes"], z["backgrounds"]):
        H, W, M, h, w = int(H), int(W), int(M), int(h), int(w)
        image = z["images"][i0:i0 + H * W * 3].reshape(H, W, 3)
        nbytes = (M * h * w + 7) // 8
        masks = np.unpackbits(z["mask_bits"][b0:b0 + nbytes])[: M * h * w].reshape(M, h, w).astype(bool)
        crops = []
        for ch, cw in z["crop_shapes"][k0:k0 + M]:
            n = 3 * int(ch) * int(cw)
            crops.append(z["crops"][c0:c0 + n].reshape(3, int(ch), int(cw)))
            c0 += n
        cases.append(dict(image=image, masks=masks, background=float(bg), crops=crops))
        i0, b0, k0 = i0 + H * W * 3, b0 + nbytes, k0 + M
    return cases


# ---- masks: resize, boxes, rectangles, index map ----------------------------------------------------------------------------------

def resize_masks_ref(masks, size, threshold=0.5):
    """:99-102 on the CPU: bool (M, H, W)."""
    m = torch.as_tensor(np.asarray(masks, dtype=bool))
    return (torch.nn.functional.interpolate(m.unsqueeze(0).float(), tuple(size), mode="bilinear").squeeze(0) > threshold).numpy()


def resize_values64(masks, size):
    """The same interpolation in float64 (M, H, W): how far every value is from the threshold."""
    m = torch.as_tensor(np.asarray(masks, dtype=bool))
    return torch.nn.functional.interpolate(m.unsqueeze(0).double(), tuple(size), mode="bilinear").squeeze(0).numpy()


def rects_ref(masks, inclusive=False):
    """(rects (M, 4) int64 half-open [X0, Y0, X1, Y1), valid (M,) bool) from the masks' boxes: :157 and :168 slice
    [x_min, x_max) x [y_min, y_max); inclusive keeps the box's last row and column.  An invalid mask has the empty rectangle."""
    boxes = boxes_ref(masks)
    rects = np.nan_to_num(boxes, nan=0.0).astype(np.int64)
    if inclusive:
        rects[:, 2:] += 1
    return mark_valid(rects, np.asarray(masks, dtype=bool).reshape(len(boxes), -1).any(axis=1))


def mark_valid(rects, has_pixel):
    rects = np.asarray(rects, dtype=np.int64).copy()
    side = rects[:, 2:] - rects[:, :2]
    valid = has_pixel & (side >= 1).all(axis=1) & (side <= MAX_SIDE).all(axis=1)
    rects[~valid] = 0
    return rects, valid


def index_map_ref(masks, offset=0):
    """sam_utils.py:214, :221 and :62: the numpy loop."""
    m = np.asarray(masks, dtype=bool)
    seg_map = -np.ones(m.shape[1:], dtype=np.int32)
    for i in range(m.shape[0]):
        seg_map[m[i]] = i
    seg_map[seg_map != -1] += offset
    return seg_map


# ---- the source plane, exact in float32 ----------------------------------------------------------------------------------------

def background_f32(background):
    return F32(F32(255.0 * background) / F32(255.0))


def plane_ref(image, mask, rect, layout="crop", background=None):
    """The float32 plane (PH, PW, 3) the resize reads: image / 255 where the mask has its bit, the background value elsewhere --
    outside the image and, for "pad_square", around the crop."""
    if background is None:
        background = {"crop": 1.0, "pad_square": 0.0}[layout]
    bg = background_f32(background)
    image, mask = np.asarray(image), np.asarray(mask, dtype=bool)
    H, W = mask.shape
    X0, Y0, X1, Y1 = (int(v) for v in rect)
    cw, ch = X1 - X0, Y1 - Y0
    assert cw >= 1 and ch >= 1
    crop = np.full((ch, cw, 3), bg, F32)
    ys, xs = np.arange(Y0, Y1), np.arange(X0, X1)
    yin, xin = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
    sub_img = image[np.ix_(ys[yin], xs[xin])].astype(F32) / F32(255.0)
    sub_mask = mask[np.ix_(ys[yin], xs[xin])]
    inner = crop[np.ix_(yin, xin)]
    inner[sub_mask] = sub_img[sub_mask]
    crop[np.ix_(yin, xin)] = inner
    if layout == "crop":
        return crop
    assert layout == "pad_square"
    L = max(ch, cw)
    plane = np.full((L, L, 3), bg, F32)
    if ch > cw:
        plane[:, (L - cw) // 2:(L - cw) // 2 + cw] = crop
    else:
        plane[(L - ch) // 2:(L - ch) // 2 + ch] = crop
    return plane


# ---- the two weight tables, float32 arithmetic -------------------------------------------------------------------------------

def aa_weights(n_in, n_out):
    """_upsample_bilinear2d_aa's weights in float32: a list over the output index of (xmin, float32 weights of xmin .. xmax - 1)."""
    scale = F32(n_in) / F32(n_out)
    support = scale if scale >= F32(1.0) else F32(1.0)
    inv = F32(1.0) / scale if scale >= F32(1.0) else F32(1.0)
    table = []
    for i in range(n_out):
        center = scale * (F32(i) + F32(0.5))
        xmin = max(0, int((center - support) + F32(0.5)))
        xmax = min(int((center + support) + F32(0.5)), n_in)
        j = np.arange(xmin, xmax).astype(F32)
        w = np.maximum(F32(0.0), F32(1.0) - np.abs(((j - center) + F32(0.5)) * inv)).astype(F32)
        total = F32(0.0)
        for v in w:
            total = F32(total + v)   # the sequential float32 sum
        table.append((xmin, (w / total).astype(F32)))
    return table


def linear_weights(n_in, n_out):
    """upsample_bilinear2d's two taps (align_corners=False) as ATen computes them for float32 -- pm_source_taps of
    csrc/packed_masks.h: src = max(fma(scale, dst + 0.5, -0.5), 0).  (The product of two float32 numbers, one of them a small integer
    + 0.5, minus 0.5 is exact in float64, so one rounding of the float64 result is the fused operation.)  The same list form as
    aa_weights: (i0, [l0, l1]), or (i0, [l0 + l1]) where the two taps coincide."""
    scale = F32(n_in) / F32(n_out)
    table = []
    for d in range(n_out):
        src = max(F32(np.float64(scale) * (d + 0.5) - 0.5), F32(0.0))
        i0 = min(int(np.floor(src)), n_in - 1)
        lam = min(max(F32(src - F32(i0)), F32(0.0)), F32(1.0))
        l0, l1 = F32(F32(1.0) - lam), lam
        table.append((i0, np.asarray([l0, l1], F32)) if i0 < n_in - 1 else (i0, np.asarray([np.float64(l0) + np.float64(l1)])))
    return table


def weights(n_in, n_out, antialias):
    return aa_weights(n_in, n_out) if antialias else linear_weights(n_in, n_out)


def dense(table, n_in):
    """(n_out, n_in) float64 matrix of a weight table, and the number of taps of every output index."""
    Wm = np.zeros((len(table), n_in), np.float64)
    for i, (lo, w) in enumerate(table):
        Wm[i, lo:lo + len(w)] += np.asarray(w, np.float64)
    return Wm, np.asarray([max(len(w), 2) for _, w in table])


def resize_ref64(plane, size, antialias):
    """(3, Sh, Sw) float64: the float32 plane contracted with the float32 weights in float64; and the tap counts (n_y (Sh,),
    n_x (Sw,))."""
    PH, PW = plane.shape[:2]
    Wy, n_y = dense(weights(PH, size[0], antialias), PH)
    Wx, n_x = dense(weights(PW, size[1], antialias), PW)
    return np.einsum("yp,pqc,xq->cyx", Wy, plane.astype(np.float64), Wx), n_y, n_x


def tiles_ref64(plane, size=(224, 224), antialias=True, mean=CLIP_MEAN, std=CLIP_STD):
    """(want (3, Sh, Sw) float64, bound (3, Sh, Sw) float64 for a float32 result).  The normalisation uses the float32 values of mean
    and std, which are what the kernel is given, in float64 arithmetic.

    The bound: plane values lie in [0, 1] and the weights are non-negative and sum to 1 within rounding, so every partial sum is at
    most 1 + O(2^-24).  A float32 sum of n products errs by at most n roundings of the products and n of the sums, 2 n 2^-24; the
    weights' own division adds one rounding each, which the "+ 4" covers together with the float32 taps' sum not being exactly 1.
    The width pass (n_x taps) feeds the height pass (n_y taps, weights summing to 1), so the resized value errs by at most
    2 (n_x + n_y + 4) 2^-24, and after (r - mean) / std by that / std plus two roundings of the result, 2^-23 |want|."""
    r, n_y, n_x = resize_ref64(plane, size, antialias)
    mean64 = np.asarray(mean, F32).astype(np.float64)[:, None, None]
    std64 = np.asarray(std, F32).astype(np.float64)[:, None, None]
    want = (r - mean64) / std64
    bound = 2.0 * (n_x[None, None, :] + n_y[None, :, None] + 4) * 2.0 ** -24 / np.abs(std64) + 2.0 ** -23 * np.abs(want)
    return want, bound


def half_bound(want, bound):
    """The bound for a float16 result: one more rounding, 2^-11 |want|."""
    return bound + 2.0 ** -11 * np.abs(want)


def tiles_interpolate(plane, size=(224, 224), antialias=True, mean=CLIP_MEAN, std=CLIP_STD):
    """The reference's operation itself on the CPU: torchvision's Resize on a tensor is F.interpolate(mode='bilinear',
    align_corners=False, antialias=...); then Normalize, (r - mean) / std in float32.  (3, Sh, Sw) float32."""
    x = torch.from_numpy(np.ascontiguousarray(plane)).permute(2, 0, 1)[None]
    r = torch.nn.functional.interpolate(x, tuple(size), mode="bilinear", align_corners=False, antialias=antialias)[0]
    m = torch.tensor(mean, dtype=torch.float32)[:, None, None]
    s = torch.tensor(std, dtype=torch.float32)[:, None, None]
    return ((r - m) / s).numpy()


def normalised_background(background, mean=CLIP_MEAN, std=CLIP_STD):
    """(3,) float32: what every element of an invalid mask's tile holds."""
    return ((background_f32(background) - np.asarray(mean, F32)) / np.asarray(std, F32)).astype(F32)
