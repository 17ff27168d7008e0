"""Designed edge scenes, decision margins and the per-group tolerance rule of the rasterizer's edge tests
(tests/test_raster_edges_host.py on the CPU, tests/test_raster_edges.py on the GPU).

The rule is the one of tests/edge_ref.py, applied per GROUP -- the image per pixel (all channels), final_T / out mask / out depth
per pixel, every gradient per Gaussian row -- against the dense float64 autograd reference of tests/dense_ref.py evaluated with
reference_quirks=True on the float32 input values:

    E32   = max(|oracle - dense64|, |dense32 - dense64|)                                  over the group
    bound = max(FACTOR * E32, FLOOR * magnitude of the terms summed into the group)
    every non-excused group:  |product - dense64| <= bound;  a group dense64 leaves at exactly zero is exactly zero, and the reverse.

Magnitude of the terms of a gradient row: the loss is split by 4 x 4 pixel blocks (8 x 8 on the many-tile scenes), each block's
float64 gradient is taken on its own and the absolute values are added (a lower bound of the true sum of term magnitudes: the
floor can only be too strict).  Of a pixel: sum_g w_g |c_g| + T |bg| from the dense weights.

The fp64 reference and a float32 kernel must take the same discrete decisions; a pixel in which a pair sits within a MARGIN of a
decision is excused, with every Gaussian blended there.  The designed classes are never excused and at most EXCUSED_GAUSSIANS /
EXCUSED_PIXELS of a scene may be (asserted on the CPU, tests/test_raster_edges_host.py).
"""
from __future__ import annotations

import math
import os
import re
from collections import namedtuple

import numpy as np
import torch

from oracle import saga_oracle as so
from seganygaussians_amd import scenes
from tests.dense_ref import build_rotation, render_dense

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "seganygaussians_amd", "csrc")


def _constant(header, name):
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, open(os.path.join(_CSRC, header)).read())
    assert m, (header, name)
    return int(m.group(1))


# batch sizes of the blend kernels, read from the headers that define them
XG = _constant("blend_fwd_split.h", "XG")      # Gaussians per MFMA group of the wave-per-quadrant forward
CHK = _constant("blend_bwd_shared.h", "CHK")   # rows per MFMA chunk of the backward kernels
FB = _constant("blend_fwd.h", "FB")            # blend-list records per forward batch
XB = _constant("blend_fwd_x3.h", "XB")         # blend-list records per batch of the tile-batched forward
ROWS = _constant("blend_bwd.h", "ROWS")        # survivor rows resident in LDS at a time in the backward
RUN_CAP = _constant("mi_rast.hip", "RUN_MODEL_CAP")   # range scan: XCD runs of equal sum(min(list length, RUN_CAP) + RUN_FIX)
RUN_FIX = _constant("mi_rast.hip", "RUN_MODEL_FIX")
LIST_LENGTHS = tuple(sorted({n + d for n in (XG, CHK, 64, FB, XB, ROWS) for d in (-1, 0, 1)}))

EXCUSED_GAUSSIANS = 2
EXCUSED_PIXELS = 4

# ---- the calibrated rule -------------------------------------------------------------------------------------------------------
# FACTOR and FLOOR per class, calibrated on the CPU by `python -m tests.raster_edge_ref` against the two float32 restatements
# (the oracle judged with E32 = |dense32 - dense64| alone, dense32 judged with E32 = |oracle - dense64| alone) over every scene
# and variant of all_cases(), never against the product: powers of two, FACTOR = 4 * 2^k and FLOOR = 2^(k - 22) with the
# smallest k for which both pass, then FLOOR lowered as far as it still passes (the floor is the part of the bound that does not
# follow the row), then FACTOR; then FACTOR doubled once, the product being a third
# rounding order (f32 atomics, fma contraction, split-bf16 MFMA sums).  A class that needs FACTOR > 256 is too ill-conditioned to
# test anything: its scene is softened instead.  MUTUAL holds the undoubled pair and the worst mutual error / bound measured with
# it; tests/test_raster_edges_host.py re-asserts that check.
MUTUAL = {
    # class: (FACTOR, log2 FLOOR, worst mutual error / bound)
    "image": (4.0, -19, 0.997),
    "final_T": (4.0, -21, 0.82),
    "out_mask": (4.0, -20, 0.734),
    "out_depth": (4.0, -20, 0.885),
    "dL_dcolors": (32.0, -19, 0.944),
    "dL_dsh": (16.0, -21, 0.91),
    "dL_dmask": (4.0, -18, 0.54),
    "dL_dmeans2D": (32.0, -18, 0.764),
    "dL_dopacity": (64.0, -18, 0.862),
    "dL_dmeans3D": (32.0, -21, 0.831),
    "dL_dcov3D": (16.0, -21, 0.857),
    "dL_dscales": (256.0, -22, 0.798),
    "dL_drotations": (256.0, -22, 0.656),
}

# The same procedure (calibrate(), unchanged) run over tile_cases() alone: the many-tile scenes "tiles" below (97 x 33 and 177 x 17)
# have lists of 200 and more entries in one tile of many, a Gaussian summed from every tile, walks that end early and centres at
# x = 90 to 170, and the two float32 restatements differ by more there than MUTUAL allows (judged against each other with MUTUAL
# they reach 2 to 12 times the bound for final_T and the image).  Worst mutual error / bound under MUTUAL_TILES: 0.986.
# MUTUAL and all_cases() stay as they are; rule() picks the table by the case's scene kind.
MUTUAL_TILES = {
    # class: (FACTOR, log2 FLOOR, worst mutual error / bound)
    "image": (64.0, -21, 0.955),
    "final_T": (4.0, -19, 0.866),
    "out_mask": (16.0, -19, 0.974),
    "out_depth": (4.0, -19, 0.82),
    "dL_dcolors": (128.0, -22, 0.686),
    "dL_dsh": (64.0, -22, 0.744),
    "dL_dmask": (128.0, -22, 0.831),
    "dL_dmeans2D": (256.0, -22, 0.676),
    "dL_dopacity": (16.0, -15, 0.674),
    "dL_dmeans3D": (128.0, -17, 0.986),
    "dL_dscales": (128.0, -22, 0.812),
    "dL_drotations": (128.0, -18, 0.764),
}
TABLES = {"edge": MUTUAL, "list": MUTUAL, "tiles": MUTUAL_TILES}


def rule(cls, scene="edge"):
    """(FACTOR, FLOOR) the product is judged with, on a case of scene kind `scene`."""
    f, lf, _ = TABLES[scene][cls]
    return 2.0 * f, 2.0 ** lf


def mutual_rule(cls, scene="edge"):
    f, lf, _ = TABLES[scene][cls]
    return f, 2.0 ** lf


# ---- scenes ----------------------------------------------------------------------------------------------------------------------

Variant = namedtuple("Variant", "colors mask mask_only cov modifier bg P kind L", defaults=("precomp", False, False, False, 1.0,
                                                                                            "zero", 96, None, None))
# colors: "precomp" | "sh0" | "sh3";  kind / L: the list-length scene ("contrib" | "raw", length), or kind "t1" | "t2" of the
# many-tile scenes;  P: total number of Gaussians (designed + make_scene fill) of the edge and many-tile scenes, or "culled" for
# the scene in which every Gaussian is behind the near plane.

NEAR = np.float32(0.2)


class _Builder:
    def __init__(self, W, H, focal, rng=None):
        self.W, self.H, self.f, self.rng = W, H, focal, rng
        self.cx, self.cy = (W - 1) * 0.5, (H - 1) * 0.5
        self.rows, self.k = [], 0

    def depth(self):
        self.k += 1
        return 2.0 + 0.04 * self.k

    def add(self, cls, u, v, z=None, sig=2.5, q=(1.0, 0.0, 0.0, 0.0), op=0.5, scale=None, exact=False):
        """Centre at pixel coordinates (u, v) (the camera is the identity: px = focal x / z + (W - 1) / 2), view depth z, screen-space
        sigma `sig` pixels per axis (or the world scales `scale`).  Unless `exact`, the centre is moved by up to 0.2 px with the
        scene's seed, so that a seed can be chosen for which no pair of the class sits on a decision."""
        if not exact and self.rng is not None:
            u, v = u + self.rng.uniform(-0.2, 0.2), v + self.rng.uniform(-0.2, 0.2)
        z = self.depth() if z is None else z
        s = np.broadcast_to(np.asarray(sig, np.float64), (3,)) * float(z) / self.f if scale is None else np.broadcast_to(scale, (3,))
        self.rows.append((cls, ((u - self.cx) * float(z) / self.f, (v - self.cy) * float(z) / self.f, z), tuple(s), tuple(q), op))


def _designed(W, H, focal, seed):
    b = _Builder(W, H, focal, np.random.default_rng(seed + 9000))
    qz = lambda deg: (math.cos(math.radians(deg) / 2), 0.0, 0.0, math.sin(math.radians(deg) / 2))
    # placement
    b.add("pixel_centre", W // 3, H // 3, exact=True)
    b.add("tile_corner", 16, 16, exact=True)
    b.add("tile_corner", 15.5, 15.5, sig=1.5, exact=True)
    b.add("last_pixel", W - 1, H - 1, exact=True)
    for u, v in ((-0.5, b.cy + 0.3), (W - 0.5, b.cy - 0.3), (b.cx + 0.3, -0.5), (b.cx - 0.3, H - 0.5)):
        b.add("border_half_out", u, v, sig=1.5, exact=True)
    # off-image centres, 3-sigma radius reaching in
    for u, v in ((-3.0, b.cy + 1.2), (W + 2.0, b.cy - 1.2), (b.cx - 2.2, -3.0), (b.cx + 2.2, H + 2.0)):
        b.add("off_image", u, v)
    b.add("cover_all", b.cx + 0.3, b.cy + 0.2, z=4.5, sig=float(max(W, H)), op=0.05)
    # beyond the 1.3 tan(fov) clamp (tx/tz = +-1.5 * 1.3 tan(fov)), large enough to touch the image
    ox, oy = 1.5 * 1.3 * W / 2, 1.5 * 1.3 * H / 2
    b.add("clamped_x", b.cx + ox, b.cy + 1.7, sig=0.45 * W + 6, op=0.6)
    b.add("clamped_y", b.cx - 2.3, b.cy - oy, sig=0.45 * H + 6, op=0.6)
    b.add("clamped_xy", b.cx - ox, b.cy + oy, sig=0.45 * max(W, H) + 8, op=0.7)
    # near plane: one float32 ulp on either side of float32(0.2)
    b.add("near_visible", b.cx - 4.4, b.cy + 2.3, z=np.nextafter(NEAR, np.float32(1)), sig=2.0, op=0.3)
    b.add("near_culled", b.cx + 4.4, b.cy - 2.3, z=np.nextafter(NEAR, np.float32(0)), sig=2.0, op=0.9)
    # tiny: the 0.3 low-pass dominates, radius 2
    b.add("tiny", b.cx - 7.3, b.cy - 3.6, z=3.0, scale=1e-4, op=0.8)
    b.add("tiny", b.cx + 6.7, b.cy + 4.4, z=3.1, scale=(1e-4, 1e-5, 1e-6), op=0.8, q=(0.8, 0.3, -0.4, 0.2))
    b.add("tiny", b.cx + 9.2, b.cy - 5.1, z=3.2, scale=1e-6, op=0.9)
    # needles 1000 : 1 at several in-plane angles
    for i, deg in enumerate((0.0, 30.0, 45.0, 90.0)):
        b.add("needle", b.cx - 9.6 + 6.1 * i, b.cy + 5.3 - 3.4 * i, sig=(6.0, 0.006, 0.006), q=qz(deg), op=0.7)
    # unnormalised quaternions
    for i, n in enumerate((0.5, 0.8, 1.3, 2.0)):
        q = np.array([0.6, -0.3, 0.5, 0.2 + 0.3 * i])
        b.add("unnorm_quat", b.cx + 11.3 - 7.2 * i, b.cy - 6.4 + 3.7 * i, sig=(2.5, 1.2, 0.8), q=tuple(q / np.linalg.norm(q) * n))
    # faint opacities around 1/255 and exactly 0, centred 0.1 px off a pixel centre
    fu, fv = min(W - 1, 3) + 0.1, min(H - 1, 2)
    b.add("faint_above", fu, fv, op=0.004, exact=True)
    b.add("faint_below", fu, fv, op=0.0039, exact=True)
    b.add("opacity_zero", fu, fv, op=0.0, exact=True)
    # equal depths: index order decides
    for i in range(4):
        b.add("equal_depth", 0.3 * W + 1.1 * i, 0.6 * H - 0.7 * i, z=4.2, op=0.5)
    # SH colours pushed below 0 in one, two, three channels (plain Gaussians with precomputed colours)
    for i in range(3):
        b.add("sh_clamped_%d" % (i + 1), 0.7 * W - 2.3 * i, 0.3 * H + 1.9 * i, op=0.6)
    # opaque stack on one pixel near a corner, in front of everything but the near-plane Gaussian: 0.5, then a saturated alpha (T 0.5 -> 0.005), then the entry that ends the pixel
    # (0.005 * (1 - 0.99) < 1e-4); two Gaussians behind it, hidden there and seen next to it
    su, sv = min(W - 1, 33) + 0.05, min(H - 1, 3) + 0.05
    b.add("stack", su, sv, z=1.5, sig=1.5, op=0.5, exact=True)
    b.add("stack", su, sv, z=1.55, sig=8.0, op=1.0, exact=True)
    b.add("stack", su, sv, z=1.6, sig=8.0, op=0.995, exact=True)
    b.add("hidden", su + 0.3, sv - 0.2, z=1.7, op=0.8)
    b.add("hidden", su - 0.4, sv + 0.3, z=1.75, op=0.6)
    return b.rows, (int(su), int(sv))


def _unit(q):
    return q / np.linalg.norm(q)


def _camera(W, H):
    focal = 0.9 * max(W, H)
    return scenes.look_at_camera(W, H, focal), focal


def _finish(W, H, C, seed, v, cam, classes, means, scales, quats, opac):
    P = len(classes)
    rng = np.random.default_rng(seed + 4000)
    feats = shs = None
    if v.colors == "precomp":
        if C == 3:
            feats = rng.uniform(0, 1, (P, 3)).astype(np.float32)
        else:
            f = rng.normal(0, 1, (P, C))
            feats = (f / (np.linalg.norm(f, axis=1, keepdims=True) + 1e-9)).astype(np.float32)
    else:
        assert C == 3
        shs = rng.normal(0, 0.3, (P, 16, 3)).astype(np.float32)
        for i, c in enumerate(classes):
            if c.startswith("sh_clamped_"):
                shs[i, 0, :int(c[-1])] = -8.0     # 0.282 * -8 + 0.5 = -1.76: below 0 whatever the other bands add
    bg = np.zeros(C, np.float32) if v.bg == "zero" else rng.uniform(0, 1, C).astype(np.float32)
    mask = rng.uniform(0, 1, P).astype(np.float32) if (v.mask or v.mask_only) else None
    means, scales, quats = (np.asarray(a, np.float32).reshape(P, -1) for a in (means, scales, quats))
    opac = np.asarray(opac, np.float32).reshape(P, 1)
    cov = None
    if v.cov:   # world covariance in fp64 from scale / rotation, handed over as cov3D_precomp
        L = build_rotation(torch.tensor(quats, dtype=torch.float64)) @ torch.diag_embed(torch.tensor(scales, dtype=torch.float64) * v.modifier)
        S = (L @ L.transpose(1, 2)).numpy()
        cov = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32)
    inp = so.Inputs(means3D=means, opacities=opac, viewmatrix=cam.viewmatrix, projmatrix=cam.projmatrix, campos=cam.campos, bg=bg,
                    image_width=W, image_height=H, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, channels=C, scale_modifier=v.modifier,
                    sh_degree={"precomp": 0, "sh0": 0, "sh3": 3}[v.colors], shs=shs, colors_precomp=feats,
                    scales=None if v.cov else scales, rotations=None if v.cov else quats, cov3D_precomp=cov, mask=mask)
    inp.classes = list(classes)
    return inp


def edge_scene(W, H, C, seed, variant: Variant):
    """The designed classes (every Gaussian of the designed part named in inp.classes) plus a make_scene fill up to variant.P
    Gaussians ("fill").  variant.P == 1: the first designed Gaussian alone; "culled": the fill alone, behind the near plane."""
    cam, focal = _camera(W, H)
    rows, stack_px = _designed(W, H, focal, seed)
    if variant.P == 1:
        rows = rows[:1]
    elif variant.P == "culled":
        rows = []
    n_fill = 40 if variant.P == "culled" else max(0, variant.P - len(rows))
    z_range = (-5.0, 0.15) if variant.P == "culled" else (1.0, 6.0)
    # fill scales for a screen-space sigma of about one pixel at any focal length (0.12 at the 37-pixel image's focal)
    fill = scenes.make_scene(n_fill, W, H, focal, C, math.log(0.12 * 33.3 / focal), 0.5, seed=seed, z_range=z_range)
    classes = [r[0] for r in rows] + ["fill"] * n_fill
    means = np.concatenate([np.array([r[1] for r in rows], np.float64).reshape(-1, 3), fill.means3D.astype(np.float64)])
    scl = np.concatenate([np.array([r[2] for r in rows], np.float64).reshape(-1, 3), fill.scales.astype(np.float64)])
    quats = np.concatenate([np.array([r[3] for r in rows], np.float64).reshape(-1, 4), fill.rotations.astype(np.float64)])
    opac = np.concatenate([np.array([r[4] for r in rows], np.float64).reshape(-1, 1), fill.opacities.astype(np.float64)])
    if variant.modifier != 1.0:
        scl = scl / variant.modifier      # the designed screen-space sizes hold for modifier * scale
    inp = _finish(W, H, C, seed, variant, cam, classes, means, scl, quats, opac)
    inp.stack_pixel = stack_px
    return inp


def list_scene(W, H, C, seed, variant: Variant):
    """One 16 x 16 image = one tile whose list has exactly variant.L entries.  kind "contrib": every entry blends at every pixel
    (wide, faint Gaussians: alpha stays above 1/255 out to 20 px from centres kept 4 px inside the tile, and (1 - 0.05)^129 stays
    far above the stop), so the survivors meet the batch sizes too.  kind "raw": every third entry has opacity 0.003 -- in the raw
    list (its rect covers the tile), never blended -- so that the raw length is L and the contributing length is not."""
    assert (W, H) == (16, 16) and variant.kind in ("contrib", "raw")
    cam, focal = _camera(W, H)
    L = variant.L
    rng = np.random.default_rng(seed + 17 * L)
    b = _Builder(W, H, focal)
    for i in range(L):
        dead = variant.kind == "raw" and i % 3 == 1
        b.add("culled_entry" if dead else "entry", rng.uniform(4, 12), rng.uniform(4, 12), z=2.0 + 0.01 * i,
              sig=rng.uniform(10, 14, 3), q=tuple(_unit(rng.normal(0, 1, 4))), op=0.003 if dead else rng.uniform(0.03, 0.05))
    rows = b.rows
    return _finish(W, H, C, seed, variant, cam, [r[0] for r in rows], [r[1] for r in rows],
                   np.array([r[2] for r in rows]) / variant.modifier, [r[3] for r in rows], [r[4] for r in rows])


# ---- scenes of many tiles and uneven density -------------------------------------------------------------------------------------
# What only exists with many tiles: a gradient row summed by atomics from every tile, the eight XCD runs cut at equal modelled
# work (csrc/tile_ranges.h, xcd_runs.h) with their queued halves, empty ranges between occupied tiles, a last tile column / row
# one pixel wide, a tile whose walk ends long before its list.  Two images whose partial last tiles buy many tiles for few pixels
# (the dense float64 reference is O(P W H)):
#   "t1"  97 x 33: 7 x 3 tiles, last tile column and last tile row 1 px wide;   "t2"  177 x 17: 12 x 2 tiles, last row 1 px tall.
TILE_SIZES = {"t1": (97, 33), "t2": (177, 17)}
DENSE_LIST = max(LIST_LENGTHS) + 1       # raw entries the dense tile's list holds at least
DENSE_TILE = {"t1": (5, 1), "t2": (10, 0)}   # (tile column, tile row)
OPAQUE_TILE = (0, 1)                     # t1
EMPTY_BAND = (4, 5, 6)                   # t2: tile columns of the top tile row
N_DENSE = {"t1": 200, "t2": 240}         # Gaussians inside the dense tile: long enough a list for an XCD run of one tile


def _tiles_designed(which, W, H, focal, seed):
    b = _Builder(W, H, focal, np.random.default_rng(seed + 9000))

    def quat():
        return tuple(_unit(b.rng.normal(0, 1, 4)))

    def inside(cls, tile, n, op):
        # rects that stay inside the one tile: a largest sigma of 1.5 px is radius 6 at most (the low-pass and the perspective
        # factor included), centres 6.2 to 10.6 px into the tile; anisotropic and rotated, so that every gradient class has terms.
        # (Sigmas of 0.5 to 0.8 px were tried first: at x = 90 or 170 the float32 rounding of the centre alone moves such a row
        # of dL_dopacity by 2^-15 of its terms, and the class would have needed FACTOR 512.)
        for _ in range(n):
            b.add(cls, 16 * tile[0] + b.rng.uniform(6.4, 10.4), 16 * tile[1] + b.rng.uniform(6.4, 10.4),
                  sig=(1.5, b.rng.uniform(1.2, 1.5), b.rng.uniform(1.2, 1.5)), q=quat(), op=b.rng.uniform(*op))

    if which == "t1":
        # in front of everything, in every tile, blended at every pixel (0.1 exp(-r^2 / (2 * 26^2)) stays above 1/255 out to 66 px)
        b.add("spanning_front", b.cx + 0.3, b.cy + 0.2, z=0.6, sig=(30.0, 26.0, 28.0), q=quat(), op=0.1)
        # seven near-opaque Gaussians over tile (0, 1) end every pixel's walk there: alpha >= 0.78 on the tile, 0.9 * 0.22^7 < 1e-4;
        # sigma 16 is radius 53: tile columns 0 to 3, short of the dense tile's neighbours.  0.98 stays below the 0.99 clamp, whose
        # contour would cross the tile otherwise
        ou, ov = 16 * OPAQUE_TILE[0] + 8, 16 * OPAQUE_TILE[1] + 8
        for i in range(7):
            b.add("opaque_front", ou, ov, z=0.8 + 0.01 * i, sig=16.0, op=0.98)
        inside("hidden", OPAQUE_TILE, 30, (0.3, 0.8))
        for k in range(1, 7):                 # every interior tile corner of the middle tile row: four tiles each
            for y in (16, 32):                # (the two on the opaque tile's corners in front of it: they blend there as well)
                b.add("corner", 16 * k, y, sig=1.5, z=(0.7 + y / 3200) if k == 1 else None)
        # centres off the image: alpha >= 1/255 on x = 96 (y = 32) alone -- one pixel further in it is at most 0.6 / 255
        for y in (7.3, 22.6, 31.4):
            b.add("last_column", W + 1.3, y, sig=0.8, op=0.15)
        for x in (40.3, 56.4, 88.3):
            b.add("last_row", x, H + 1.3, sig=0.8, op=0.3)
        inside("dense_tile", DENSE_TILE[which], N_DENSE[which], (0.01, 0.08))
        b.add("spanning_back", b.cx - 0.3, b.cy - 0.2, z=b.depth() + 5.0, sig=(26.0, 30.0, 28.0), q=quat(), op=0.1)
    else:
        for x in (32, 48, 128, 144):          # the tile corners on either side of the empty band, one tile away from it
            b.add("corner", x, 16, sig=1.5)
        inside("dense_tile", DENSE_TILE[which], N_DENSE[which], (0.01, 0.08))
    return b.rows


def tiles_scene(W, H, C, seed, variant: Variant):
    """variant.kind "t1" / "t2": the designed classes above, then a make_scene fill of variant.P - (designed) Gaussians -- of which
    t2 drops those that could reach its empty band (the band is a designed property, the fill is not)."""
    which = variant.kind
    assert (W, H) == TILE_SIZES[which]
    cam, focal = _camera(W, H)
    rows = _tiles_designed(which, W, H, focal, seed)
    n_fill = max(0, variant.P - len(rows))
    fill = scenes.make_scene(n_fill, W, H, focal, C, math.log(0.12 * 33.3 / focal), 0.5, seed=seed, z_range=(1.0, 6.0))
    keep = np.ones(n_fill, bool)
    if which == "t2":
        m = fill.means3D.astype(np.float64)
        u = focal * m[:, 0] / m[:, 2] + (W - 1) * 0.5
        # 3 sigma of the largest axis with the perspective factor (at most 1 + tan^2) and the low-pass, and 2 px on top
        r = 3.0 * np.sqrt(1.5 * (fill.scales.astype(np.float64).max(axis=1) * focal / m[:, 2]) ** 2 + 0.3) + 2.0
        keep = (u + r < 16 * EMPTY_BAND[0]) | (u - r >= 16 * (EMPTY_BAND[-1] + 1))
    classes = [r[0] for r in rows] + ["fill"] * int(keep.sum())
    cat = lambda i, a, n: np.concatenate([np.array([r[i] for r in rows], np.float64).reshape(-1, n), a.astype(np.float64)[keep]])
    scl = cat(2, fill.scales, 3)
    if variant.modifier != 1.0:
        scl = scl / variant.modifier
    return _finish(W, H, C, seed, variant, cam, classes, cat(1, fill.means3D, 3), scl, cat(3, fill.rotations, 4),
                   cat(4, fill.opacities, 1))


def tile_lists(ref):
    """(tile rows, tile columns) list lengths of a case from the oracle's full-list ranges."""
    inp = ref.inp
    gx, gy = (inp.image_width + 15) // 16, (inp.image_height + 15) // 16
    r = np.asarray(ref.fwd.state.field(so.F_RANGES), np.int64).reshape(gy * gx, 2)
    return (r[:, 1] - r[:, 0]).reshape(gy, gx)


def model_runs(ref):
    """The nine XCD run boundaries tile_ranges_kernel publishes by default for the case (csrc/tile_ranges.h: equal sums of
    min(list length, RUN_CAP) + RUN_FIX over the row-major tiles, restated by tests/test_xcd_mapping.py) on the oracle's full
    lists, and those of equal tile counts."""
    from tests.test_xcd_mapping import bounds_from_model, run_start
    lists = tile_lists(ref).reshape(-1)
    return bounds_from_model(lists, RUN_CAP, RUN_FIX), [run_start(x, len(lists)) for x in range(9)]


def make_inputs(case):
    """case = (scene function name, W, H, C, seed, Variant)."""
    fn, W, H, C, seed, v = case
    return {"edge": edge_scene, "list": list_scene, "tiles": tiles_scene}[fn](W, H, C, seed, v)


def gradient_images(inp, seed):
    W, H, C = inp.image_width, inp.image_height, inp.channels
    dL = (scenes.make_grad_image(C, H, W, seed=seed + 1) * (W * H)).astype(np.float32)
    dLm = None
    if inp.mask is not None:
        dLm = np.random.default_rng(seed + 2).normal(0, 1, (1, H, W)).astype(np.float32)
    return dL, dLm


# ---- the three CPU evaluations -------------------------------------------------------------------------------------------------

PIXEL_CLASSES = ("image", "final_T", "out_mask", "out_depth")


def classes_of_grads(inp, g):
    """The gradient classes of a run, (P, row) float64 arrays, from a dict / BackwardOut of the oracle's or the product's names.
    dL_dscales is multiplied by the scale modifier (reference quirk, CF backward.cu:295-325: dL/dscale is taken w.r.t.
    modifier * scale and not multiplied by the modifier; tests/test_oracle_dense.py compares it the same way)."""
    get = (lambda k: g.get(k)) if isinstance(g, dict) else (lambda k: getattr(g, k, None))
    P = np.asarray(inp.means3D).reshape(-1, 3).shape[0]
    out = {}
    r = lambda a, n=None: np.asarray(a, np.float64).reshape(P, -1)
    if get("dL_dmeans2D") is not None:
        out["dL_dmeans2D"] = r(get("dL_dmeans2D"))[:, :2]
        out["dL_dopacity"] = r(get("dL_dopacity"))
        out["dL_dmeans3D"] = r(get("dL_dmeans3D"))
        if inp.shs is not None:
            out["dL_dsh"] = r(get("dL_dsh"))
        if inp.cov3D_precomp is not None:
            out["dL_dcov3D"] = r(get("dL_dcov3D"))
        else:
            out["dL_dscales"] = r(get("dL_dscales")) * inp.scale_modifier
            out["dL_drotations"] = r(get("dL_drotations"))
    if inp.shs is None and get("dL_dcolors") is not None:
        out["dL_dcolors"] = r(get("dL_dcolors"))
    if inp.mask is not None and get("dL_dmask") is not None:
        out["dL_dmask"] = r(get("dL_dmask"))
    return out


def _dense(inp, dL, dLm, dt, quirks, magnitudes, block=4):
    W, H, C = inp.image_width, inp.image_height, inp.channels
    P = np.asarray(inp.means3D).reshape(-1, 3).shape[0]
    t = lambda a, g=True: None if a is None else torch.tensor(np.asarray(a, np.float64), dtype=dt, requires_grad=g)
    lv = dict(means3D=t(np.asarray(inp.means3D).reshape(P, 3)), opac=t(np.asarray(inp.opacities).reshape(P, 1)),
              scales=t(inp.scales), rots=t(inp.rotations), cov=t(inp.cov3D_precomp), cols=t(inp.colors_precomp),
              shs=t(None if inp.shs is None else np.asarray(inp.shs).reshape(P, -1, 3)), mask=t(inp.mask),
              m2d=torch.zeros(P, 3, dtype=dt, requires_grad=True))
    ref = render_dense(lv["means3D"], lv["opac"], t(inp.viewmatrix, False), t(inp.projmatrix, False), t(inp.campos, False),
                       t(inp.bg, False), W, H, inp.tanfovx, inp.tanfovy, scales=lv["scales"], rotations=lv["rots"],
                       cov3D_precomp=lv["cov"], colors_precomp=lv["cols"], shs=lv["shs"], sh_degree=inp.sh_degree,
                       scale_modifier=inp.scale_modifier, means2D_offset=lv["m2d"], mask=lv["mask"], dt=dt, reference_quirks=quirks)
    names = dict(m2d="dL_dmeans2D", opac="dL_dopacity", means3D="dL_dmeans3D", shs="dL_dsh", cov="dL_dcov3D", scales="dL_dscales",
                 rots="dL_drotations", cols="dL_dcolors")
    keys = [k for k in names if lv[k] is not None]
    leaves = [lv[k] for k in keys]
    prod = ref["color"] * torch.tensor(dL, dtype=dt)                                   # (C, H, W)
    total = [torch.zeros_like(x) for x in leaves]
    mags = [torch.zeros_like(x) for x in leaves]
    if magnitudes:
        # one batched backward over the block x block pixel blocks (4 x 4; coarser for the many-tile scenes, which only lowers
        # the floor): block b's loss is the sum of `prod` over its pixels
        by, bx = (H + block - 1) // block, (W + block - 1) // block
        ys, xs = torch.meshgrid(torch.arange(H) // block, torch.arange(W) // block, indexing="ij")
        sel = torch.nn.functional.one_hot((ys * bx + xs).reshape(-1), by * bx).T.reshape(by * bx, 1, H, W).to(dt)
        gs = torch.autograd.grad(prod, leaves, grad_outputs=sel.expand(-1, C, -1, -1), retain_graph=True, allow_unused=True,
                                 is_grads_batched=True)
        for i, g in enumerate(gs):
            if g is not None:
                total[i] = g.sum(0)
                mags[i] = g.abs().sum(0)
    else:
        gs = torch.autograd.grad(prod.sum(), leaves, retain_graph=True, allow_unused=True)
        total = [torch.zeros_like(x) if g is None else g for x, g in zip(leaves, gs)]
    raw = {names[k]: g.double().numpy() for k, g in zip(keys, total)}
    rawm = {names[k]: g.double().numpy() for k, g in zip(keys, mags)}
    if inp.mask is not None:
        # reference quirk (DEPTH/cuda_rasterizer/backward.cu:516): dL/dout_mask reaches dL_dmask alone
        raw["dL_dmask"] = torch.autograd.grad((ref["mask"] * torch.tensor(dLm, dtype=dt)).sum(), lv["mask"],
                                              retain_graph=True)[0].double().numpy()
        rawm["dL_dmask"] = (ref["weights"].double() @ torch.tensor(np.abs(dLm), dtype=torch.float64).reshape(-1))[
            torch.argsort(ref["order"])].numpy()
    if inp.scale_modifier != 1.0 and "dL_dscales" in raw:     # classes_of_grads multiplies by the modifier: undo for autograd's
        raw["dL_dscales"] = raw["dL_dscales"] / inp.scale_modifier
        rawm["dL_dscales"] = rawm["dL_dscales"] / inp.scale_modifier
    out = classes_of_grads(inp, raw)
    n = H * W
    out["image"] = ref["color"].detach().double().numpy().reshape(C, n).T.copy()
    out["final_T"] = ref["final_T"].detach().double().numpy().reshape(n, 1)
    if inp.mask is not None:
        out["out_mask"] = ref["mask"].detach().double().numpy().reshape(n, 1)
        out["out_depth"] = ref["depth"].detach().double().numpy().reshape(n, 1)
    mag = None
    if magnitudes:
        mag = {k: v.max(axis=1) for k, v in classes_of_grads(inp, rawm).items()}
        o = ref["order"]
        w = ref["weights"].double()                                                       # (P, N), list order
        a = ref["alpha_eff"].double()
        col = ref["colors"].double()[o].abs()
        bg = torch.tensor(np.asarray(inp.bg, np.float64))
        Tf = ref["final_T"].detach().double().reshape(-1)
        mag["image"] = ((w.T @ col) + Tf[:, None] * bg.abs()[None]).max(dim=1).values.numpy()
        K = (a / (1 - a)).sum(0)
        mag["final_T"] = (Tf * (1 + K)).numpy()
        if inp.mask is not None:
            mag["out_mask"] = (w.T @ lv["mask"].detach().double().abs()[o]).numpy()
            mag["out_depth"] = (w.T @ ref["view_z"].double().abs()[o]).numpy()
        # hybrid-exp allowances (tests/test_raster_edges.py): k_g = 1 + sum_{j<g} alpha_j / (1 - alpha_j)
        kg = 1 + torch.cumsum(a / (1 - a), 0) - a / (1 - a)
        mag["image_hybrid"] = ((kg * w).T @ col).max(dim=1).values.numpy()
        mag["K"] = K.numpy()
    return out, mag, ref


def oracle_classes(inp, dL, dLm):
    """The oracle's forward and backward as classes (+ its ForwardOut)."""
    W, H, C = inp.image_width, inp.image_height, inp.channels
    n = H * W
    if getattr(inp, "mask_only", False):
        fwd = so.mask_forward(inp)
        out = {"out_mask": np.asarray(fwd.mask, np.float64).reshape(n, 1),
               "dL_dmask": np.asarray(so.mask_backward(inp, fwd, dLm[0]), np.float64).reshape(-1, 1)}
        return out, fwd
    fwd = so.forward(inp)
    assert fwd.rc == 0
    bwd = so.backward(inp, fwd, dL, None if dLm is None else dLm[0])
    out = classes_of_grads(inp, bwd)
    out["image"] = np.asarray(fwd.color, np.float64).reshape(C, n).T.copy()
    out["final_T"] = fwd.state.field(so.F_FINAL_T).astype(np.float64).reshape(n, 1)
    if inp.mask is not None:
        out["out_mask"] = np.asarray(fwd.mask, np.float64).reshape(n, 1)
        out["out_depth"] = np.asarray(fwd.depth, np.float64).reshape(n, 1)
    return out, fwd


MASK_ONLY_CLASSES = ("out_mask", "dL_dmask")
MAG_BLOCK = {"tiles": 8}     # pixel-block edge of the term magnitudes per scene kind (4 unless named): a 290-Gaussian case stays affordable


class Reference:
    """The three CPU evaluations of one case and everything derived from them."""

    def __init__(self, case, quirks=True):
        self.case = case
        inp = self.inp = make_inputs(case)
        v = case[5]
        inp.mask_only = bool(v.mask_only)
        self.dL, self.dLm = gradient_images(inp, case[4])
        # a few threads at most: the tensors are small, and more threads cost more than they give when the machine is busy;
        # one for float32, whose sums then have an order that does not depend on how many cores the machine has
        threads = torch.get_num_threads()
        try:
            torch.set_num_threads(min(4, threads))
            self.d64, self.mag, ref = _dense(inp, self.dL, self.dLm, torch.float64, quirks, True, MAG_BLOCK.get(case[0], 4))
            torch.set_num_threads(1)
            self.d32, _, ref32 = _dense(inp, self.dL, self.dLm, torch.float32, quirks, False)
        finally:
            torch.set_num_threads(threads)
        self.oracle, self.fwd = oracle_classes(inp, self.dL, self.dLm)
        if v.mask_only:
            self.d64 = {k: self.d64[k] for k in MASK_ONLY_CLASSES}
            self.d32 = {k: self.d32[k] for k in MASK_ONLY_CLASSES}
        self.classes = [k for k in self.d64]
        self.radii = ref["radii"].numpy()
        self.radii32 = ref32["radii"].numpy()
        self.tiles_touched = ref["tiles_touched"].numpy()
        self.dense = {k: (ref[k].numpy() if ref[k] is not None else None) for k in
                      ("raw_alpha", "power", "power_terms", "member", "stop_value", "alive", "weights", "alpha_eff", "sh_pre_clamp",
                       "txtz", "tytz", "view_z", "order", "contrib")}
        self._margins()

    def _margins(self):
        d, inp = self.dense, self.inp
        P, N = d["member"].shape
        o = d["order"]
        considered = d["member"] & np.concatenate([np.ones((1, N), bool), d["alive"][:-1]], 0)   # pairs the kernels evaluate
        a = np.minimum(d["raw_alpha"], 0.99)
        near = np.abs(255.0 * a - 1.0) <= 1e-4
        near |= np.abs(d["raw_alpha"] / 0.99 - 1.0) <= 1e-4
        # power at 0: within 1e-4 absolute AND within 1e-4 of the magnitude of its own three terms -- a centre on a pixel centre has
        # power ~ -1e-13 with terms of 1e-13, whose sign no float32 rounding turns (the conic is positive definite by a margin)
        near |= (np.abs(d["power"]) <= 1e-4) & (np.abs(d["power"]) < 1e-4 * d["power_terms"])
        ae = d["alpha_eff"]
        K = (ae / (1 - ae)).sum(0)
        blended_or_stop = considered & (d["power"] <= 0) & (a >= 1.0 / 255.0)
        near_stop = blended_or_stop & (np.abs(d["stop_value"] / 1e-4 - 1.0) <= 4e-6 * K[None] + 1e-5)
        self.near_pairs = (near & considered) | near_stop
        # per Gaussian (input order)
        ng = np.zeros(P, bool)
        infront = d["view_z"] > 0.2
        if d["sh_pre_clamp"] is not None:
            ng |= infront & (np.abs(d["sh_pre_clamp"]) <= 1e-5).any(axis=1)
        for q, lim in ((d["txtz"], 1.3 * inp.tanfovx), (d["tytz"], 1.3 * inp.tanfovy)):
            ng |= infront & (np.abs(np.abs(q) / lim - 1.0) <= 1e-4)
        ng |= np.abs(d["view_z"] - np.float64(NEAR)) < np.float64(np.spacing(NEAR))
        self.near_gaussians = ng
        pix = self.near_pairs.any(axis=0) | (considered & ng[o][:, None]).any(axis=0)
        gl = (d["weights"] > 0)[:, pix].any(axis=1)                                              # list order
        g = ng.copy()
        g[o[gl]] = True
        self.excused_pixels, self.excused_gaussians = pix, g
        self.K_max = float(K.max()) if K.size else 0.0

    def excused(self, cls):
        return self.excused_pixels if cls in PIXEL_CLASSES else self.excused_gaussians

    # ---- the rule ----
    def ratios(self, cls, product, factor, floor, e32_from=("oracle", "d32"), extra=None):
        """error / bound per group (excused groups 0), and the groups whose exact-zero state differs."""
        want = self.d64[cls]
        got = np.asarray(product, np.float64).reshape(want.shape)
        e32 = np.zeros(want.shape[0])
        for k in e32_from:
            e32 = np.maximum(e32, np.abs(getattr(self, k)[cls] - want).max(axis=1))
        bound = np.maximum(factor * e32, floor * self.mag[cls])
        if extra is not None:
            bound = bound + extra
        with np.errstate(invalid="ignore"):
            err = np.abs(got - want).max(axis=1)              # NaN / inf in the product stay: never <= 1
        r = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
        zero_differs = (np.abs(want).max(axis=1) == 0) != (np.abs(got).max(axis=1) == 0)
        if cls == "dL_dsh":   # a clamped colour channel cuts that channel's dL_dsh exactly
            zc = (np.abs(want.reshape(len(want), -1, 3)).max(axis=1) == 0) != (np.abs(got.reshape(len(got), -1, 3)).max(axis=1) == 0)
            zero_differs = zero_differs | zc.any(axis=1)
        ex = self.excused(cls)
        return np.where(ex, 0.0, r), zero_differs & ~ex

    def check(self, name, product: dict, extra=None, classes=None):
        """Asserts the rule for every class present in `product`; prints and returns the worst error / bound per class."""
        worst, failed = {}, []
        assert classes is not None or set(self.classes) <= set(product), sorted(set(self.classes) - set(product))
        for cls in (classes or self.classes):
            assert cls in product, (name, cls, "missing from the product's outputs")
            f, fl = rule(cls, self.case[0])
            r, zd = self.ratios(cls, product[cls], f, fl, extra=None if extra is None else extra.get(cls))
            worst[cls] = float("nan") if np.isnan(r).any() else float(r.max()) if r.size else 0.0
            bad = np.flatnonzero(~(r <= 1.0) | zd)
            if bad.size:
                failed.append((cls, [(int(i), self.group_name(cls, i), float(r[i]), bool(zd[i])) for i in bad[:6]], int(bad.size)))
        print(f"{name}: error / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        assert not failed, (name, failed)
        return worst

    def group_name(self, cls, i):
        if cls in PIXEL_CLASSES:
            return "pixel (%d, %d)" % (i % self.inp.image_width, i // self.inp.image_width)
        return self.inp.classes[i]

    def hybrid_extra(self):
        """Allowances of the default (hybrid exp) forward on top of the strict bound: 1e-6 is csrc/common.h's bound on alpha."""
        ex = {"image": 1e-6 * self.mag["image_hybrid"]}
        for cls in self.classes:
            if cls not in PIXEL_CLASSES:
                ex[cls] = 1e-6 * self.K_max * self.mag[cls]
        return ex


_CACHE = {}


def reference(case) -> Reference:
    """The three CPU evaluations per (scene, variant), computed once per process."""
    if case not in _CACHE:
        _CACHE[case] = Reference(case)
    return _CACHE[case]


# ---- the cases -------------------------------------------------------------------------------------------------------------------

SEED = 3
CONFIGS = {
    "rgb": (3, Variant()),
    "sh0": (3, Variant(colors="sh0", bg="random")),
    "sh3": (3, Variant(colors="sh3", bg="random")),
    "mask_depth": (3, Variant(colors="sh3", mask=True, bg="random")),
    "mask_only": (3, Variant(mask_only=True)),
    "cov3d": (3, Variant(cov=True)),
    "modifier": (32, Variant(modifier=1.6)),
    "c16": (16, Variant()),
    "c17": (17, Variant(bg="random")),
    "c32": (32, Variant()),
    "c48": (48, Variant(bg="random")),
    "c64": (64, Variant()),
    "c80": (80, Variant(bg="random")),
    "c128": (128, Variant()),          # the features-only backward alone
}
STRICT_CONFIGS = tuple(k for k in CONFIGS if k != "c128")
FEATURE_CONFIGS = ("c16", "c32", "c48", "c64", "c128")
SMALL_SIZES = ((16, 16), (1, 1), (40, 5), (5, 40))
SMALL_CONFIGS = ("rgb",) + FEATURE_CONFIGS     # the small sizes and P = 1: RGB, C = 32, and every width of the features-only backward


# seeds other than SEED, chosen on the CPU so that the caps on excused groups hold (tests/test_raster_edges_host.py asserts them):
# keyed by (scene, W, H, colours, kind, L)
SEEDS = {
    ("list", 16, 16, "sh3", "raw", 128): 4,      # seed 3: one colour channel within 6e-6 of the clamp at 0
    ("edge", 16, 16, "precomp", None, None): 4,  # seed 3: a fill Gaussian within 1e-5 of alpha = 1/255 on pixel (14, 14)
    # seeds 2, 4 and 5: a pair on a decision in one pixel of the dense tile, which excuses every Gaussian blended there (150 and
    # more); seed 3 is clean and cuts the runs without one of a single tile; seed 6 is clean and leaves the dense tile a run of its own
    ("tiles", 97, 33, "precomp", "t1", None): 6,
    ("tiles", 97, 33, "sh3", "t1", None): 6,
}


def _seed(fn, W, H, v):
    return SEEDS.get((fn, W, H, v.colors, v.kind, v.L), SEED)


def edge_case(cfg, W=37, H=21, P=96):
    C, v = CONFIGS[cfg]
    v = v._replace(P=P)
    return ("edge", W, H, C, _seed("edge", W, H, v), v)


def list_case(cfg, kind, L):
    C, v = CONFIGS[cfg]
    v = v._replace(kind=kind, L=L)
    return ("list", 16, 16, C, _seed("list", 16, 16, v), v)


def small_cases(cfg):
    return [edge_case(cfg, W, H) for W, H in SMALL_SIZES] + [edge_case(cfg, P=1), edge_case(cfg, P="culled")]


def list_cases(cfg):
    """Every length of LIST_LENGTHS, once for the contributing entries and once for the raw list."""
    return [list_case(cfg, kind, L) for kind in ("contrib", "raw") for L in LIST_LENGTHS]


TILE_CONFIGS = {"t1": ("rgb", "mask_depth", "mask_only", "c32", "c64"), "t2": ("c32", "rgb")}
TILE_P = {"t1": 266, "t2": 290}      # designed + fill


def tile_case(which, cfg):
    C, v = CONFIGS[cfg]
    W, H = TILE_SIZES[which]
    v = v._replace(P=TILE_P[which], kind=which)
    return ("tiles", W, H, C, _seed("tiles", W, H, v), v)


def tile_cases():
    """The many-tile scenes in their configurations: a calibration input of their own (MUTUAL_TILES), not part of all_cases()."""
    return [tile_case(which, cfg) for which, cfgs in TILE_CONFIGS.items() for cfg in cfgs]


def all_cases():
    """Every case a GPU test of the edge and list scenes uses (the input of MUTUAL's calibration)."""
    out = []
    for cfg in CONFIGS:
        out.append(edge_case(cfg))
        out += list_cases(cfg)
    for cfg in SMALL_CONFIGS:
        out += small_cases(cfg)
    return out


# ---- calibration ---------------------------------------------------------------------------------------------------------------

def mutual_samples(ref: Reference):
    """Per class the (error, other restatement's error, magnitude) of every non-excused group, for both directions of the mutual
    check: the oracle judged by dense32's error, dense32 judged by the oracle's."""
    out = {}
    for cls in ref.classes:
        want = ref.d64[cls]
        eo = np.abs(ref.oracle[cls] - want).max(axis=1)
        ed = np.abs(ref.d32[cls] - want).max(axis=1)
        keep = ~ref.excused(cls)
        m = ref.mag[cls][keep]
        out[cls] = (np.concatenate([eo[keep], ed[keep]]), np.concatenate([ed[keep], eo[keep]]), np.concatenate([m, m]))
    return out


def calibrate(cases, floor_first=True):
    acc = {}
    for case in cases:
        for cls, s in mutual_samples(Reference(case)).items():
            acc.setdefault(cls, []).append(s)
    table = {}
    for cls, parts in acc.items():
        e, E, m = (np.concatenate([p[i] for p in parts]) for i in range(3))
        def passes(F, lf):
            return bool((e <= np.maximum(F * E, (2.0 ** lf) * m)).all())

        k = 0                                       # raise both together until the mutual check passes ...
        while not passes(4.0 * 2 ** k, -22 + k):
            k += 1
        F, lf = 4.0 * 2 ** k, -22 + k
        for what in (("floor", "factor") if floor_first else ("factor", "floor")):   # ... then take back what is not needed
            while what == "floor" and lf > -22 and passes(F, lf - 1):
                lf -= 1
            while what == "factor" and F > 4 and passes(F / 2, lf):
                F /= 2
        worst = float((e / np.maximum(np.maximum(F * E, (2.0 ** lf) * m), 1e-300)).max()) if e.size else 0.0
        table[cls] = (F, lf, round(worst, 3))
    return table


if __name__ == "__main__":
    import sys
    which = sys.argv[1:] or ["edge", "tiles"]      # `python -m tests.raster_edge_ref tiles`: the second table alone
    if "edge" in which:
        for first in (True, False):
            print("MUTUAL, FLOOR lowered first (the committed table):" if first else
                  "MUTUAL, FACTOR lowered first (for comparison, DESIGN.md 2a):")
            for k, v in sorted(calibrate(all_cases(), floor_first=first).items()):
                print(f'    "{k}": {v},')
    if "tiles" in which:
        print("MUTUAL_TILES, FLOOR lowered first (the committed table):")
        for k, v in sorted(calibrate(tile_cases()).items()):
            print(f'    "{k}": {v},')
