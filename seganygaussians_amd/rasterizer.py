"""Host-side mirror of the reference's Python extension API, on top of the C-ABI (include/mi_rast.h).

This file plays the role of BOTH the reference's torch glue (CF/rasterize_points.cu:35-216: tensor
allocation, shape check, P==0 short circuit, M = sh.size(1)) and its Python package
(CF/diff_gaussian_rasterization_contrastive_f/__init__.py: GaussianRasterizationSettings,
GaussianRasterizer, _RasterizeGaussians), parameterised by channel count and variant so that ONE
implementation serves the three reference packages:

    diff_gaussian_rasterization               C = 3                  (BASE/)
    diff_gaussian_rasterization_contrastive_f C = 32 (or 64)         (CF/)
    diff_gaussian_rasterization_depth         C = 3 + mask + depth   (DEPTH/)

Same names, argument order, return order and error messages as the reference.  PyTorch is used for
device memory, streams and autograd plumbing only; all compute is in libmi_rast.so.  There is no
CPU fallback: missing library or non-GPU tensors raise.
"""
from __future__ import annotations

import contextlib
import math
import os
import ctypes as C
import threading
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _lib
from ._ffi import check, contig, dev_ptr, stream_ptr
from .geometry_cache import GeometryCache, disable_geometry_cache, enable_geometry_cache, geometry_cache  # noqa: F401  (re-exported)


def cpu_deep_copy_tuple(input_tuple):
    copied_tensors = [item.cpu().clone() if isinstance(item, torch.Tensor) else item for item in input_tuple]
    return tuple(copied_tensors)


class GaussianRasterizationSettings(NamedTuple):
    # field order == CF/diff_gaussian_rasterization_contrastive_f/__init__.py:156-168
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


class _Resizer:
    """Replacement for resizeFunctional (CF/rasterize_points.cu:27-33): a growable torch uint8 buffer
    handed to the library as a C callback."""

    def __init__(self, device):
        self.device = device
        self.tensor = torch.empty(0, dtype=torch.uint8, device=device)
        self.cb = _lib.RESIZE_FN(self._resize)

    def _resize(self, nbytes, _user):
        try:
            self.tensor = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
            return self.tensor.data_ptr()
        except Exception:  # allocation failure -> NULL -> MI_RAST_ERR_ALLOC
            return None


# Per-call options of the native forward (include/mi_rast.h: `flags`, `features_ready_event`).  The C library keeps no
# state between calls; what the reference API has no argument for is held HERE, per host thread, and handed over with
# each call.
class _CallOptions(threading.local):
    def __init__(self):
        self.flags = 0
        self.features_ready = None   # torch.cuda.Event, kept alive until the forward that consumes it has returned
        self.grad_mode = True        # torch.is_grad_enabled() of the CALLER (autograd switches it off inside Function.forward)

    def call_flags(self):
        """The flags of the next forward: this thread's forward_flags() plus the process-wide switches (enable_antialiasing)."""
        return int(self.flags) | (_lib.MI_RAST_ANTIALIAS if _antialiasing else 0)


_opts = _CallOptions()

# ---- antialiased render mode (EXTENSION, include/mi_rast.h: MI_RAST_ANTIALIAS) ---------------------------------------------------
# The opacity of every Gaussian is scaled by sqrt(det(cov2D) / det(cov2D + 0.3 I)): the Mip-Splatting compensation of the 0.3 px
# screen filter, upstream 3DGS's `antialiasing` switch.  GaussianRasterizationSettings keeps the reference's fields, so the mode is
# a flag: forward_flags(antialiasing=True) per block and thread, or process-wide -- enable_antialiasing() / MI_RAST_ANTIALIASING=1
# in the environment, for unchanged reference scripts -- which ORs the bit into every forward of the three drop-in packages (and
# of lifting.lift_scores).  The backward gets the bit through ForwardNotes like every flag.
_antialiasing = os.environ.get("MI_RAST_ANTIALIASING", "") not in ("", "0")


def enable_antialiasing(on=True):
    """Process-wide opt-in to the antialiased render mode (see above); returns the previous setting."""
    global _antialiasing
    prev, _antialiasing = _antialiasing, bool(on)
    return prev


def antialiasing_enabled():
    return _antialiasing


@contextlib.contextmanager
def forward_flags(full_lists=None, f32_blend=None, no_cull=None, fast_exp=None, verify_lists=None, tile_fwd=None, exact_exp=None,
                  equal_runs=None, antialiasing=None):
    """Within the block, forwards of this thread run with the given modes: `full_lists` materialises the reference's
    point_list / full-list positions (parity tests), `f32_blend` / `tile_fwd` select the f32 FMA-chain / tile-batched forwards for 32/64
    channels (comparison kernels of the PROFILING build only -- MI_RAST_LIB=libmi_rast_prof.so; the product library refuses them with
    MI_RAST_ERR_INVALID), `no_cull` switches the exact-conservative cull off (testing aid), `fast_exp` evaluates exp() as
    v_exp_f32(x * log2e) instead of the device library's expf the reference's kernels call (+2 % views/s, ~5 ulp: a few
    alpha >= 1/255 decisions differ from the reference's); `verify_lists` (debugging aid) checks that the count and emit passes of the
    lean lists agree slot by slot; `exact_exp` makes the forward blend call expf for every pair (product default: the hybrid form of
    csrc/common.h -- same decisions, alpha to 1e-6): alpha / T / n_contrib / final_T are then bit-identical to a build of the
    reference's kernels; `equal_runs` (A/B aid) keeps the blend kernels' XCD runs at equal tile counts instead of equal modelled work;
    `antialiasing` scales every opacity by sqrt(det(cov2D) / det(cov2D + 0.3 I)) (include/mi_rast.h: MI_RAST_ANTIALIAS; the process-wide
    switch enable_antialiasing() / MI_RAST_ANTIALIASING=1 is ORed in after these flags, so antialiasing=False cannot switch the mode
    off for a block while that switch is on: call enable_antialiasing(False)).  The flags of a
    forward are remembered with its buffers and handed to its backward."""
    prev = _opts.flags
    for bit, v in ((_lib.MI_RAST_FULL_LISTS, full_lists), (_lib.MI_RAST_F32_BLEND, f32_blend), (_lib.MI_RAST_NO_CULL, no_cull),
                   (_lib.MI_RAST_FAST_EXP, fast_exp), (_lib.MI_RAST_VERIFY_LISTS, verify_lists),
                   (_lib.MI_RAST_TILE_FWD, tile_fwd), (_lib.MI_RAST_EXACT_EXP, exact_exp), (_lib.MI_RAST_EQUAL_RUNS, equal_runs),
                   (_lib.MI_RAST_ANTIALIAS, antialiasing)):
        if v is not None:
            _opts.flags = (_opts.flags | bit) if v else (_opts.flags & ~bit)
    try:
        yield
    finally:
        _opts.flags = prev


class ForwardNotes:
    """What a native forward tells the backward of ITS buffers, left on the geometry buffer as `.mi_notes`: the MI_RAST_* flags it
    ran with (the backward re-takes the forward's decisions: it needs the same ones) and, after a forward with prezero, who may
    skip the backward's fills.  `prezero` is the zero-filled (P, channels) tensor that becomes dL_dcolors, `pack_zeroed` says that
    the packed field gradients inside the geometry buffer are zero as well.  `epoch` is the epoch cell of the GeometryCache entry
    this forward filled: a hit of that view shares the geometry buffer's scratch and bumps the cell."""
    __slots__ = ("flags", "prezero", "pack_zeroed", "epoch", "epoch_seen")

    def __init__(self, flags, prezero=None, pack_zeroed=False, epoch=None):
        self.flags, self.prezero, self.pack_zeroed = int(flags), prezero, bool(pack_zeroed)
        self.epoch, self.epoch_seen = epoch, (None if epoch is None else epoch[0])

    @classmethod
    def for_hit(cls, flags, prezero=None):
        """A forward that reused a cached view: the scratch is shared between the forwards of the view, so its backward fills it."""
        return cls(flags, prezero, pack_zeroed=False)

    def claim(self):
        """(prezeroed, pack_zeroed) for ONE backward: a second one through a retained graph gets (None, False) and fills for
        itself.  pack_zeroed is also False once a hit of this cached view came in after the forward: it may have used the scratch."""
        prezeroed, self.prezero = self.prezero, None
        pack_zeroed, self.pack_zeroed = self.pack_zeroed, False
        if pack_zeroed and self.epoch is not None and self.epoch[0] != self.epoch_seen:
            pack_zeroed = False
        return prezeroed, pack_zeroed


def _take_notes(geomBuffer):
    """The autograd Functions keep a forward's notes in ctx and take them off the buffer (a cached view's buffer outlives the graph)."""
    return geomBuffer.__dict__.pop("mi_notes", None) or ForwardNotes(0)


# ---- features-only backward (EXTENSION, include/mi_rast.h: MI_RAST_BWD_FEATURES_ONLY) ------------------------------------------
# SAGA's contrastive feature training optimises `_point_features` alone (scene/gaussian_model_ff.py:154-162), but every parameter of
# its model requires grad and the renderer creates `screenspace_points` with requires_grad=True (gaussian_renderer/__init__.py:308):
# autograd asks the rasterizer for all eight gradients, the reference computes them, and nobody reads seven of them.
#   * AUTOMATIC, always on: when autograd itself says that only colors_precomp needs a gradient (ctx.needs_input_grad), the backward
#     computes that one alone -- plain autograd semantics, nothing to opt into.
#   * OPT-IN, for unchanged reference scripts: enable_features_only_backward() / MI_RAST_FEATURES_ONLY_BACKWARD=1 makes every backward
#     of the feature rasterizer return dL_dcolors_precomp and None for the rest (means2D.grad, xyz.grad, ... stay unset).
# Either way the result equals the default backward's dL_dcolors up to the order of the atomic sums.  Never used by the headline
# benchmark: the reference's step computes all eight gradients, and so does bench.py's.
_features_only_backward = os.environ.get("MI_RAST_FEATURES_ONLY_BACKWARD", "") not in ("", "0")


def enable_features_only_backward(on=True):
    """Opt-in: backward passes through the rasterizer produce the gradient of colors_precomp only (see above); returns the previous
    setting.  Applies to calls with precomputed colours / features of a width that is a multiple of 16; others run the full backward."""
    global _features_only_backward
    prev, _features_only_backward = _features_only_backward, bool(on)
    return prev


def features_only_backward_enabled():
    return _features_only_backward


def _features_only_applies(channels, colors_precomp, needs_input_grad, debug):
    """needs_input_grad: (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, ...) of the Function."""
    if debug or colors_precomp is None or colors_precomp.numel() == 0 or not needs_input_grad[3]:
        return False
    if not _lib.load().mi_rast_features_only_supported(int(channels)):
        return False
    others = [needs_input_grad[k] for k in (0, 1, 2, 4, 5, 6, 7)]
    return _features_only_backward or not any(others)


def rasterize_gaussians_native(channels, with_mask_depth, background, means3D, colors, opacity, mask, scales,
                               rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy,
                               image_height, image_width, sh, degree, campos, prefiltered, debug, prezero=False):
    """RasterizeGaussiansCUDA (CF/rasterize_points.cu:35-115; DEPTH/rasterize_points.cu:35-130).

    prezero (a backward will follow: the autograd Functions set it when an input requires grad): the forward also leaves the
    backward's accumulators zero-filled -- a (P, channels) dL_dcolors tensor allocated here and the packed field gradients
    inside the geometry buffer -- stored by the blend kernel beside its own work (include/mi_rast.h: dL_dcolor_next,
    MI_RAST_PREZERO_BWD) instead of by two fill passes in front of the backward.  Both facts are left on the returned geometry
    buffer as `.mi_notes` (ForwardNotes: `.prezero`, `.pack_zeroed`); hand what its `claim()` returns to ONE
    rasterize_gaussians_backward_native call (`prezeroed=`, `pack_zeroed=`).  The dL_dcolors tensor is only made here while it is
    no larger than the image (P <= H W: the kernel takes the fill while it at most doubles its own stores; a larger one is
    cheapest as the backward's own torch.zeros, as before); prezero="always" makes it regardless (tests: the library then uses a
    fill command)."""
    ready = _opts.features_ready          # one-shot: consumed by THIS forward whatever happens below (P == 0, an exception)
    _opts.features_ready = None
    if means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    _check_widths(channels, background, colors, means3D.size(0))
    L = _lib.load()
    P, H, W = means3D.size(0), int(image_height), int(image_width)
    dev = means3D.device
    if not means3D.is_cuda:
        raise RuntimeError("means3D must be a GPU tensor; the MI355X rasterizer has no CPU path")
    radii = torch.zeros(P, dtype=torch.int32, device=dev) if P == 0 else torch.empty(P, dtype=torch.int32, device=dev)
    geom, binning, img = _Resizer(dev), _Resizer(dev), _Resizer(dev)
    rendered = 0
    if P != 0:
        # the kernels write every element, so no zero-fill pass (reference: torch::full(0.0), :68)
        out_color = torch.empty((channels, H, W), dtype=torch.float32, device=dev)
        out_mask = torch.empty((1, H, W), dtype=torch.float32, device=dev) if with_mask_depth else None
        out_depth = torch.empty((1, H, W), dtype=torch.float32, device=dev) if with_mask_depth else None
        M = sh.size(1) if sh.numel() != 0 else 0
        t = [contig(x) for x in (background, means3D, sh, colors, opacity, scales, rotations, cov3D_precomp,
                                  viewmatrix, projmatrix, campos, mask)]
        bg_c, m3_c, sh_c, col_c, op_c, sc_c, rot_c, cov_c, vm_c, pm_c, cp_c, mk_c = t
        n = C.c_int(0)
        flags = _opts.call_flags()
        grad_colors = None
        if prezero and (P <= H * W or prezero == "always"):
            grad_colors = torch.empty((P, channels), dtype=torch.float32, device=dev)
        if with_mask_depth and (mk_c is None or mk_c.numel() != P or not mk_c.is_cuda or mk_c.dtype != torch.float32):
            # the DEPTH package always passes a mask (DEPTH/.../__init__.py:323); without one out_mask / out_depth
            # would be left unwritten
            raise RuntimeError("mask must hold one float32 per Gaussian on the GPU (diff_gaussian_rasterization_depth)")
        # frozen-geometry reuse (opt-in, GeometryCache): same geometry + camera as an earlier forward -> the blend stage alone
        cache, ckey = geometry_cache(), None
        if cache is not None and cache.eligible(debug, prefiltered, flags):
            ckey = cache.key(dev, P, H, W, tan_fovx, tan_fovy, scale_modifier, degree, M, flags, bg_c, m3_c, sh_c, col_c, op_c,
                             sc_c, rot_c, cov_c, vm_c, pm_c, cp_c)
            hit = cache.lookup(ckey)
            if hit is not None:
                hit["epoch"][0] += 1                 # the miss forward's pre-zeroed scratch is no longer its backward's alone
                img_t = torch.empty(hit["img_bytes"], dtype=torch.uint8, device=dev)
                with torch.cuda.device(dev):
                    rc = L.mi_rast_forward_reuse(
                        P, int(channels), int(hit["num_rendered"]), dev_ptr(bg_c, "bg", dev), W, H, dev_ptr(col_c, "colors_precomp", dev),
                        hit["geom"].data_ptr(), hit["blend_list"].data_ptr(), hit["ranges"].data_ptr(), hit["words"].data_ptr(),
                        img_t.data_ptr(), int(hit["longest_run"]), dev_ptr(mk_c, "mask", dev) if with_mask_depth else None,
                        out_color.data_ptr(), out_mask.data_ptr() if with_mask_depth else None,
                        out_depth.data_ptr() if with_mask_depth else None, flags,
                        None if ready is None else C.c_void_p(ready.cuda_event),
                        None if grad_colors is None else grad_colors.data_ptr(), stream_ptr(dev))
                del ready
                check(rc)
                geom_t = hit["geom"].view(-1)        # a new tensor object over the shared storage: the notes are per forward
                geom_t.mi_notes = ForwardNotes.for_hit(flags, grad_colors)
                res = (hit["num_rendered"], out_color) + ((out_mask, out_depth) if with_mask_depth else ()) + \
                      (hit["radii"].clone(), geom_t, hit["blend_list"], img_t)   # (a caller may change its radii in place)
                return res
        with torch.cuda.device(dev):
            rc = L.mi_rast_forward(
                geom.cb, None, binning.cb, None, img.cb, None, P, int(degree), int(M), int(channels),
                dev_ptr(bg_c, "bg", dev), W, H, dev_ptr(m3_c, "means3D", dev), dev_ptr(sh_c, "sh", dev),
                dev_ptr(col_c, "colors_precomp", dev), dev_ptr(op_c, "opacities", dev),
                dev_ptr(sc_c, "scales", dev), float(scale_modifier), dev_ptr(rot_c, "rotations", dev),
                dev_ptr(cov_c, "cov3D_precomp", dev), dev_ptr(vm_c, "viewmatrix", dev),
                dev_ptr(pm_c, "projmatrix", dev), dev_ptr(cp_c, "campos", dev), float(tan_fovx), float(tan_fovy),
                int(bool(prefiltered)), dev_ptr(mk_c, "mask", dev) if with_mask_depth else None,
                out_color.data_ptr(), out_mask.data_ptr() if with_mask_depth else None,
                out_depth.data_ptr() if with_mask_depth else None, radii.data_ptr(), int(bool(debug)),
                flags | (_lib.MI_RAST_PREZERO_BWD if prezero else 0),
                None if ready is None else C.c_void_p(ready.cuda_event),
                None if grad_colors is None else grad_colors.data_ptr(), stream_ptr(dev), C.byref(n))
        del ready
        check(rc)
        rendered = n.value
        entry = None if ckey is None else cache.capture(ckey, W, H, rendered, radii, geom.tensor, binning.tensor, img.tensor)
        # (the backward takes the zeroed scratch of a cached view only while no hit came in between: the entry's epoch)
        geom.tensor.mi_notes = ForwardNotes(flags, grad_colors, bool(prezero), entry["epoch"] if (entry and prezero) else None)
    else:
        out_color = torch.zeros((channels, H, W), dtype=torch.float32, device=dev)
        out_mask = torch.zeros((1, H, W), dtype=torch.float32, device=dev) if with_mask_depth else None
        out_depth = torch.zeros((1, H, W), dtype=torch.float32, device=dev) if with_mask_depth else None
    if with_mask_depth:
        return rendered, out_color, out_mask, out_depth, radii, geom.tensor, binning.tensor, img.tensor
    return rendered, out_color, radii, geom.tensor, binning.tensor, img.tensor


def _check_widths(channels, background, colors, P):
    """The reference compiles NUM_CHANNELS into its kernels, which then index `bg_color[ch]` and `colors[id * C + ch]` for every
    ch < C without a check (forward.cu:343-374, backward.cu:446-535).  Here the width is a run-time argument (the contrastive_f
    drop-in reads it off `colors_precomp`), so a background left over from another width, or a colour tensor of another width
    than the call says, is caught instead of read out of bounds."""
    if background is None or background.numel() < channels:   # (a longer one is harmless: the kernels read bg[0 .. channels))
        raise RuntimeError(f"bg must hold one value per channel: {0 if background is None else background.numel()} given, "
                           f"{channels} channels rendered")
    if colors is not None and colors.numel() != 0 and P != 0 and (colors.ndimension() != 2 or colors.size(0) != P
                                                                  or colors.size(1) != channels):
        raise RuntimeError(f"colors_precomp must have dimensions (num_points, {channels}); got {tuple(colors.shape)}")


def set_features_ready_event(event) -> None:
    """The next forward of this host thread makes its stream wait for `event` (a recorded torch.cuda.Event, or None to
    cancel) right before its blend stage; everything before it -- preprocess, binning, per-tile sort -- only
    reads the geometry and runs ahead.  For training loops that optimise colors_precomp alone.  The event is passed to that
    one mi_rast_forward call as an argument (include/mi_rast.h: features_ready_event) and a reference is held until it
    returns; an error in that forward drops it as well."""
    _opts.features_ready = event


def _flags_of(geomBuffer, flags):
    """The MI_RAST_* flags a backward must run with are those of the forward that filled `geomBuffer`: given explicitly
    (the autograd Functions keep the forward's notes in ctx), else the notes the native forward left on its tensor, else none."""
    if flags is not None:
        return flags
    notes = getattr(geomBuffer, "mi_notes", None)
    return 0 if notes is None else notes.flags


def rasterize_gaussians_backward_native(channels, with_mask_depth, background, means3D, radii, colors, scales,
                                        rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx,
                                        tan_fovy, dL_dout_color, dL_dout_mask, sh, degree, campos, geomBuffer, R,
                                        binningBuffer, imageBuffer, debug, flags=None, prezeroed=None, pack_zeroed=None,
                                        features_only=False):
    """RasterizeGaussiansBackwardCUDA (CF/rasterize_points.cu:117-196; DEPTH/rasterize_points.cu).

    prezeroed: the zero-filled (P, channels) tensor the forward of THESE buffers produced with prezero=True, not used by any
    backward before: it becomes dL_dcolors.  pack_zeroed: that forward also left the packed field gradients in its geometry
    buffer zeroed (None: as `prezeroed`): their fill is skipped.
    features_only (extension, include/mi_rast.h: MI_RAST_BWD_FEATURES_ONLY): dL_dcolors alone is computed and returned in its place
    of the tuple, None everywhere else."""
    L = _lib.load()
    P = means3D.size(0)
    H, W = dL_dout_color.size(1), dL_dout_color.size(2)
    M = sh.size(1) if sh.numel() != 0 else 0
    dev = means3D.device
    _check_widths(channels, background, colors, P)
    if dL_dout_color.ndimension() != 3 or dL_dout_color.size(0) != channels:
        raise RuntimeError(f"dL_dout_color must have dimensions ({channels}, H, W); got {tuple(dL_dout_color.shape)}")
    if features_only and (with_mask_depth or colors.numel() == 0):
        raise RuntimeError("features_only backward needs precomputed colours and the plain (not DEPTH) rasterizer")
    full = not features_only
    o = dict(device=dev, dtype=torch.float32)
    # The reference allocates ten zero tensors (rasterize_points.cu:151-159).  Same tensors here: dL_dcolors and dL_dsh,
    # which the kernels accumulate into, zero-filled; the others carved from ONE uninitialised block that
    # mi_rast_backward writes in full (zeros for Gaussians that were not rendered, include/mi_rast.h) -- 96 B per Gaussian
    # of fill traffic and nine fill launches less.  dL_dcolors -- the one gradient SAGA's feature training keeps
    # (`_point_features.grad`) -- has its own storage, so holding it does not pin the geometry gradients.
    # `debug` poisons the block with NaN first: a row the library failed to write would surface in the gradients.
    # The features-only backward has dL_dcolors alone: no block, no dL_dsh, and the library is told M = 0 and debug = 0.
    g = {}
    if full:
        shapes = [("dL_dmeans3D", (P, 3)), ("dL_dmeans2D", (P, 3)), ("dL_dconic", (P, 2, 2)), ("dL_dopacity", (P, 1)),
                  ("dL_dcov3D", (P, 6)), ("dL_dscales", (P, 3)), ("dL_drotations", (P, 4))]
        if with_mask_depth:
            shapes.append(("dL_dmask", (P, 1)))   # DEPTH/rasterize_points.cu:167: torch::zeros({P, 1})
        counts = [math.prod(shp) for _, shp in shapes]
        starts = [0]
        for n in counts:
            starts.append(starts[-1] + (n + 3) // 4 * 4)   # keep every tensor 16-byte aligned
        flat = torch.empty(starts[-1], **o)
        if debug:
            flat.fill_(float("nan"))
        for (name, shp), n, off in zip(shapes, counts, starts):
            g[name] = flat[off:off + n].view(shp)
    if pack_zeroed is None:
        pack_zeroed = prezeroed is not None
    if prezeroed is not None and (tuple(prezeroed.shape) != (P, channels) or prezeroed.device != dev or (debug and full)):
        prezeroed = None
    g["dL_dcolors"] = prezeroed if prezeroed is not None else torch.zeros((P, channels), **o)
    if full:
        g["dL_dsh"] = torch.zeros((P, M, 3), **o)
    if P != 0:
        def only_full(x):
            return x if full else None

        def grad(name, present=True):
            return g[name].data_ptr() if (present and name in g) else None

        t = [contig(x) for x in (background, means3D, only_full(sh), colors, only_full(scales), only_full(rotations),
                                  only_full(cov3D_precomp), viewmatrix, projmatrix, campos, dL_dout_color,
                                  dL_dout_mask if with_mask_depth else None, radii)]
        bg_c, m3_c, sh_c, col_c, sc_c, rot_c, cov_c, vm_c, pm_c, cp_c, dpix_c, dmask_c, radii_c = t
        with torch.cuda.device(dev):
            rc = L.mi_rast_backward(
                P, int(degree), int(M) if full else 0, int(channels), int(R), dev_ptr(bg_c, "bg", dev), W, H,
                dev_ptr(m3_c, "means3D", dev), dev_ptr(sh_c, "sh", dev), dev_ptr(col_c, "colors_precomp", dev),
                dev_ptr(sc_c, "scales", dev), float(scale_modifier), dev_ptr(rot_c, "rotations", dev),
                dev_ptr(cov_c, "cov3D_precomp", dev), dev_ptr(vm_c, "viewmatrix", dev),
                dev_ptr(pm_c, "projmatrix", dev), dev_ptr(cp_c, "campos", dev), float(tan_fovx), float(tan_fovy),
                dev_ptr(radii_c, "radii", dev, torch.int32), geomBuffer.data_ptr(), binningBuffer.data_ptr(),
                imageBuffer.data_ptr(), dev_ptr(dpix_c, "dL_dout_color", dev), dev_ptr(dmask_c, "dL_dout_mask", dev),
                grad("dL_dmeans2D"), grad("dL_dconic"), grad("dL_dopacity"), grad("dL_dcolors"), grad("dL_dmask"),
                grad("dL_dmeans3D"), grad("dL_dcov3D"), grad("dL_dsh", M > 0), grad("dL_dscales"), grad("dL_drotations"),
                int(bool(debug)) if full else 0,
                int(_flags_of(geomBuffer, flags)) | (0 if full else _lib.MI_RAST_BWD_FEATURES_ONLY)
                | (_lib.MI_RAST_PREZERO_BWD if pack_zeroed else 0), stream_ptr(dev))
        check(rc)
    if features_only:
        return None, g["dL_dcolors"], None, None, None, None, None, None
    if with_mask_depth:
        return (g["dL_dmeans2D"], g["dL_dcolors"], g["dL_dopacity"], g["dL_dmask"], g["dL_dmeans3D"], g["dL_dcov3D"], g["dL_dsh"],
                g["dL_dscales"], g["dL_drotations"])
    return (g["dL_dmeans2D"], g["dL_dcolors"], g["dL_dopacity"], g["dL_dmeans3D"], g["dL_dcov3D"], g["dL_dsh"], g["dL_dscales"],
            g["dL_drotations"])


def mark_visible_native(means3D, viewmatrix, projmatrix):
    """markVisible (CF/rasterize_points.cu:198-216)."""
    L = _lib.load()
    P = means3D.size(0)
    dev = means3D.device
    present = torch.zeros(P, dtype=torch.bool, device=dev)
    if P != 0:
        m3_c, vm_c, pm_c = contig(means3D), contig(viewmatrix), contig(projmatrix)
        with torch.cuda.device(dev):
            rc = L.mi_rast_mark_visible(P, dev_ptr(m3_c, "means3D", dev), dev_ptr(vm_c, "viewmatrix", dev),
                                        dev_ptr(pm_c, "projmatrix", dev), present.data_ptr(), stream_ptr(dev))
        check(rc)
    return present


def rasterize_mask_gaussians_native(means3D, opacity, mask, scales, rotations, scale_modifier, cov3D_precomp,
                                    viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width,
                                    prefiltered, debug):
    """RasterizeMaskGaussiansCUDA (DEPTH/rasterize_points.cu, mask-only forward)."""
    _opts.features_ready = None           # a features-ready event is for the next FEATURE forward of this thread: never left armed
    if means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    L = _lib.load()
    P, H, W = means3D.size(0), int(image_height), int(image_width)
    dev = means3D.device
    radii = torch.zeros(P, dtype=torch.int32, device=dev)
    geom, binning, img = _Resizer(dev), _Resizer(dev), _Resizer(dev)
    rendered = 0
    if P != 0:
        out_mask = torch.empty((1, H, W), dtype=torch.float32, device=dev)
        t = [contig(x) for x in (means3D, opacity, mask, scales, rotations, cov3D_precomp, viewmatrix, projmatrix)]
        m3_c, op_c, mk_c, sc_c, rot_c, cov_c, vm_c, pm_c = t
        n = C.c_int(0)
        mask_flags = _opts.call_flags()
        with torch.cuda.device(dev):
            rc = L.mi_rast_mask_forward(
                geom.cb, None, binning.cb, None, img.cb, None, P, W, H, dev_ptr(m3_c, "means3D", dev),
                dev_ptr(op_c, "opacities", dev), dev_ptr(mk_c, "mask", dev), dev_ptr(sc_c, "scales", dev),
                float(scale_modifier), dev_ptr(rot_c, "rotations", dev), dev_ptr(cov_c, "cov3D_precomp", dev),
                dev_ptr(vm_c, "viewmatrix", dev), dev_ptr(pm_c, "projmatrix", dev), float(tan_fovx),
                float(tan_fovy), int(bool(prefiltered)), out_mask.data_ptr(), radii.data_ptr(), int(bool(debug)),
                mask_flags, stream_ptr(dev), C.byref(n))
        check(rc)
        rendered = n.value
        geom.tensor.mi_notes = ForwardNotes(mask_flags)
    else:
        out_mask = torch.zeros((1, H, W), dtype=torch.float32, device=dev)
    return rendered, out_mask, radii, geom.tensor, binning.tensor, img.tensor


def rasterize_mask_gaussians_backward_native(means3D, dL_dout_mask, geomBuffer, R, binningBuffer, imageBuffer, debug, flags=None):
    L = _lib.load()
    P = means3D.size(0)
    H, W = dL_dout_mask.size(-2), dL_dout_mask.size(-1)
    dev = means3D.device
    dL_dmask = torch.zeros((P, 1), dtype=torch.float32, device=dev)   # DEPTH/rasterize_points.cu:349
    if P != 0:
        d_c = contig(dL_dout_mask)
        with torch.cuda.device(dev):
            rc = L.mi_rast_mask_backward(P, int(R), W, H, geomBuffer.data_ptr(), binningBuffer.data_ptr(),
                                         imageBuffer.data_ptr(), dev_ptr(d_c, "dL_dout_mask", dev),
                                         dL_dmask.data_ptr(), int(bool(debug)), int(_flags_of(geomBuffer, flags)),
                                         stream_ptr(dev))
        check(rc)
    return dL_dmask


# --------------------------------------------------------------------------------------------------
# autograd + nn.Module layer, generated per (channels, variant)
# --------------------------------------------------------------------------------------------------

_MSG_COLORS = 'Please provide excatly one of either SHs or precomputed colors!'
_MSG_COV = 'Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!'
_SNAPSHOT_FW = ("snapshot_fw.dump", "\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
_SNAPSHOT_BW = ("snapshot_bw.dump", "\nAn error occured in backward. Writing snapshot_bw.dump for debugging.\n")


def _snapshot_call(debug, args, fn, path, message):
    """fn(*args); under `debug` the reference's snapshot: a CPU copy of `args` taken first and saved when the call raises."""
    if not debug:
        return fn(*args)
    cpu_args = cpu_deep_copy_tuple(args)  # Copy them before they can be corrupted
    try:
        return fn(*args)
    except Exception as ex:
        torch.save(cpu_args, path)
        print(message)
        raise ex


def _one_of_colors(shs, colors_precomp):
    if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
        raise Exception(_MSG_COLORS)


def _one_of_cov(scales, rotations, cov3D_precomp):
    if ((scales is None or rotations is None) and cov3D_precomp is None) or \
            ((scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception(_MSG_COV)


def _or_empty(*tensors):
    """The reference's default for an argument that was not given: an empty CPU tensor (-> NULL in the library call)."""
    return tuple(torch.Tensor([]) if t is None else t for t in tensors)


class _RasterizerModule(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        with torch.no_grad():
            rs = self.raster_settings
            visible = mark_visible_native(positions, rs.viewmatrix, rs.projmatrix)
        return visible


def _make_plain(channels):
    """BASE / CF packages: CF/diff_gaussian_rasterization_contrastive_f/__init__.py:21-220."""

    class _RasterizeGaussians(torch.autograd.Function):
        @staticmethod
        def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                    raster_settings):
            rs = raster_settings
            args = (rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
                    rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, sh,
                    rs.sh_degree, rs.campos, rs.prefiltered, rs.debug)

            # a backward will follow: its accumulators are zero-filled by the forward's blend kernel (rasterize_gaussians_native)
            # (needs_input_grad is requires_grad of the inputs whatever the grad mode: render.py's no_grad forwards of a model whose
            # parameters require grad would zero 128 MB per view for a backward that never comes)
            prezero = _opts.grad_mode and bool(any(ctx.needs_input_grad)) and not rs.debug
            # (the native forward is looked up in this module when the call is made: tests replace it)
            num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer = _snapshot_call(
                rs.debug, args, lambda bg, m3, col, op, *rest: rasterize_gaussians_native(
                    channels, False, bg, m3, col, op, None, *rest, prezero=prezero), *_SNAPSHOT_FW)
            ctx.raster_settings = rs
            ctx.num_rendered = num_rendered
            ctx.mi_notes = _take_notes(geomBuffer)   # flags + who may skip the fills: the first backward claims them
            ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer,
                                  binningBuffer, imgBuffer)
            ctx.mark_non_differentiable(radii)
            # autograd would otherwise hand backward a zero-filled int32 (P,) "gradient" for radii on every call (a 4-MB fill)
            ctx.set_materialize_grads(False)
            ctx.out_shape = tuple(color.shape)
            return color, radii

        @staticmethod
        def backward(ctx, grad_out_color, _):
            num_rendered = ctx.num_rendered
            rs = ctx.raster_settings
            if grad_out_color is None:   # the image was not used: what autograd would have materialised
                grad_out_color = torch.zeros(ctx.out_shape, dtype=torch.float32, device=ctx.saved_tensors[1].device)
            (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer, binningBuffer,
             imgBuffer) = ctx.saved_tensors
            args = (rs.bg, means3D, radii, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
                    rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, grad_out_color, sh, rs.sh_degree, rs.campos,
                    geomBuffer, num_rendered, binningBuffer, imgBuffer, rs.debug)
            prezeroed, pack_zeroed = ctx.mi_notes.claim()
            feat_only = _features_only_applies(channels, colors_precomp, ctx.needs_input_grad, rs.debug)
            (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh,
             grad_scales, grad_rotations) = _snapshot_call(
                rs.debug, args, lambda *a: rasterize_gaussians_backward_native(
                    channels, False, *a[:13], None, *a[13:], flags=ctx.mi_notes.flags, prezeroed=prezeroed,
                    pack_zeroed=pack_zeroed, features_only=feat_only), *_SNAPSHOT_BW)
            return (grad_means3D, grad_means2D, grad_sh, grad_colors_precomp, grad_opacities, grad_scales,
                    grad_rotations, grad_cov3Ds_precomp, None)

    def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                            raster_settings):
        # grad mode as the CALLER sees it (inside Function.forward it is always off): decides whether the forward leaves the backward's
        # buffers zeroed (prezero).  Every entry point that reaches .apply must set it; it is put back afterwards so that a caller
        # reaching .apply by another path never sees the value of somebody else's call (the backward fills for itself when in doubt).
        _opts.grad_mode = torch.is_grad_enabled()
        try:
            return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                             cov3Ds_precomp, raster_settings)
        finally:
            _opts.grad_mode = True

    class GaussianRasterizer(_RasterizerModule):
        def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                    cov3D_precomp=None):
            _one_of_colors(shs, colors_precomp)
            _one_of_cov(scales, rotations, cov3D_precomp)
            shs, colors_precomp, scales, rotations, cov3D_precomp = _or_empty(shs, colors_precomp, scales, rotations, cov3D_precomp)
            return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                       cov3D_precomp, self.raster_settings)

    return _RasterizeGaussians, rasterize_gaussians, GaussianRasterizer


def _make_depth():
    """DEPTH package: DEPTH/diff_gaussian_rasterization_depth/__init__.py:21-391."""
    channels = 3

    class _RasterizeGaussians(torch.autograd.Function):
        @staticmethod
        def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, mask, scales, rotations, cov3Ds_precomp,
                    raster_settings):
            rs = raster_settings
            args = (rs.bg, means3D, colors_precomp, opacities, mask, scales, rotations, rs.scale_modifier,
                    cov3Ds_precomp, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height,
                    rs.image_width, sh, rs.sh_degree, rs.campos, rs.prefiltered, rs.debug)
            # (never asks for prezero: its backward fills for itself)
            num_rendered, color, out_mask, depth, radii, geomBuffer, binningBuffer, imgBuffer = _snapshot_call(
                rs.debug, args, lambda *a: rasterize_gaussians_native(channels, True, *a), *_SNAPSHOT_FW)
            ctx.mask_shape = mask.shape
            ctx.raster_settings = rs
            ctx.num_rendered = num_rendered
            ctx.mi_notes = _take_notes(geomBuffer)
            ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer,
                                  binningBuffer, imgBuffer)
            ctx.mark_non_differentiable(radii)
            ctx.set_materialize_grads(False)   # see the plain variant: no zero-filled "gradients" for radii / unused outputs
            ctx.out_shapes = (tuple(color.shape), tuple(out_mask.shape))
            return color, out_mask, depth, radii

        @staticmethod
        def backward(ctx, grad_out_color, grad_out_mask, grad_out_depth, _):
            num_rendered = ctx.num_rendered
            rs = ctx.raster_settings
            dev_ = ctx.saved_tensors[1].device
            if grad_out_color is None:
                grad_out_color = torch.zeros(ctx.out_shapes[0], dtype=torch.float32, device=dev_)
            if grad_out_mask is None:
                grad_out_mask = torch.zeros(ctx.out_shapes[1], dtype=torch.float32, device=dev_)
            (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer, binningBuffer,
             imgBuffer) = ctx.saved_tensors
            args = (rs.bg, means3D, radii, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
                    rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, grad_out_color, grad_out_mask, sh,
                    rs.sh_degree, rs.campos, geomBuffer, num_rendered, binningBuffer, imgBuffer, rs.debug)
            (grad_means2D, grad_colors_precomp, grad_opacities, grad_mask, grad_means3D, grad_cov3Ds_precomp, grad_sh,
             grad_scales, grad_rotations) = _snapshot_call(
                rs.debug, args, lambda *a: rasterize_gaussians_backward_native(channels, True, *a, flags=ctx.mi_notes.flags),
                *_SNAPSHOT_BW)
            # the reference hands back (P,1) (DEPTH/rasterize_points.cu:167), which autograd accepts only for a (P,1)
            # mask; same P values here, shaped like the mask that came in, so that (P,) works as well
            grad_mask = grad_mask.view(ctx.mask_shape)
            return (grad_means3D, grad_means2D, grad_sh, grad_colors_precomp, grad_opacities, grad_mask, grad_scales,
                    grad_rotations, grad_cov3Ds_precomp, None)

    class _RasterizeMaskGaussians(torch.autograd.Function):
        # DEPTH/diff_gaussian_rasterization_depth/__init__.py:185-292
        @staticmethod
        def forward(ctx, means3D, means2D, opacities, mask, scales, rotations, cov3Ds_precomp, raster_settings):
            rs = raster_settings
            num_rendered, out_mask, radii, geomBuffer, binningBuffer, imgBuffer = rasterize_mask_gaussians_native(
                means3D, opacities, mask, scales, rotations, rs.scale_modifier, cov3Ds_precomp, rs.viewmatrix,
                rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, rs.prefiltered, rs.debug)
            ctx.raster_settings = rs
            ctx.num_rendered = num_rendered
            ctx.mask_shape = mask.shape
            ctx.mi_notes = _take_notes(geomBuffer)
            ctx.save_for_backward(means3D, means2D, opacities, scales, rotations, cov3Ds_precomp, radii, geomBuffer,
                                  binningBuffer, imgBuffer)
            ctx.mark_non_differentiable(radii)
            ctx.set_materialize_grads(False)
            ctx.out_shape = tuple(out_mask.shape)
            return out_mask, radii

        @staticmethod
        def backward(ctx, grad_out_mask, _):
            rs = ctx.raster_settings
            if grad_out_mask is None:
                grad_out_mask = torch.zeros(ctx.out_shape, dtype=torch.float32, device=ctx.saved_tensors[0].device)
            (means3D, means2D, opacities, scales, rotations, cov3Ds_precomp, radii, geomBuffer, binningBuffer,
             imgBuffer) = ctx.saved_tensors
            grad_mask = rasterize_mask_gaussians_backward_native(means3D, grad_out_mask, geomBuffer, ctx.num_rendered,
                                                                 binningBuffer, imgBuffer, rs.debug,
                                                                 flags=ctx.mi_notes.flags).view(ctx.mask_shape)
            # only the mask receives a real gradient; the reference hands ZEROS (not None) to every other input
            # (DEPTH/.../__init__.py:278-290) -- kept, but shaped like the inputs so autograd accepts them.
            z = [torch.zeros_like(t) if need else None for t, need in
                 zip((means3D, means2D, opacities), ctx.needs_input_grad[0:3])]
            z2 = [torch.zeros_like(t) if (need and t.numel()) else None for t, need in
                  zip((scales, rotations, cov3Ds_precomp), ctx.needs_input_grad[4:7])]
            return z[0], z[1], z[2], grad_mask, z2[0], z2[1], z2[2], None

    def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, mask, scales, rotations, cov3Ds_precomp,
                            raster_settings):
        return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, mask, scales, rotations,
                                         cov3Ds_precomp, raster_settings)

    def rasterize_mask_gaussians(means3D, means2D, opacities, mask, scales, rotations, cov3Ds_precomp,
                                 raster_settings):
        return _RasterizeMaskGaussians.apply(means3D, means2D, opacities, mask, scales, rotations, cov3Ds_precomp,
                                             raster_settings)

    class GaussianRasterizer(_RasterizerModule):
        def forward(self, means3D, means2D, opacities, mask, shs=None, colors_precomp=None, scales=None,
                    rotations=None, cov3D_precomp=None):
            _one_of_colors(shs, colors_precomp)
            _one_of_cov(scales, rotations, cov3D_precomp)
            shs, colors_precomp, scales, rotations, cov3D_precomp = _or_empty(shs, colors_precomp, scales, rotations, cov3D_precomp)
            return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, mask, scales, rotations,
                                       cov3D_precomp, self.raster_settings)

        def forward_mask(self, means3D, means2D, opacities, mask, scales=None, rotations=None, cov3D_precomp=None):
            _one_of_cov(scales, rotations, cov3D_precomp)
            scales, rotations, cov3D_precomp = _or_empty(scales, rotations, cov3D_precomp)
            return rasterize_mask_gaussians(means3D, means2D, opacities, mask, scales, rotations, cov3D_precomp,
                                            self.raster_settings)

    return _RasterizeGaussians, _RasterizeMaskGaussians, rasterize_gaussians, rasterize_mask_gaussians, \
        GaussianRasterizer


_PLAIN_CACHE = {}


def make_auto_rasterizer(default_channels: int = 32):
    """The feature rasterizer with the channel count taken from the call: NUM_CHANNELS is a compile-time constant of the
    reference's package (CF/cuda_rasterizer/config_contrastive_f.h:15 = 32; a user who trains 64-D features edits the header and
    rebuilds), here a run-time argument of the C-ABI -- so the drop-in reads it off `colors_precomp` (or the background
    colour when SH colours are given), falling back to `default_channels`.  Returns (rasterize_gaussians, GaussianRasterizer)
    with the reference's signatures."""

    def _channels(colors_precomp, raster_settings):
        if colors_precomp is not None and torch.is_tensor(colors_precomp) and colors_precomp.dim() == 2 and colors_precomp.size(1) > 0:
            return int(colors_precomp.size(1))
        bg = getattr(raster_settings, "bg", None)
        if torch.is_tensor(bg) and bg.numel() > 0:
            return int(bg.numel())
        return int(default_channels)

    def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
        return make_rasterizer(_channels(colors_precomp, raster_settings))[1](means3D, means2D, sh, colors_precomp, opacities, scales,
                                                                             rotations, cov3Ds_precomp, raster_settings)

    class GaussianRasterizer(_RasterizerModule):
        def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None):
            impl = make_rasterizer(_channels(colors_precomp, self.raster_settings))[2](self.raster_settings)
            return impl(means3D=means3D, means2D=means2D, opacities=opacities, shs=shs, colors_precomp=colors_precomp, scales=scales,
                        rotations=rotations, cov3D_precomp=cov3D_precomp)

    return rasterize_gaussians, GaussianRasterizer


def make_rasterizer(channels: int):
    """(autograd Function, functional wrapper, nn.Module) for the plain C-channel rasterizer."""
    if channels not in _PLAIN_CACHE:
        _PLAIN_CACHE[channels] = _make_plain(channels)
    return _PLAIN_CACHE[channels]


_DEPTH = None


def make_depth_rasterizer():
    global _DEPTH
    if _DEPTH is None:
        _DEPTH = _make_depth()
    return _DEPTH
