"""2D-to-3D score lifting on the MI355X: per-Gaussian votes of per-view score images, and the multi-view 3D mask (DESIGN.md
section 20; include/mi_rast.h, csrc/lift.h).

The last step of the reference's open-vocabulary segmentation, clip_utils.get_3d_mask (clip_utils/__init__.py:291-330), renders a
zero mask per camera, takes loss = -(target * rendered).sum(), calls backward() and accumulates minus the gradient into a
per-Gaussian vote that it thresholds at 0.  The render is linear in the mask, so the vote of Gaussian g is

    sum over the views of  3 * sum over the pixels p of  target(p) alpha_g(p) T_g(p)

(3: render_mask repeats the mask over three colour channels).  lift_scores() computes the inner sum for K score images of one view
in ONE front-to-back walk of the tile lists -- no image, no per-pixel state, no backward --, vote_3d_mask() sums it over the views.

float32 tensors on one GPU.  No autograd: the votes are a sum of blending weights, which the reference takes under a backward() of
its own and never differentiates; inputs that require grad are used as values.  The rows are added with float atomics: the last
bits of the votes depend on the order in which the tiles' contributions arrive.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

import torch
import torch.nn.functional as F

from . import _lib
from ._ffi import check, contig, dev_ptr, stream_ptr
from .rasterizer import _MSG_COV, _Resizer, _opts

MAX_CHANNELS = _lib.MI_RAST_LIFT_MAX_CHANNELS


class LiftState(NamedTuple):
    """What a lift (or any forward) of one geometry, camera and list mode left behind, for further lifts of the same view:
    lift_scores(..., state=...) runs the kernel alone over it and only reads the buffers."""
    num_rendered: int
    radii: torch.Tensor
    geom: torch.Tensor
    binning: torch.Tensor
    img: torch.Tensor
    width: int
    height: int
    flags: int


def _scores_3d(scores, who):
    if not isinstance(scores, torch.Tensor) or scores.dim() not in (2, 3):
        raise ValueError(f"{who}: scores must be a (K, H, W) or (H, W) tensor")
    s = scores[None] if scores.dim() == 2 else scores
    if not 1 <= s.shape[0] <= MAX_CHANNELS:
        raise ValueError(f"{who}: need 1 <= K <= {MAX_CHANNELS} score channels, got {s.shape[0]}")
    return s


def lift_scores(scores, means3D, opacities, *, scales=None, rotations=None, cov3D_precomp=None, viewmatrix=None, projmatrix=None,
                tanfovx=None, tanfovy=None, scale_modifier=1.0, prefiltered=False, out=None, state=None, return_state=False):
    """votes[g, k] = sum over the pixels p of alpha_g(p) T_g(p) scores[k, p], with alpha and T as the forward blends them.

    scores: (K, H, W) or (H, W), K <= 64; the render size is the scores' size.  Returns votes (P, K): a fresh zero tensor, or `out`
    ACCUMULATED into (rows of Gaussians that blend nowhere are not touched).  return_state: also a LiftState; state=: the kernel
    alone over the buffers of an earlier lift or forward of the same view (the geometry arguments are then not read).  Honours
    rasterizer.forward_flags(full_lists, no_cull, fast_exp, equal_runs).  Equal to dL_dcolors of the rasterizer's backward with
    dL_dpixels = scores, up to the order of the sums.  No autograd."""
    s = _scores_3d(scores, "lift_scores")
    K, H, W = (int(v) for v in s.shape)
    if means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    if state is None:
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception(_MSG_COV)
        if viewmatrix is None or projmatrix is None or tanfovx is None or tanfovy is None:
            raise ValueError("lift_scores: viewmatrix, projmatrix, tanfovx and tanfovy are required without state=")
    elif (state.width, state.height) != (W, H):
        raise ValueError(f"lift_scores: state is of a {state.width} x {state.height} view, scores are {W} x {H}")
    P, dev = int(means3D.size(0)), means3D.device
    if out is None:
        votes = torch.zeros((P, K), dtype=torch.float32, device=dev)
    else:
        if out.shape != (P, K) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
            raise ValueError(f"lift_scores: out must be a contiguous float32 ({P}, {K}) tensor on {dev}")
        votes = out
    if P == 0:
        empty = torch.empty(0, dtype=torch.uint8, device=dev)
        st = state or LiftState(0, torch.zeros(0, dtype=torch.int32, device=dev), empty, empty, empty, W, H, _opts.call_flags())
        return (votes, st) if return_state else votes
    L = _lib.load()
    s_c = contig(s.detach())
    with torch.cuda.device(dev):
        if state is not None:
            rc = L.mi_rast_lift_reuse(P, K, int(state.num_rendered), W, H, state.geom.data_ptr(), state.binning.data_ptr(),
                                      state.img.data_ptr(), dev_ptr(s_c, "scores", dev), votes.data_ptr(), int(state.flags),
                                      stream_ptr(dev))
            check(rc)
            return (votes, state) if return_state else votes
        radii = torch.zeros(P, dtype=torch.int32, device=dev)
        geom, binning, img = _Resizer(dev), _Resizer(dev), _Resizer(dev)
        t = [None if x is None else contig(x.detach()) for x in (means3D, opacities, scales, rotations, cov3D_precomp, viewmatrix, projmatrix)]
        m3_c, op_c, sc_c, rot_c, cov_c, vm_c, pm_c = t
        n = C.c_int(0)
        rc = L.mi_rast_lift(
            geom.cb, None, binning.cb, None, img.cb, None, P, K, W, H, dev_ptr(m3_c, "means3D", dev), dev_ptr(op_c, "opacities", dev),
            dev_ptr(sc_c, "scales", dev), float(scale_modifier), dev_ptr(rot_c, "rotations", dev), dev_ptr(cov_c, "cov3D_precomp", dev),
            dev_ptr(vm_c, "viewmatrix", dev), dev_ptr(pm_c, "projmatrix", dev), float(tanfovx), float(tanfovy),
            int(bool(prefiltered)), dev_ptr(s_c, "scores", dev), votes.data_ptr(), radii.data_ptr(), 0, _opts.call_flags(),
            stream_ptr(dev), C.byref(n))
    check(rc)
    if not return_state:
        return votes
    return votes, LiftState(n.value, radii, geom.tensor, binning.tensor, img.tensor, W, H, _opts.call_flags())


def state_of_forward(num_rendered, radii, geomBuffer, binningBuffer, imageBuffer, image_width, image_height, flags=None):
    """The LiftState of a native forward's results (rasterize_gaussians_native, rasterize_mask_gaussians_native): a lift over it
    reads the buffers only, so it is legal between that forward and its backward.  flags: the forward's (default: the ones the
    forward left on its geometry buffer)."""
    if flags is None:
        notes = geomBuffer.__dict__.get("mi_notes")
        flags = notes.flags if notes is not None else _opts.call_flags()
    return LiftState(int(num_rendered), radii, geomBuffer, binningBuffer, imageBuffer, int(image_width), int(image_height), int(flags))


def vote_3d_mask(cameras, scores, means3D, opacities, *, scales=None, rotations=None, cov3D_precomp=None, scale_modifier=1.0,
                 threshold=0.0):
    """The multi-view 3D mask of clip_utils.get_3d_mask (clip_utils/__init__.py:291-330): (votes > threshold, votes).

    cameras: objects with the reference's camera attributes FoVx, FoVy, image_height, image_width, world_view_transform,
    full_proj_transform.  scores: one (h, w) or (K, h, w) tensor per camera (the same K for all), None skips that view; a score image
    of another size than the camera's is resized with F.interpolate(mode="bilinear") as the reference does (:306).  The votes (P, K)
    are summed in place over the views.  They are the reference's `tmp_mask` DIVIDED BY 3 -- it repeats the mask over three colour
    channels and sums their gradients --, so their sign and the thresholded mask at 0 are the reference's."""
    if len(cameras) != len(scores):
        raise ValueError(f"vote_3d_mask: {len(cameras)} cameras but {len(scores)} score images")
    votes = None
    for cam, sc in zip(cameras, scores):
        if sc is None:
            continue
        s = _scores_3d(sc, "vote_3d_mask").to(torch.float32)
        H, W = int(cam.image_height), int(cam.image_width)
        if tuple(s.shape[-2:]) != (H, W):
            s = F.interpolate(s[None], size=(H, W), mode="bilinear")[0]
        if votes is not None and votes.shape[1] != s.shape[0]:
            raise ValueError(f"vote_3d_mask: score images of {votes.shape[1]} and of {s.shape[0]} channels")
        votes = lift_scores(s, means3D, opacities, scales=scales, rotations=rotations, cov3D_precomp=cov3D_precomp,
                            viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform,
                            tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), scale_modifier=scale_modifier, out=votes)
    if votes is None:
        votes = torch.zeros((int(means3D.size(0)), 1), dtype=torch.float32, device=means3D.device)
    return votes > threshold, votes
