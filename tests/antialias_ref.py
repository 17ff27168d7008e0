"""References of the antialiased render mode (include/mi_rast.h: MI_RAST_ANTIALIAS) for
tests/test_antialias_host.py (CPU) and tests/test_antialias.py (GPU).

The mode scales the opacity of every Gaussian by h = sqrt(max(0.000025, det(cov2D) / det(cov2D + 0.3 I))).  The reference has no
counterpart, so the truth is float64 autograd: h_factor() below, built from the same quirk-detached 2-D covariance as
tests/dense_ref.py: render_dense(reference_quirks=True), times the opacities, fed into render_dense -- autograd differentiates
through the blend and through h.  The two float32 restatements of the rule of tests/raster_edge_ref.py:
  (i)  the same expression in float32;
  (ii) the unchanged CPU oracle given opacity * h32 as its opacities, dL_dopacity = h32 * dL_dw, and the h path added by float32
       autograd of h32 with the upstream gradient opacity * dL_dw.
"""
from __future__ import annotations

import copy
import math

import numpy as np
import torch

from oracle import saga_oracle as so
from tests import raster_edge_ref as er
from tests.dense_ref import build_rotation, render_dense

RHO_FLOOR = 0.000025
H_FLOOR = 0.005


def cov2d(means3D, viewmatrix, W, H, tanfovx, tanfovy, *, scales=None, rotations=None, cov3D_precomp=None, scale_modifier=1.0):
    """(a0, b, c0): the 2-D covariance before the dilation, as render_dense(reference_quirks=True) forms it (a clamped t.x / t.y
    is a constant), in the dtype of the inputs."""
    dt = means3D.dtype
    P = means3D.shape[0]
    hom = torch.cat([means3D, torch.ones(P, 1, dtype=dt)], 1)
    p_view = hom @ viewmatrix
    if cov3D_precomp is None:
        L = build_rotation(rotations) @ torch.diag_embed(scale_modifier * scales)
        Sigma = L @ L.transpose(1, 2)
    else:
        c = cov3D_precomp
        Sigma = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], 1).reshape(-1, 3, 3)
    focal_x, focal_y = W / (2.0 * tanfovx), H / (2.0 * tanfovy)
    tx, ty, tz = p_view[:, 0], p_view[:, 1], p_view[:, 2]
    limx, limy = 1.3 * tanfovx, 1.3 * tanfovy
    txtz, tytz = tx / tz, ty / tz
    txc = torch.clamp(txtz, -limx, limx) * tz
    tyc = torch.clamp(tytz, -limy, limy) * tz
    txc = torch.where((txtz < -limx) | (txtz > limx), txc.detach(), txc)
    tyc = torch.where((tytz < -limy) | (tytz > limy), tyc.detach(), tyc)
    zero = torch.zeros_like(tz)
    J = torch.stack([focal_x / tz, zero, -(focal_x * txc) / (tz * tz), zero, focal_y / tz, -(focal_y * tyc) / (tz * tz),
                     zero, zero, zero], 1).reshape(-1, 3, 3)
    Tm = J @ viewmatrix[:3, :3].T
    cov = Tm @ Sigma @ Tm.transpose(1, 2)
    return cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]


def h_of_cov(a0, b, c0):
    """(h, rho) of the definition, differentiable: the floor cuts the gradient (rho at or under it: h is the constant 0.005)."""
    det0 = a0 * c0 - b * b
    det1 = (a0 + 0.3) * (c0 + 0.3) - b * b
    rho = det0 / det1
    return torch.sqrt(torch.clamp(rho, min=RHO_FLOOR)), rho


def h_factor(means3D, viewmatrix, W, H, tanfovx, tanfovy, **kw):
    """h per Gaussian, (P,), differentiable in means3D and scales / rotations or cov3D_precomp, in the dtype given."""
    return h_of_cov(*cov2d(means3D, viewmatrix, W, H, tanfovx, tanfovy, **kw))[0]


def render_dense_aa(means3D, opacities, viewmatrix, projmatrix, campos, bg, W, H, tanfovx, tanfovy, **kw):
    """render_dense with the mode: opacities * h in place of the opacities, one autograd graph."""
    h = h_factor(means3D, viewmatrix, W, H, tanfovx, tanfovy, scales=kw.get("scales"), rotations=kw.get("rotations"),
                 cov3D_precomp=kw.get("cov3D_precomp"), scale_modifier=kw.get("scale_modifier", 1.0))
    return render_dense(means3D, opacities * h.reshape(opacities.shape), viewmatrix, projmatrix, campos, bg, W, H, tanfovx, tanfovy, **kw)


def h32_of(inp):
    """(h32, rho32, leaves, h32 tensor) of restatement (i) on the float32 inputs: numpy float32 arrays and the autograd handles."""
    P = np.asarray(inp.means3D).reshape(-1, 3).shape[0]
    t = lambda a, g=True: None if a is None else torch.tensor(np.asarray(a, np.float32), dtype=torch.float32, requires_grad=g)
    lv = dict(means3D=t(np.asarray(inp.means3D).reshape(P, 3)), scales=t(inp.scales), rots=t(inp.rotations), cov=t(inp.cov3D_precomp))
    a0, b, c0 = cov2d(lv["means3D"], t(inp.viewmatrix, False), inp.image_width, inp.image_height, inp.tanfovx, inp.tanfovy,
                      scales=lv["scales"], rotations=lv["rots"], cov3D_precomp=lv["cov"], scale_modifier=inp.scale_modifier)
    h, rho = h_of_cov(a0, b, c0)
    return h.detach().numpy(), rho.detach().numpy(), lv, h


def oracle_classes_aa(inp, dL, dLm):
    """Restatement (ii): the oracle on opacity * h32, its gradients completed by the chain rule through h32 (module docstring)."""
    h32, _, lv, h_t = h32_of(inp)
    op = np.asarray(inp.opacities, np.float32).reshape(-1)
    inp_w = copy.copy(inp)
    inp_w.opacities = (op * h32).astype(np.float32).reshape(-1, 1)
    out, fwd = er.oracle_classes(inp_w, dL, dLm)
    if "dL_dopacity" in out:
        g_w = out["dL_dopacity"].reshape(-1).astype(np.float32)
        out["dL_dopacity"] = (h32 * g_w).astype(np.float64).reshape(-1, 1)
        keys = [k for k in ("means3D", "scales", "rots", "cov") if lv[k] is not None]
        gs = torch.autograd.grad(h_t, [lv[k] for k in keys], grad_outputs=torch.tensor(op * g_w), allow_unused=True)
        names = dict(means3D="dL_dmeans3D", scales="dL_dscales", rots="dL_drotations", cov="dL_dcov3D")
        for k, g in zip(keys, gs):
            if g is not None:
                # (dL_dscales: classes_of_grads holds modifier * the reference's quirk value, the true derivative -- so is autograd's)
                add = g.numpy().astype(np.float32)
                out[names[k]] = (out[names[k]].astype(np.float32) + add).astype(np.float64)
    return out, fwd


def h_path32(inp):
    """What restatement (ii) adds per unit of opacity * dL_dw: the float32 autograd gradient of h32 in every geometry leaf, (P, .)."""
    _, _, lv, h_t = h32_of(inp)
    keys = [k for k in ("means3D", "scales", "rots", "cov") if lv[k] is not None]
    gs = torch.autograd.grad(h_t.sum(), [lv[k] for k in keys], allow_unused=True)
    return {k: (np.zeros(tuple(lv[k].shape), np.float32) if g is None else g.numpy()) for k, g in zip(keys, gs)}


class AAReference(er.Reference):
    """er.Reference of a scene rendered with the mode: dense64 / dense32 through render_dense_aa, the oracle through
    oracle_classes_aa; margins, excused groups and the rule are the parent's, evaluated on opacity * h.

    The existing test modules stay as they are, so this class has no hook in er.Reference to use: __init__ below restates
    er.Reference.__init__ (keep the two in step when that one changes) and swaps the module global er.render_dense while er._dense
    runs -- not thread-safe: build references from one thread, as pytest does.  Importing this module adds er.TABLES["aa"]."""

    def __init__(self, case, inp):
        self.case = case
        self.inp = inp
        inp.mask_only = False
        self.dL, self.dLm = er.gradient_images(inp, case[4])
        threads = torch.get_num_threads()
        saved = er.render_dense
        try:
            er.render_dense = render_dense_aa          # er._dense builds the leaves and calls it: same leaves through both paths
            torch.set_num_threads(min(4, threads))
            self.d64, self.mag, ref = er._dense(inp, self.dL, self.dLm, torch.float64, True, True, 4)
            torch.set_num_threads(1)
            self.d32, _, ref32 = er._dense(inp, self.dL, self.dLm, torch.float32, True, False)
        finally:
            er.render_dense = saved
            torch.set_num_threads(threads)
        self.oracle, self.fwd = oracle_classes_aa(inp, self.dL, self.dLm)
        self.classes = [k for k in self.d64]
        self.radii = ref["radii"].numpy()
        self.radii32 = ref32["radii"].numpy()
        self.tiles_touched = ref["tiles_touched"].numpy()
        self.dense = {k: (ref[k].numpy() if ref[k] is not None else None) for k in
                      ("raw_alpha", "power", "power_terms", "member", "stop_value", "alive", "weights", "alpha_eff", "sh_pre_clamp",
                       "txtz", "tytz", "view_z", "order", "contrib")}
        self._margins()
        self.h32, self.rho32, _, _ = h32_of(inp)
        t = lambda a: None if a is None else torch.tensor(np.asarray(a, np.float64))
        P = len(self.radii)
        a0, b, c0 = cov2d(t(np.asarray(inp.means3D).reshape(P, 3)), t(inp.viewmatrix), inp.image_width, inp.image_height, inp.tanfovx,
                          inp.tanfovy, scales=t(inp.scales), rotations=t(inp.rotations), cov3D_precomp=t(inp.cov3D_precomp),
                          scale_modifier=inp.scale_modifier)
        h, rho = h_of_cov(a0, b, c0)
        self.h64, self.rho64 = h.numpy(), rho.numpy()


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
MODIFIER = 0.6
AA_CONFIGS = {"rgb": ("sh3", False), "mask_depth": ("mask_depth", False), "c32": ("c32", False), "c32_cov": ("c32", True)}


def _designed_aa(W, H, focal):
    """(class, centre u, v, depth, sigma px per axis, quaternion, opacity) of the Gaussians appended to the edge scene."""
    cx, cy = (W - 1) * 0.5, (H - 1) * 0.5
    qz = lambda deg: (math.cos(math.radians(deg) / 2), 0.0, 0.0, math.sin(math.radians(deg) / 2))
    s01 = math.sqrt(0.3 / 9.0)                       # s^2 / (s^2 + 0.3) = 0.1
    ox = 1.5 * 1.3 * W / 2
    return [("aa_subpixel", cx + 5.3, cy - 6.2, 6.3, (s01,) * 3, (1.0, 0.0, 0.0, 0.0), 0.9),
            ("aa_large", cx - 8.4, cy + 3.1, 6.4, (8.0,) * 3, (1.0, 0.0, 0.0, 0.0), 0.5),
            # (axis-aligned: det0 of a needle turned in the image plane is a difference of two float32 products of 250 each, noise of 3e-6 in rho)
            ("aa_needle", cx + 2.6, cy + 6.3, 6.5, (6.0, 1e-4, 1e-4), qz(0.0), 1.0),
            ("aa_faint", cx - 3.7, cy - 7.4, 6.6, (s01,) * 3, (1.0, 0.0, 0.0, 0.0), 0.03),
            ("aa_clamped", cx + ox, cy - 2.2, 6.7, (8.0, 7.0, 7.5), (0.9, 0.1, -0.2, 0.3), 0.6)]


def aa_scene(cfg, W=37, H=21, P=96):
    """(case, inputs): er.edge_case(cfg, W, H, P) at scale_modifier 0.6 with the designed Gaussians of the mode appended (P == 1:
    the first designed Gaussian of the edge scene alone, as there)."""
    base, cov = AA_CONFIGS[cfg]
    case = er.edge_case(base, W, H, P)
    v = case[5]._replace(modifier=MODIFIER, cov=False)
    inp = er.make_inputs(case[:5] + (v,))
    case = ("aa",) + case[1:5] + (v,)     # scene kind "aa": judged with AA_TABLE below
    if P != 1:
        # One change to the edge scene: its saturated stack Gaussian (opacity 1, sigma 8 px) has w = 0.99533 under the mode, and
        # w exp(power) meets the 0.99 clamp within 8e-7 on pixel (34, 3), next to the stack pixel -- a decision margin that would excuse
        # designed Gaussians.  At sigma 9 px (w = 0.99631) the stack pixel is still saturated and the clamp's contour passes 4e-4 or
        # more (relative) from every pixel centre.
        k = [i for i, c in enumerate(inp.classes) if c == "stack" and float(inp.opacities[i, 0]) == 1.0]
        assert len(k) == 1
        inp.scales[k[0]] *= np.float32(9.0 / 8.0)
        focal = 0.9 * max(W, H)
        rows = _designed_aa(W, H, focal)
        n = len(rows)
        cx, cy = (W - 1) * 0.5, (H - 1) * 0.5
        rng = np.random.default_rng(77)
        f32 = lambda a, k: np.asarray(a, np.float32).reshape(n, k)
        inp.means3D = np.concatenate([inp.means3D, f32([((u - cx) * z / focal, (v_ - cy) * z / focal, z) for _, u, v_, z, *_ in rows], 3)])
        inp.scales = np.concatenate([inp.scales, f32([tuple(np.asarray(s) * z / focal / MODIFIER) for _, _, _, z, s, _, _ in rows], 3)])
        inp.rotations = np.concatenate([inp.rotations, f32([r[5] for r in rows], 4)])
        inp.opacities = np.concatenate([inp.opacities, f32([r[6] for r in rows], 1)])
        if inp.colors_precomp is not None:
            f = rng.normal(0, 1, (n, inp.channels))
            f = np.abs(f) if inp.channels == 3 else f / np.linalg.norm(f, axis=1, keepdims=True)
            inp.colors_precomp = np.concatenate([inp.colors_precomp, f.astype(np.float32)])
        if inp.shs is not None:
            inp.shs = np.concatenate([np.asarray(inp.shs).reshape(-1, 16, 3), rng.normal(0, 0.3, (n, 16, 3)).astype(np.float32)])
        if inp.mask is not None:
            inp.mask = np.concatenate([np.asarray(inp.mask).reshape(-1), rng.uniform(0, 1, n).astype(np.float32)])
        inp.classes = list(inp.classes) + [r[0] for r in rows]
    if cov:
        L = build_rotation(torch.tensor(inp.rotations, dtype=torch.float64)) @ torch.diag_embed(torch.tensor(inp.scales, dtype=torch.float64) * MODIFIER)
        S = (L @ L.transpose(1, 2)).numpy()
        inp.cov3D_precomp = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32)
        inp.scales = inp.rotations = None
    return case + (cfg,), inp


# ---- the rule --------------------------------------------------------------------------------------------------------------------
# er.MUTUAL, but for the classes in which the two float32 restatements do not pass it against each other on these scenes
# (tests/test_antialias_host.py asserts the mutual check): those are recalibrated on the CPU by er.calibrate()'s own procedure over
# the four scenes of AA_CONFIGS -- `python -m tests.antialias_ref` prints the table -- never against the product.
#   dL_dsh: under er.MUTUAL's (16, 2^-21) the worst mutual error / bound is 1.138 (rgb and mask_depth, SH degree 3 at modifier 0.6).
AA_RECALIBRATED = {
    "dL_dsh": (32.0, -22, 0.569),
}
AA_TABLE = dict(er.MUTUAL, **AA_RECALIBRATED)
er.TABLES["aa"] = AA_TABLE


def calibrate_aa(classes=None):
    """er.calibrate()'s procedure (FLOOR lowered first) on the mutual samples of the scenes of the mode."""
    acc = {}
    for cfg in AA_CONFIGS:
        for cls, smp in er.mutual_samples(reference(cfg)).items():
            acc.setdefault(cls, []).append(smp)
    table = {}
    for cls, parts in acc.items():
        e, E, m = (np.concatenate([p[i] for p in parts]) for i in range(3))
        passes = lambda F, lf: bool((e <= np.maximum(F * E, (2.0 ** lf) * m)).all())
        k = 0
        while not passes(4.0 * 2 ** k, -22 + k):
            k += 1
        F, lf = 4.0 * 2 ** k, -22 + k
        while lf > -22 and passes(F, lf - 1):
            lf -= 1
        while F > 4 and passes(F / 2, lf):
            F /= 2
        worst = float((e / np.maximum(np.maximum(F * E, (2.0 ** lf) * m), 1e-300)).max()) if e.size else 0.0
        table[cls] = (F, lf, round(worst, 3))
    return table


_CACHE = {}


def reference(cfg, W=37, H=21, P=96) -> AAReference:
    """The three CPU evaluations of one scene of the mode, computed once per process."""
    key = (cfg, W, H, P)
    if key not in _CACHE:
        case, inp = aa_scene(cfg, W, H, P)
        _CACHE[key] = AAReference(case, inp)
    return _CACHE[key]


SMALL = ((16, 16), (1, 1), (40, 5))


def known_answer_inputs(s2, opacity=0.9, W=32, H=32, z=4.0):
    """P = 1: a Gaussian on the optical axis at depth z, isotropic 2-D variance s2 px^2, three channels of colour 1, tanfov 1."""
    from seganygaussians_amd import scenes
    focal = W / 2.0
    cam = scenes.look_at_camera(W, H, focal)
    s = math.sqrt(s2) * z / focal
    return so.Inputs(means3D=np.array([[0, 0, z]], np.float32), opacities=np.array([[opacity]], np.float32), viewmatrix=cam.viewmatrix,
                     projmatrix=cam.projmatrix, campos=cam.campos, bg=np.zeros(3, np.float32), image_width=W, image_height=H,
                     tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, channels=3, scale_modifier=1.0, sh_degree=0, shs=None,
                     colors_precomp=np.ones((1, 3), np.float32), scales=np.full((1, 3), s, np.float32),
                     rotations=np.array([[1, 0, 0, 0]], np.float32), cov3D_precomp=None, mask=None)


def dense_image(inp, antialias):
    t = lambda a: None if a is None else torch.tensor(np.asarray(a, np.float64))
    P = np.asarray(inp.means3D).reshape(-1, 3).shape[0]
    fn = render_dense_aa if antialias else render_dense
    return fn(t(np.asarray(inp.means3D).reshape(P, 3)), t(np.asarray(inp.opacities).reshape(P, 1)), t(inp.viewmatrix), t(inp.projmatrix),
              t(inp.campos), t(inp.bg), inp.image_width, inp.image_height, inp.tanfovx, inp.tanfovy, scales=t(inp.scales),
              rotations=t(inp.rotations), cov3D_precomp=t(inp.cov3D_precomp), colors_precomp=t(inp.colors_precomp),
              scale_modifier=inp.scale_modifier, reference_quirks=True)["color"].numpy()


if __name__ == "__main__":
    for k_, v_ in sorted(calibrate_aa().items()):
        print(f'    "{k_}": {v_},')
