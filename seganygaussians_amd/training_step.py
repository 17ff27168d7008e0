"""What follows loss.backward() in the RGB-Gaussian training (train_scene.py:126-138) on the MI355X:

  * FusedAdam            -- torch.optim.Adam whose step() is ONE launch over all parameter groups (scene/gaussian_model.py:170-187
                            builds six); same constructor, param_groups, state and state_dict().
  * densification_stats  -- train_scene.py:126 and GaussianModel.add_densification_stats (scene/gaussian_model.py:582-584) in one
                            launch, no boolean-mask indexing, no host synchronisation.
  * densify_and_prune    -- scene/gaussian_model.py:566-578 (N = 2) as plan / scan / gather kernels with ONE host read (the counts);
                            rebinds the optimizer's parameters and state the way densification_postfix and prune_points leave them.
  * fused_*              -- the three GaussianModel methods install_dropin(fuse_training_step=True) binds.

The kernels need contiguous float32 tensors on one GPU.  FusedAdam.step() falls back to torch.optim.Adam.step() for anything else
(that is the same optimizer, not another implementation of the kernels); the two densification functions have no CPU path."""
from __future__ import annotations

import ctypes as C
import math

import torch
from torch.optim.optimizer import _get_scalar_dtype     # the dtype torch.optim.Adam gives its 'step'

from . import _lib
from ._ffi import check, stream_ptr

GROUP_KINDS = {"xyz": _lib.MI_TRAIN_XYZ, "scaling": _lib.MI_TRAIN_SCALING, "rotation": _lib.MI_TRAIN_ROTATION}     # every other name: a copy
_COPY, _MOMENT = _lib.MI_TRAIN_COPY, _lib.MI_TRAIN_MOMENT
ADAM_MAX_TENSORS = _lib.MI_TRAIN_ADAM_MAX_TENSORS


def _dense_f32(t) -> bool:
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and not t.is_sparse and t.is_contiguous()


def _ptr_table(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


class FusedAdam(torch.optim.Adam):
    """torch.optim.Adam with the step of all groups in one HIP launch (16 tensors per launch).  State entries are those of
    torch.optim.Adam ('step', 'exp_avg', 'exp_avg_sq'), so a state_dict() moves between the two classes either way and the reference's
    cat_tensors_to_optimizer / _prune_optimizer / replace_tensor_to_optimizer work on it unchanged."""

    @classmethod
    def from_optimizer(cls, opt: torch.optim.Adam) -> "FusedAdam":
        """A FusedAdam over the same parameters, groups (names and learning rates included) and state as `opt`."""
        new = cls([dict(g, params=list(g["params"])) for g in opt.param_groups], **opt.defaults)
        for p, st in opt.state.items():
            new.state[p] = st
        return new

    def _fusable(self) -> bool:
        for group in self.param_groups:
            if group["weight_decay"] != 0 or group["amsgrad"] or group["maximize"] or group.get("capturable") or group.get("differentiable"):
                return False
            if any(isinstance(x, torch.Tensor) for x in (group["lr"], group["eps"], *group["betas"])):
                return False
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state.get(p, {})
                tensors = [p, p.grad] + [st[k] for k in ("exp_avg", "exp_avg_sq") if k in st]
                if not all(_dense_f32(t) and t.device == p.device and t.shape == p.shape for t in tensors):
                    return False
        return True

    @torch.no_grad()
    def step(self, closure=None):
        if not self._fusable():
            base = torch.optim.Adam.step
            if getattr(base, "hooked", False):      # the step hooks already run around this method
                base = getattr(base, "__wrapped__", base)
            return base(self, closure)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        launches = {}
        for group in self.param_groups:
            beta1, beta2 = (float(b) for b in group["betas"])
            lr, eps = float(group["lr"]), float(group["eps"])
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if len(state) == 0:                 # as torch.optim.Adam._init_group
                    state["step"] = torch.tensor(0.0, dtype=_get_scalar_dtype())
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if not isinstance(state["step"], torch.Tensor):
                    state["step"] = torch.tensor(float(state["step"]), dtype=_get_scalar_dtype())
                state["step"] += 1
                t = float(state["step"])
                key = (p.device, 1.0 / math.sqrt(1.0 - beta2 ** t), beta1, beta2, eps)
                launches.setdefault(key, []).append((p, p.grad, state["exp_avg"], state["exp_avg_sq"], lr / (1.0 - beta1 ** t)))
        L = _lib.load()
        for (dev, inv_sqrt_bc2, beta1, beta2, eps), rows in launches.items():
            with torch.cuda.device(dev):
                for at in range(0, len(rows), ADAM_MAX_TENSORS):
                    part = rows[at:at + ADAM_MAX_TENSORS]
                    n = len(part)
                    check(L.mi_train_adam_step(n, *(_ptr_table([r[k].data_ptr() if r[k].numel() else None for r in part]) for k in range(4)),
                                               (C.c_size_t * n)(*(r[0].numel() for r in part)), (C.c_double * n)(*(r[4] for r in part)),
                                               inv_sqrt_bc2, beta1, beta2, eps, stream_ptr(dev)))
        return loss


def densification_stats(accum, denom, viewspace_grad, radii, max_radii2D=None) -> None:
    """In place, for the rows with radii > 0: accum += |viewspace_grad[:, :2]|, denom += 1 and, when given,
    max_radii2D = max(max_radii2D, radii).  Replaces train_scene.py:126 together with gaussians.add_densification_stats(...):

        densification_stats(gaussians.xyz_gradient_accum, gaussians.denom, viewspace_point_tensor.grad, radii, gaussians.max_radii2D)

    accum, denom: float32 (P, 1) or (P,); viewspace_grad: float32 (P, 3); radii: (P,) int32 (another integer type or a bool mask is
    converted); max_radii2D: float32 (P,).  One launch, no host synchronisation."""
    if not isinstance(viewspace_grad, torch.Tensor) or viewspace_grad.dim() != 2 or viewspace_grad.shape[1] != 3:
        raise ValueError(f"densification_stats: viewspace_grad must be (P, 3), got {tuple(getattr(viewspace_grad, 'shape', ()))}")
    P = int(viewspace_grad.shape[0])
    outs = [("accum", accum), ("denom", denom)] + ([("max_radii2D", max_radii2D)] if max_radii2D is not None else [])
    for name, t in outs:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != P or not t.is_contiguous():
            raise ValueError(f"densification_stats: {name} must be a contiguous float32 tensor of {P} elements")
    if not isinstance(radii, torch.Tensor) or radii.numel() != P or radii.is_floating_point():
        raise ValueError(f"densification_stats: radii must be an integer or bool tensor of {P} elements")
    if viewspace_grad.dtype != torch.float32:
        raise ValueError(f"densification_stats: viewspace_grad must be float32, got {viewspace_grad.dtype}")
    dev = viewspace_grad.device
    for name, t in outs + [("viewspace_grad", viewspace_grad), ("radii", radii)]:
        if not t.is_cuda or t.device != dev:
            raise ValueError(f"densification_stats: {name} must be on the GPU of viewspace_grad, got {t.device} (there is no CPU fallback)")
    if P == 0:
        return
    L = _lib.load()
    grad = viewspace_grad.contiguous()
    radii = radii.to(torch.int32).contiguous()
    with torch.cuda.device(dev):
        check(L.mi_train_densify_stats(P, radii.data_ptr(), grad.data_ptr(), accum.data_ptr(), denom.data_ptr(),
                                       None if max_radii2D is None else max_radii2D.data_ptr(), stream_ptr(dev)))


def densify_and_prune(params: dict, optimizer, accum, denom, max_radii2D, max_grad, min_opacity, extent, percent_dense, max_screen_size):
    """scene/gaussian_model.py:566-578 with N = 2.  params: name -> float32 (P, ...) GPU tensor, with at least 'xyz', 'scaling',
    'rotation' and 'opacity' (the reference's group names; any other name is copied row for row).  optimizer: None, or an optimizer
    with one parameter per group and a 'name' per group, as scene/gaussian_model.py:175-187 builds it.

    Returns (new_params, accum, denom, max_radii2D): new leaf tensors that require grad, and the three statistics zeroed at the new
    length.  Rows: originals that were not split, clones, first children, second children, minus what the final prune deletes.  The
    optimizer's groups point at the new tensors; the moments of surviving originals are kept, those of new rows are zero.  The
    normal samples are drawn with the reference's own call under the caller's seed.  One host read (the counts)."""
    for name in ("xyz", "scaling", "rotation", "opacity"):
        if name not in params:
            raise ValueError(f"densify_and_prune: params lacks '{name}'")
    if not float(max_grad) > 0.0:
        raise ValueError("densify_and_prune: max_grad must be > 0 (at 0 the reference selects its own zero-padded clone rows)")
    xyz = params["xyz"]
    P = int(xyz.shape[0])
    dev = xyz.device
    for name, t in list(params.items()) + [("accum", accum), ("denom", denom)]:
        if not _dense_f32(t.detach()) or t.device != dev or t.shape[0] != P:
            raise ValueError(f"densify_and_prune: {name} must be a contiguous float32 tensor of {P} rows on the GPU of xyz (there is no CPU fallback)")
    for name, cols in (("xyz", 3), ("scaling", 3), ("rotation", 4), ("opacity", 1)):
        if params[name].numel() != P * cols:
            raise ValueError(f"densify_and_prune: {name} must have {cols} columns")
    if accum.numel() != P or denom.numel() != P:
        raise ValueError(f"densify_and_prune: accum and denom must have {P} elements")
    groups = {}
    if optimizer is not None:
        for g in optimizer.param_groups:
            if g.get("name") in params:
                if len(g["params"]) != 1 or g["params"][0] is not params[g["name"]]:
                    raise ValueError(f"densify_and_prune: the optimizer's group '{g['name']}' does not hold params['{g['name']}']")
                groups[g["name"]] = g

    def zeros_stats(n):
        return (torch.zeros((n, 1), device=dev), torch.zeros((n, 1), device=dev), torch.zeros((n,), device=dev))

    if P == 0:
        return dict(params), *zeros_stats(0)
    L = _lib.load()
    src, kinds, names = [], [], []      # names: (group name, state key or None)
    for name, t in params.items():
        src.append(t.detach())
        kinds.append(GROUP_KINDS.get(name, _COPY))
        names.append((name, None))
        st = optimizer.state.get(t) if name in groups else None
        if st:
            for key in ("exp_avg", "exp_avg_sq"):
                if not _dense_f32(st[key]) or st[key].shape != t.shape:
                    raise ValueError(f"densify_and_prune: the optimizer's {key} of '{name}' must be a contiguous float32 GPU tensor like the parameter")
                src.append(st[key])
                kinds.append(_MOMENT)
                names.append((name, key))
    if len(src) > _lib.MI_TRAIN_DENSIFY_MAX_TENSORS:
        raise ValueError(f"densify_and_prune: {len(src)} tensors, at most {_lib.MI_TRAIN_DENSIFY_MAX_TENSORS}")
    cols = [t.numel() // P for t in src]
    live = [k for k, c in enumerate(cols) if c > 0]      # f_rest at SH degree 0 has no column: nothing to gather
    with torch.cuda.device(dev):
        stream = stream_ptr(dev)
        ws = torch.empty((L.mi_train_densify_workspace_bytes(P),), device=dev, dtype=torch.uint8)
        split_rows = torch.empty((P,), device=dev, dtype=torch.int64)
        check(L.mi_train_densify_plan(P, accum.data_ptr(), denom.data_ptr(), params["scaling"].data_ptr(), params["opacity"].data_ptr(),
                                      float(max_grad), float(min_opacity), float(extent), float(percent_dense), 1 if max_screen_size else 0,
                                      ws.data_ptr(), ws.numel(), split_rows.data_ptr(), stream))
        counts = (C.c_int * len(_lib.MI_TRAIN_COUNTS))()
        check(L.mi_train_densify_counts(P, ws.data_ptr(), ws.numel(), counts, stream))
        _, n_split, n_orig, n_clone, n_child = (int(c) for c in counts)
        new_rows = n_orig + n_clone + 2 * n_child
        # scene/gaussian_model.py:529-531, the reference's own draw: children that the final prune deletes consume theirs too
        samples = None
        if n_split:
            stds = torch.exp(params["scaling"].detach()[split_rows[:n_split]]).repeat(2, 1)
            samples = torch.normal(mean=torch.zeros((stds.size(0), 3), device=dev), std=stds)
        dst = [torch.empty((new_rows,) + tuple(t.shape[1:]), device=dev, dtype=torch.float32) for t in src]
        n = len(live)
        check(L.mi_train_densify_apply(P, counts, n, _ptr_table([src[k].data_ptr() for k in live]),
                                       _ptr_table([dst[k].data_ptr() if new_rows else None for k in live]), (C.c_int * n)(*(cols[k] for k in live)),
                                       (C.c_int * n)(*(kinds[k] for k in live)),
                                       None if samples is None else samples.data_ptr(), ws.data_ptr(), ws.numel(), stream))
    out, moments = {}, {}
    for (name, key), t in zip(names, dst):
        if key is None:
            out[name] = torch.nn.Parameter(t.requires_grad_(True))
        else:
            moments[(name, key)] = t
    for name, g in groups.items():
        st = optimizer.state.pop(g["params"][0], None)
        g["params"][0] = out[name]
        if st:
            if (name, "exp_avg") in moments:
                st["exp_avg"], st["exp_avg_sq"] = moments[(name, "exp_avg")], moments[(name, "exp_avg_sq")]
            optimizer.state[out[name]] = st
    return out, *zeros_stats(new_rows)


# ---- the reference's GaussianModel (scene/gaussian_model.py), bound by install_dropin(fuse_training_step=True) ------------------

_MODEL_FIELDS = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
                 "rotation": "_rotation"}


def fused_training_setup(self, training_args):
    """The reference's training_setup, then its torch.optim.Adam swapped for a FusedAdam over the same groups."""
    self._reference_training_setup(training_args)
    self.optimizer = FusedAdam.from_optimizer(self.optimizer)


def fused_add_densification_stats(self, viewspace_point_tensor, update_filter):
    densification_stats(self.xyz_gradient_accum, self.denom, viewspace_point_tensor.grad, update_filter)


def fused_densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size):
    params = {name: getattr(self, field) for name, field in _MODEL_FIELDS.items()}
    new, self.xyz_gradient_accum, self.denom, self.max_radii2D = densify_and_prune(
        params, self.optimizer, self.xyz_gradient_accum, self.denom, self.max_radii2D, max_grad, min_opacity, extent, self.percent_dense,
        max_screen_size)
    for name, field in _MODEL_FIELDS.items():
        setattr(self, field, new[name])
