"""The cut that ends the segmentation workflow on the MI355X (C entry points: include/mi_model_edit.h):
GaussianModel.segment / roll_back / clear_segment (scene/gaussian_model.py:376-472) and FeatureGaussianModel's
(scene/gaussian_model_ff.py:257-320), which the GUI's "segment3d", "roll back" and "clear" buttons, the notebooks and render.py call.

  * cut_rows        -- keep the selected rows of up to 32 tensors: plan (no host read), counts (the ONE host read), apply (a row map,
                       then one gather launch over all tensors).
  * SegmentStack    -- the state of the cuts (`level`, the reference's _mask, and `times`, its segment_times) with cut / roll_back /
                       clear / current_mask, for callers without the reference's classes.
  * segment_models  -- one plan and one host read for several models in the same state (the GUI's scene and feature pair).
  * fused_*         -- the three methods install_model_edit() binds to both of the reference's classes.

The state is `level` and `times` alone: the current rows are the original rows with level == times + 1, in row order.  Everything
is moved as 4-byte words, so every kept row is its source row bit for bit.  The kernels need contiguous float32 tensors on one GPU;
there is no CPU path."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._args import f32, no_grad_one_gpu
from ._ffi import check, stream_ptr

MAX_TENSORS = _lib.MI_EDIT_MAX_TENSORS
MAX_COLS = _lib.MI_EDIT_MAX_COLS
COUNTS = tuple(_lib.MI_EDIT_COUNTS)
PLAN_LAUNCHES, APPLY_LAUNCHES = 4, 2     # current rows, scan, selection, scan; row map, gather
EMPTY_MASK_MESSAGE = "Seems like the mask is empty, segmenting the whole point cloud. Please run seg.py first."


def _ptr_table(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def _row_mask(who, mask):
    """A bool tensor with one entry per current row; (n, 1) and the like are flattened as the reference's squeeze() does."""
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool:
        raise ValueError(f"{who}: mask must be a bool tensor, got {getattr(mask, 'dtype', type(mask))}")
    if mask.dim() != 1:
        if mask.dim() == 0 or mask.numel() != max(mask.shape):
            raise ValueError(f"{who}: mask must be (n,) or (n, 1), got {tuple(mask.shape)}")
        mask = mask.reshape(-1)
    return mask


def _level(who, level, n_rows):
    f32(who, "level", level)
    if level.dim() != 1 or not level.is_contiguous() or level.shape[0] < max(n_rows, 1):
        raise ValueError(f"{who}: level must be a contiguous float32 (P0,) tensor with P0 >= {max(n_rows, 1)} rows, got {tuple(level.shape)}")
    return level


def _checked(who, level, segment_times, mask, tensor_lists):
    """Every check that needs neither the library nor a device read.  Returns (mask, n_rows, device)."""
    mask = _row_mask(who, mask)
    n_rows = int(mask.shape[0])
    if n_rows < 1:
        raise ValueError(f"{who}: mask has no entry")
    named = [("mask", mask)]
    for m, (lvl, tensors) in enumerate(zip(level, tensor_lists)):
        tensors = list(tensors)
        if not 1 <= len(tensors) <= MAX_TENSORS:
            raise ValueError(f"{who}: {len(tensors)} tensors, need 1 to {MAX_TENSORS}")
        named.append((f"level[{m}]" if len(level) > 1 else "level", _level(who, lvl, n_rows)))
        for k, t in enumerate(tensors):
            name = f"tensors[{k}]"
            f32(who, name, t)
            if t.dim() < 1 or t.shape[0] != n_rows:
                raise ValueError(f"{who}: {name} has {t.shape[0] if t.dim() else 0} rows, mask has {n_rows} entries")
            if not t.is_contiguous():
                raise ValueError(f"{who}: {name} must be contiguous")
            if t.numel() // n_rows > MAX_COLS:
                raise ValueError(f"{who}: {name} has {t.numel() // n_rows} values per row, at most {MAX_COLS}")
            named.append((name, t.detach()))     # a cut has no backward: the outputs are new leaves
    times = int(segment_times)
    if times < 0:
        raise ValueError(f"{who}: segment_times is negative")
    dev = no_grad_one_gpu(who, named, "mask")
    return mask.contiguous(), n_rows, dev


class _Plan:
    """plan and counts of one cut: the workspace that carries the row flags to apply, and the three counts."""

    def __init__(self, who, level, segment_times, mask, n_rows, dev):
        L = _lib.load()
        self.P0, self.n_rows, self.dev = int(level.shape[0]), n_rows, dev
        with torch.cuda.device(dev):
            stream = stream_ptr(dev)
            self.ws = torch.empty((L.mi_edit_workspace_bytes(self.P0),), device=dev, dtype=torch.uint8)
            check(L.mi_edit_plan(self.P0, level.data_ptr(), int(segment_times), n_rows, mask.data_ptr(), self.ws.data_ptr(), self.ws.numel(), stream))
            self.counts = (C.c_int * len(COUNTS))()
            check(L.mi_edit_counts(self.P0, self.ws.data_ptr(), self.ws.numel(), self.counts, stream))
        self.current, self.selected, self.kept = (int(c) for c in self.counts)
        if self.current != n_rows:
            raise ValueError(f"{who}: level and segment_times describe {self.current} current rows, the mask and the tensors have {n_rows}; "
                             "nothing was modified")
        self.inverted = self.selected == 0

    def apply(self, level, tensors):
        """New tensors of `kept` rows; level (None: left alone) gets + 1 in every kept original row."""
        L = _lib.load()
        dev, kept = self.dev, self.kept
        src = [t.detach() for t in tensors]
        dst = [torch.empty((kept,) + tuple(t.shape[1:]), device=dev, dtype=torch.float32) for t in src]
        cols = [t.numel() // self.n_rows for t in src]
        n = len(src)
        with torch.cuda.device(dev):
            check(L.mi_edit_apply(self.P0, self.n_rows, self.counts, None if level is None else level.data_ptr(), n,
                                  _ptr_table([t.data_ptr() if c else None for t, c in zip(src, cols)]),
                                  _ptr_table([t.data_ptr() if c else None for t, c in zip(dst, cols)]), (C.c_int * n)(*cols),
                                  self.ws.data_ptr(), self.ws.numel(), stream_ptr(dev)))
        return [torch.nn.Parameter(d, requires_grad=t.requires_grad) if isinstance(t, torch.nn.Parameter) else d for t, d in zip(tensors, dst)]


def cut_rows(level, segment_times, mask, tensors):
    """Keeps the rows of `tensors` that `mask` selects (all of them when it selects none) and adds one to `level` of every kept
    original row, in place.  level: float32 (P0,), the cuts every original row has survived plus one; the tensors' rows must be the
    original rows with level == segment_times + 1, in order.  mask: bool (n_rows,) or (n_rows, 1).  tensors: 1 to 32 contiguous
    float32 GPU tensors of n_rows rows each, any trailing shape (none is fine: (n_rows, 0, 3) comes back as (kept, 0, 3)).

    Returns (new_tensors, kept, inverted): new tensors of `kept` rows, an nn.Parameter for an nn.Parameter with its requires_grad;
    inverted says that the mask selected nothing and every row was kept.  Raises ValueError, with nothing modified, when level and
    segment_times describe another number of current rows than the tensors have.  One host read (the counts)."""
    who = "cut_rows"
    tensors = list(tensors)
    mask, n_rows, dev = _checked(who, [level], segment_times, mask, [tensors])
    plan = _Plan(who, level, segment_times, mask, n_rows, dev)
    return plan.apply(level, tensors), plan.kept, plan.inverted


def roll_back_level(level, segment_times) -> None:
    """In place: level - 1 in the rows with level == segment_times + 1 (the reference's roll_back).  One expression, no host read."""
    level.sub_((level == int(segment_times) + 1).to(level.dtype))


class SegmentStack:
    """The state of successive cuts of tensors that share their rows, for callers without the reference's classes.

        stack = SegmentStack(P0, device)
        tensors, kept, inverted = stack.cut(mask, tensors)      # the tensors given are kept for roll_back, by reference
        tensors = stack.roll_back()                             # None on an empty stack
        tensors = stack.clear()                                 # the tensors of before the first cut; None on an empty stack
        stack.current_mask()                                    # bool (P0,): what the GUI saves

    level is float32 (P0,), times the number of cuts in force, as the reference's _mask and segment_times."""

    def __init__(self, P0, device="cuda"):
        if int(P0) < 1:
            raise ValueError(f"SegmentStack: need P0 >= 1, got {P0}")
        self.level = torch.ones((int(P0),), dtype=torch.float32, device=device)
        self.times = 0
        self._old = []

    @property
    def depth(self) -> int:
        return len(self._old)

    def cut(self, mask, tensors):
        tensors = list(tensors)
        new, kept, inverted = cut_rows(self.level, self.times, mask, tensors)
        self._old.append(tensors)
        self.times += 1
        return new, kept, inverted

    def roll_back(self):
        if not self._old:
            return None
        tensors = self._old.pop()
        roll_back_level(self.level, self.times)
        self.times -= 1
        return tensors

    def clear(self):
        if not self._old:
            return None
        tensors = self._old[0]
        self._old = []
        self.times = 0
        self.level = torch.ones_like(self.level)
        return tensors

    def current_mask(self):
        return self.level == self.times + 1


# ---- the reference's GaussianModel and FeatureGaussianModel, bound by install_model_edit() ----------------------------------------

# attribute -> the list its earlier values are pushed on; the class with _point_features is the feature model
_EDIT_FIELDS = {
    "scene": {"_xyz": "old_xyz", "_features_dc": "old_features_dc", "_features_rest": "old_features_rest", "_opacity": "old_opacity",
              "_scaling": "old_scaling", "_rotation": "old_rotation"},
    "feature": {"_xyz": "old_xyz", "_point_features": "old_point_features", "_opacity": "old_opacity", "_scaling": "old_scaling",
                "_rotation": "old_rotation"},
}


def _fields(model):
    return _EDIT_FIELDS["feature" if hasattr(model, "_point_features") else "scene"]


def segment_models(models, mask):
    """segment(mask) of several models in the same state -- the same number of original and of current rows and the same
    segment_times, as the GUI's scene and feature pair is -- with ONE plan and ONE host read; the row map and the gather run once
    per model.  The plan is made from the first model's _mask: that the others' hold the same values is the caller's contract (it
    is not read back).  Each model is left as its own segment(mask) leaves it; returns (kept, inverted)."""
    who = "segment_models"
    models = list(models)
    if not models:
        raise ValueError(f"{who}: no model")
    for m in models:
        if getattr(m, "optimizer", None) is not None:
            raise ValueError(f"{who}: a model has an optimizer; set it to None (the cut does not prune optimizer state)")
        if int(m.segment_times) != int(models[0].segment_times) or m._mask.shape != models[0]._mask.shape:
            raise ValueError(f"{who}: the models are not in the same state (segment_times, original rows)")
    tensor_lists = [[getattr(m, field) for field in _fields(m)] for m in models]
    mask, n_rows, dev = _checked(who, [m._mask for m in models], models[0].segment_times, mask, tensor_lists)
    plan = _Plan(who, models[0]._mask, models[0].segment_times, mask, n_rows, dev)
    if plan.inverted:
        print(EMPTY_MASK_MESSAGE)
    raised = set()
    for m, tensors in zip(models, tensor_lists):
        shared = m._mask.data_ptr() in raised      # two models with ONE _mask tensor: its rows go up once
        new = plan.apply(None if shared else m._mask, tensors)
        raised.add(m._mask.data_ptr())
        if hasattr(m, "old_mask"):      # the scene model keeps its _mask tensors too (the same object every time)
            m.old_mask.append(m._mask)
        for (field, old), t_old, t_new in zip(_fields(m).items(), tensors, new):
            getattr(m, old).append(t_old)
            setattr(m, field, t_new)
        m.segment_times += 1
    return plan.kept, plan.inverted


def fused_segment(self, mask=None):
    assert mask is not None
    if self.optimizer is not None:
        # the reference's GaussianModel prunes its optimizer here and its FeatureGaussianModel refuses: neither is this module's
        # business (no caller does it), so it is the reference's own method that runs
        ref = getattr(type(self), "_reference_segment", None)
        if ref is None:
            raise ValueError("fused segment: the model has an optimizer; set it to None")
        return ref(self, mask)
    segment_models([self], mask)


def fused_roll_back(self):
    fields = _fields(self)
    if not all(getattr(self, old) for old in fields.values()):      # an empty stack: nothing changes
        return
    for field, old in fields.items():
        setattr(self, field, getattr(self, old).pop())
    roll_back_level(self._mask, self.segment_times)
    self.segment_times -= 1


def fused_clear_segment(self):
    fields = _fields(self)
    if not all(getattr(self, old) for old in fields.values()):
        return
    for field, old in fields.items():
        setattr(self, field, getattr(self, old)[0])
        setattr(self, old, [])
    if hasattr(self, "old_mask"):
        self.old_mask = []
    self.segment_times = 0
    self._mask = torch.ones((self._xyz.shape[0],), dtype=torch.float, device=self._xyz.device)
