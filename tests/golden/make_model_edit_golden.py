"""Writes tests/golden/model_edit/model_edit.npz: what the reference's own segment / roll_back / clear_segment
(scene/gaussian_model.py:376-472, scene/gaussian_model_ff.py:257-320) leave after every operation of seeded sequences, for
tests/test_model_edit_host.py (the restatement) and tests/test_model_edit.py (the kernels).

Run where the reference sources are (tests/reference_helpers.py: REF_ROOT); not part of the tests:

    python tests/golden/make_model_edit_golden.py [--reference <checkout>]

The two modules import the rasterizer, simple_knn and plyfile at their top, so only the three methods of each class are taken: the
file is parsed, the method definitions are compiled at run time in a namespace that holds torch, and nothing of their text is kept.
They run on CPU tensors; clear_segment's torch.ones(..., device="cuda") is redirected to the CPU for the call.

Per case: P0 in {1, 37, 257, 1000} original rows and 6 to 10 operations: cuts with random masks of several densities, an all-false
mask (everything is kept), an all-true mask, an (n, 1) mask, roll backs (more of them than cuts, too), clear (on an empty stack,
too), a cut after a roll back.  Every tensor's first column carries the original row number.  Stored after every operation: the
surviving row numbers, _mask, segment_times and the depth of the old_* lists.  Asserted here: no operation of any case raises, in
either class; both classes, and every tensor of each, hold the same rows; tests/model_edit_ref.py agrees after every operation.

One thing the reference does not do: a mask of ONE entry is squeezed to zero dimensions, on which FeatureGaussianModel.segment's
own `mask.shape[0]` raises IndexError (GaussianModel.segment has that line commented out and goes on, with tensors that gain a
leading axis).  So the feature class runs every case except P0 = 1, where exactly that IndexError is asserted, and no sequence with
P0 > 1 is drawn that would cut down to a single row."""
import argparse
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import model_edit_ref as mr  # noqa: E402
from tests import reference_helpers as rh  # noqa: E402

SIZES = [1, 37, 257, 1000]
CASES_PER_SIZE = 4
METHODS = ("segment", "roll_back", "clear_segment")


def reference_methods(reference_root, module, class_name):
    path = os.path.join(reference_root, "scene", module + ".py")
    tree = ast.parse(open(path).read(), path)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == class_name)
    fns = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in METHODS]
    assert sorted(f.name for f in fns) == sorted(METHODS), [f.name for f in fns]
    ns = {"torch": torch}
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)
    return {name: ns[name] for name in METHODS}


class Model:
    """The attributes the three methods work on, and nothing else of the reference's classes."""

    def __init__(self, kind, methods, P0, seed):
        self.kind, self.methods, self.P0 = kind, methods, P0
        self.layout = mr.LAYOUTS[kind](3) if kind == "scene" else mr.LAYOUTS[kind](8)
        self.optimizer = None
        self.segment_times = 0
        for field in list(self.layout) + (["_mask"] if kind == "scene" else []):
            setattr(self, "old" + field, [])
        mr.fill_model(self, self.layout, P0, seed, "cpu", parameters=False)

    def run(self, op, mask):
        ones = torch.ones
        torch.ones = lambda *a, **k: ones(*a, **{key: v for key, v in k.items() if key != "device"})
        try:
            if op == mr.CUT:
                self.methods["segment"](self, mask.clone())
            else:
                self.methods["roll_back" if op == mr.ROLL_BACK else "clear_segment"](self)
        finally:
            torch.ones = ones

    def rows(self):
        """The rows every tensor holds (all must agree); a one-entry mask leaves the scene class's tensors with extra leading axes."""
        out = None
        for field, trailing in self.layout.items():
            cols = int(np.prod(trailing))
            ids = getattr(self, field).reshape(-1, cols)[:, 0].to(torch.int64)
            assert out is None or torch.equal(out, ids), field
            out = ids
        return out

    def depth(self):
        depths = {len(getattr(self, "old" + field)) for field in self.layout}
        assert len(depths) == 1
        return depths.pop()


def draw_ops(rng, P0):
    """[(op, mask or None)] of 6 to 10 operations; masks are drawn against a CutState so that their lengths fit."""
    state = mr.CutState(P0)
    n_ops = int(rng.integers(6, 11))
    kinds = ["random", "none", "all", "column", "random", "roll", "cut_after_roll", "roll", "roll", "roll", "clear", "clear", "random", "roll"]
    order = [kinds[k] for k in rng.permutation(len(kinds))][:n_ops]
    if rng.random() < 0.5:
        order[0] = rng.choice(["clear", "roll"])      # on an empty stack
    ops = []
    for kind in order:
        n = len(state.rows)
        if kind in ("roll", "clear"):
            op, mask = (mr.ROLL_BACK if kind == "roll" else mr.CLEAR), None
        else:
            op = mr.CUT
            if kind == "cut_after_roll" and state.earlier:
                state.apply(mr.ROLL_BACK)
                ops.append((mr.ROLL_BACK, None))
                n = len(state.rows)
            if kind == "none":
                mask = np.zeros(n, bool)
            elif kind == "all":
                mask = np.ones(n, bool)
            else:
                density = float(rng.choice([0.1, 0.3, 0.6, 0.9]))
                mask = rng.random(n) < density
                while P0 > 1 and 0 < mask.sum() < 2:      # never down to one row (see the module's text); nothing selected is fine
                    mask = rng.random(n) < max(density, 0.5)
            mask = torch.from_numpy(mask)
            if kind == "column":
                mask = mask.reshape(n, 1)
        state.apply(op, mask)
        ops.append((op, mask))
    return ops[:10] if len(ops) >= 6 else ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=rh.REF_ROOT)
    ap.add_argument("--out", default=mr.GOLDEN)
    args = ap.parse_args()
    methods = {"scene": reference_methods(args.reference, "gaussian_model", "GaussianModel"),
               "feature": reference_methods(args.reference, "gaussian_model_ff", "FeatureGaussianModel")}
    rng = np.random.default_rng(20261)
    data = {k: [] for k in ("case_P0", "case_ops", "op", "mask_column", "mask_len", "mask_bits", "n_rows", "rows", "level", "times", "depth")}
    seen = {"none": 0, "all": 0, "column": 0, "roll_empty": 0, "clear_empty": 0, "clear": 0, "cut_after_roll": 0, "levels_1245": 0}
    for P0 in SIZES:
        for c in range(CASES_PER_SIZE):
            ops = draw_ops(rng, P0)
            assert 6 <= len(ops) <= 10 or P0 == 1, len(ops)
            models = [Model("scene", methods["scene"], P0, c)] + ([Model("feature", methods["feature"], P0, c)] if P0 > 1 else [])
            restated = mr.CutState(P0)
            if P0 == 1:      # the one place where a reference class raises: its own assert line, on a zero-dimensional mask
                lone = Model("feature", methods["feature"], 1, c)
                try:
                    lone.run(mr.CUT, torch.ones(1, dtype=torch.bool))
                    raise AssertionError("FeatureGaussianModel.segment took a one-entry mask")
                except IndexError:
                    pass
            previous = None
            for op, mask in ops:
                depth_before = models[0].depth()
                for m in models:
                    m.run(op, mask)      # nothing is caught here: a case in which the reference raises stops the generator
                restated.apply(op, mask)
                rows = models[0].rows()
                for m in models:
                    assert torch.equal(m.rows(), rows) and torch.equal(m._mask, models[0]._mask) and m.segment_times == models[0].segment_times
                    assert m.depth() == models[0].depth()
                assert torch.equal(rows, restated.rows) and torch.equal(models[0]._mask, restated.level)
                assert models[0].segment_times == restated.times and models[0].depth() == len(restated.earlier)
                assert torch.equal(torch.nonzero(models[0]._mask == models[0].segment_times + 1).reshape(-1), rows)
                if op == mr.CUT:
                    seen["none"] += int(not mask.any())
                    seen["all"] += int(bool(mask.all()))
                    seen["column"] += int(mask.dim() == 2)
                    seen["cut_after_roll"] += int(previous == mr.ROLL_BACK)
                else:
                    seen["roll_empty" if op == mr.ROLL_BACK else "clear_empty"] += int(depth_before == 0)
                    seen["clear"] += int(op == mr.CLEAR and depth_before > 0)
                levels = set(models[0]._mask.tolist())
                seen["levels_1245"] += int(len(levels) >= 3 and any(l + 1 not in levels and l + 2 in levels for l in levels))
                previous = op
                data["op"].append(op)
                data["mask_column"].append(int(mask is not None and mask.dim() == 2))
                data["mask_len"].append(0 if mask is None else mask.numel())
                if mask is not None:
                    data["mask_bits"].append(mask.reshape(-1).numpy())
                data["n_rows"].append(len(rows))
                data["rows"].append(rows.numpy())
                data["level"].append(models[0]._mask.numpy().copy())      # a copy: the methods go on writing into this tensor
                data["times"].append(models[0].segment_times)
                data["depth"].append(models[0].depth())
            data["case_P0"].append(P0)
            data["case_ops"].append(len(ops))
    print("cases", len(data["case_P0"]), "operations", len(data["op"]), seen)
    assert all(v >= 1 for v in seen.values()), seen
    level = np.concatenate(data["level"])
    assert level.max() < 127 and np.array_equal(level, level.astype(np.int8))
    out = dict(case_P0=np.asarray(data["case_P0"], np.int32), case_ops=np.asarray(data["case_ops"], np.int32), op=np.asarray(data["op"], np.int8),
               mask_column=np.asarray(data["mask_column"], np.int8), mask_len=np.asarray(data["mask_len"], np.int32),
               mask_bits=np.packbits(np.concatenate(data["mask_bits"])), n_rows=np.asarray(data["n_rows"], np.int32),
               rows=np.concatenate(data["rows"]).astype(np.int16), level=level.astype(np.int8), times=np.asarray(data["times"], np.int32),
               depth=np.asarray(data["depth"], np.int32))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **out)
    back = mr.load_cases(args.out)
    assert len(back) == len(data["case_P0"]) and sum(len(c["ops"]) for c in back) == len(data["op"])
    for case in back:      # what was written is what the restatement gives (which agreed with the reference above)
        state = mr.CutState(case["P0"])
        for op in case["ops"]:
            state.apply(op["op"], op["mask"])
            assert torch.equal(state.rows, op["rows"]) and torch.equal(state.level, op["level"]) and state.times == op["times"]
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
