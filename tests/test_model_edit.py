"""GPU checks of the model cut (seganygaussians_amd/model_edit.py, csrc/model_edit.h, csrc/row_compact.h).

There is no tolerance in this feature: a kept row is its source row bit for bit, so everything is compared as int32 views, against
boolean indexing on the CPU and against the fixture written from the reference's own methods (tests/model_edit_ref.py)."""
import importlib
import sys

import numpy as np
import pytest
import torch

import seganygaussians_amd
from seganygaussians_amd import _lib
from seganygaussians_amd import model_edit as me
from tests import model_edit_ref as mr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SIZES = (1, 63, 64, 65, 255, 256, 257, 513, 1000, 65_795)      # 65 795 rows: 258 workgroups, so a thread of the scan has two
TRAILING = [(1,), (3,), (4,), (32,), (15, 3), (0, 3)]


def _masks(P):
    rng = np.random.default_rng(P)
    first, last = np.zeros(P, bool), np.zeros(P, bool)
    first[0], last[-1] = True, True
    hole = np.ones(P, bool)
    hole[256 * ((P // 256) // 2):256 * ((P // 256) // 2) + 256] = False      # one whole workgroup of rows unselected
    return {"all": np.ones(P, bool), "none": np.zeros(P, bool), "first": first, "last": last, "alternating": np.arange(P) % 2 == 0,
            "random 0.3": rng.random(P) < 0.3, "a workgroup out": hole}


def _check_cut(P, name, mask, host, dev, level=None, times=0):
    level = torch.ones(P, device=DEV) if level is None else level
    before = level.cpu()
    new, kept, inverted = me.cut_rows(level, times, torch.from_numpy(mask).to(DEV), dev)
    keep = torch.from_numpy(mask if mask.any() else ~mask)
    assert (kept, inverted) == (int(keep.sum()), not mask.any()), (P, name)
    for k, (t, n) in enumerate(zip(host, new)):
        assert n.device == DEV and n.is_contiguous() and mr.bits_equal(n.cpu(), t[keep]), (P, name, k)
    want = before.clone()
    want[torch.nonzero(before == times + 1).reshape(-1)[keep]] += 1
    assert torch.equal(level.cpu(), want), (P, name)
    return new


@pytest.mark.parametrize("P", SIZES)
def test_rows_are_gathered_bit_for_bit(P):
    host = [mr.tagged_tensor(P, trailing, 7 * P + k) for k, trailing in enumerate(TRAILING)]
    dev = [t.to(DEV) for t in host]
    for name, mask in _masks(P).items():
        new = _check_cut(P, name, mask, host, dev)
        assert new[-1].shape == (int(mask.sum()) or P, 0, 3)
    for t, d in zip(host, dev):
        assert mr.bits_equal(d.cpu(), t)      # the sources are not written


@pytest.mark.parametrize("P", (257, 1000))
def test_one_tensor_and_thirty_two_in_one_call(P):
    mask = _masks(P)["random 0.3"]
    shapes = [TRAILING[k % len(TRAILING)] for k in range(32)]
    host = [mr.tagged_tensor(P, s, 31 * P + k) for k, s in enumerate(shapes)]
    _check_cut(P, "32 tensors", mask, host, [t.to(DEV) for t in host])
    _check_cut(P, "1 tensor", mask, host[3:4], [host[3].to(DEV)])
    _check_cut(P, "only a tensor without columns", mask, host[5:6], [host[5].to(DEV)])


def test_a_cut_of_a_cut_reads_the_levels():
    # 1000 original rows of which 400 are current at segment_times = 2; the others are at lower levels or, a stale entry, above
    P0, rng = 1000, np.random.default_rng(5)
    lv = rng.integers(1, 3, P0).astype(np.float32)
    current = np.sort(rng.permutation(P0)[:400])
    lv[current] = 3.0
    lv[np.setdiff1d(np.arange(P0), current)[:5]] = 4.0
    for name, mask in _masks(400).items():
        host = [mr.tagged_tensor(400, (3,), 1), mr.tagged_tensor(400, (15, 3), 2)]
        level = torch.from_numpy(lv.copy()).to(DEV)
        _check_cut(400, name, mask, host, [t.to(DEV) for t in host], level=level, times=2)


def _layout_tensors(P0, seed):
    return [mr.tagged_tensor(P0, (3,), seed), mr.tagged_tensor(P0, (2, 3), seed + 1)]


def test_fixture_sequences_through_segment_stack():
    for c, case in enumerate(mr.load_cases()):
        P0 = case["P0"]
        original = _layout_tensors(P0, c)
        tensors = [t.to(DEV) for t in original]
        stack = me.SegmentStack(P0, DEV)
        for k, op in enumerate(case["ops"]):
            where = (P0, c, k)
            if op["op"] == mr.CUT:
                tensors, kept, inverted = stack.cut(op["mask"].to(DEV), tensors)
                assert kept == len(op["rows"]) and inverted == (not op["mask"].any()), where
            else:
                depth_before = stack.depth
                back = stack.roll_back() if op["op"] == mr.ROLL_BACK else stack.clear()
                assert (back is None) == (depth_before == 0), where      # on an empty stack nothing changes
                tensors = tensors if back is None else back
            assert (stack.times, stack.depth) == (op["times"], op["depth"]), where
            assert torch.equal(stack.level.cpu(), op["level"]), where
            assert torch.equal(torch.nonzero(stack.current_mask()).reshape(-1).cpu(), op["rows"]), where
            for t, o in zip(tensors, original):
                assert mr.bits_equal(t.cpu(), o[op["rows"]]), where


@pytest.fixture
def classes(tmp_path, monkeypatch):
    """The two stand-in classes, patched by install_model_edit()."""
    names = ("scene", "scene.gaussian_model", "scene.gaussian_model_ff")

    def forget():
        sys.meta_path[:] = [f for f in sys.meta_path if not isinstance(f, seganygaussians_amd._PatchOnImport)]
        for k in names:
            sys.modules.pop(k, None)
        importlib.invalidate_caches()
    forget()
    mr.write_stand_ins(tmp_path)
    monkeypatch.syspath_prepend(str(tmp_path))
    seganygaussians_amd.install_model_edit()
    yield {"scene": importlib.import_module("scene.gaussian_model").GaussianModel,
           "feature": importlib.import_module("scene.gaussian_model_ff").FeatureGaussianModel}
    forget()


def _old_lists(model, layout):
    return ["old" + field for field in layout] + (["old_mask"] if hasattr(model, "old_mask") else [])


@pytest.mark.parametrize("kind", ["scene", "feature"])
def test_fixture_sequences_through_the_patched_classes(classes, kind, capsys):
    layout = mr.LAYOUTS[kind](3) if kind == "scene" else mr.LAYOUTS[kind](8)
    for c, case in enumerate(mr.load_cases()):
        P0 = case["P0"]
        model = classes[kind]()
        original = mr.fill_model(model, layout, P0, c, DEV)
        original = {f: t.cpu() for f, t in original.items()}
        for k, op in enumerate(case["ops"]):
            where = (kind, P0, c, k)
            level_tensor, before = model._mask, {f: getattr(model, f) for f in layout}
            depth_before = len(model.old_xyz)
            capsys.readouterr()
            if op["op"] == mr.CUT:
                assert model.segment(op["mask"].to(DEV)) is None
                said = capsys.readouterr().out
                assert (said == me.EMPTY_MASK_MESSAGE + "\n") == (not op["mask"].any()) and said in ("", me.EMPTY_MASK_MESSAGE + "\n"), where
                for f in layout:      # pushed by reference, not copied; a Parameter comes back as one
                    assert getattr(model, "old" + f)[-1] is before[f] and isinstance(getattr(model, f), torch.nn.Parameter), where
                    assert getattr(model, f).requires_grad and getattr(model, f).is_leaf, where
                assert model._mask is level_tensor, where      # updated in place
            elif op["op"] == mr.ROLL_BACK:
                model.roll_back()
                assert model._mask is level_tensor, where
            else:
                model.clear_segment()
                assert (model._mask is level_tensor) == (depth_before == 0), where      # a NEW tensor of ones, unless the stack was empty
            assert model.segment_times == op["times"] and model.calls == [], where
            assert {len(getattr(model, o)) for o in _old_lists(model, layout) if o != "old_mask"} == {op["depth"]}, where
            assert torch.equal(model._mask.cpu(), op["level"]) and model._mask.dtype == torch.float32 and model._mask.device == DEV, where
            for f in layout:
                assert mr.bits_equal(getattr(model, f).detach().cpu(), original[f][op["rows"]]), where + (f,)
        if kind == "scene":      # the reference's roll_back leaves old_mask alone: one entry per cut since the last clear
            assert all(m is model._mask for m in model.old_mask)


def test_segment_models_is_two_cuts_with_one_host_read(classes, monkeypatch):
    P0 = 1000
    L = _lib.load()
    calls = {"counts": 0, "plan": 0, "apply": 0}
    for name in calls:
        def wrapped(*args, _name=name, _fn=getattr(L, "mi_edit_" + name)):
            calls[_name] += 1
            return _fn(*args)
        monkeypatch.setattr(L, "mi_edit_" + name, wrapped)
    layouts = {"scene": mr.LAYOUTS["scene"](15), "feature": mr.LAYOUTS["feature"](32)}
    masks = [torch.from_numpy(np.random.default_rng(1).random(P0) < 0.4), None, torch.zeros(1, dtype=torch.bool)]

    def pair():
        models = {k: classes[k]() for k in layouts}
        for k, m in models.items():
            mr.fill_model(m, layouts[k], P0, 3, DEV)
        return models
    together, apart = pair(), pair()
    for step, mask in enumerate(masks):
        n = together["scene"]._xyz.shape[0]
        mask = (torch.from_numpy(np.random.default_rng(2).random(n) < 0.5) if mask is None else mask.expand(n).contiguous()).to(DEV)
        calls.update(counts=0, plan=0, apply=0)
        kept, inverted = me.segment_models([together["scene"], together["feature"]], mask)
        assert calls == {"counts": 1, "plan": 1, "apply": 2}, step
        assert inverted == (not mask.any()) and kept == (int(mask.sum()) or n)
        for k in layouts:
            apart[k].segment(mask)
            assert together[k].segment_times == apart[k].segment_times == step + 1
            assert torch.equal(together[k]._mask, apart[k]._mask)
            for f in layouts[k]:
                assert mr.bits_equal(getattr(together[k], f).detach().cpu(), getattr(apart[k], f).detach().cpu()), (step, k, f)
                assert len(getattr(together[k], "old" + f)) == step + 1
    with pytest.raises(ValueError, match="not in the same state"):
        apart["scene"].roll_back()
        me.segment_models([together["scene"], apart["scene"]], torch.ones(together["scene"]._xyz.shape[0], dtype=torch.bool, device=DEV))


def test_a_model_in_another_state_is_refused_and_left_alone(classes):
    # 10 original rows, all current, but tensors of 7 rows: the reference fails with an index error here
    host = [mr.tagged_tensor(7, (3,), 1), mr.tagged_tensor(7, (4,), 2)]
    dev = [t.to(DEV) for t in host]
    level = torch.ones(10, device=DEV)
    mask = torch.tensor([True, False] * 3 + [True], device=DEV)
    with pytest.raises(ValueError, match="cut_rows: level and segment_times describe 10 current rows, the mask and the tensors have 7; nothing was modified"):
        me.cut_rows(level, 0, mask, dev)
    assert torch.equal(level.cpu(), torch.ones(10)) and all(mr.bits_equal(d.cpu(), t) for d, t in zip(dev, host))
    stack = me.SegmentStack(10, DEV)
    with pytest.raises(ValueError, match="10 current rows"):
        stack.cut(mask, dev)
    assert (stack.times, stack.depth) == (0, 0) and bool(stack.current_mask().all())
    model = classes["feature"]()
    layout = mr.LAYOUTS["feature"](8)
    mr.fill_model(model, layout, 7, 0, DEV)
    model._mask = torch.ones(10, device=DEV)
    before = {f: getattr(model, f) for f in layout}
    with pytest.raises(ValueError, match="segment_models: level and segment_times describe 10 current rows"):
        model.segment(mask)
    assert model.segment_times == 0 and torch.equal(model._mask.cpu(), torch.ones(10))
    assert all(getattr(model, f) is before[f] and getattr(model, "old" + f) == [] for f in layout)


def test_another_stream_and_a_second_run_give_the_same_bits():
    P = 65_795
    host = [mr.tagged_tensor(P, (3,), 1), mr.tagged_tensor(P, (15, 3), 2)]
    dev = [t.to(DEV) for t in host]
    mask = torch.from_numpy(_masks(P)["random 0.3"]).to(DEV)
    runs = []
    torch.cuda.synchronize()
    for stream in (None, torch.cuda.Stream(DEV), None):
        level = torch.ones(P, device=DEV)
        torch.cuda.synchronize()
        if stream is None:
            new, kept, _ = me.cut_rows(level, 0, mask, dev)
        else:
            with torch.cuda.stream(stream):
                new, kept, _ = me.cut_rows(level, 0, mask, dev)
            stream.synchronize()
        torch.cuda.synchronize()
        runs.append([n.cpu() for n in new] + [level.cpu()])
    keep = mask.cpu()
    assert all(mr.bits_equal(a, t[keep]) for a, t in zip(runs[0], host))
    for other in runs[1:]:
        assert all(mr.bits_equal(a, b) for a, b in zip(runs[0], other))


def test_parameters_come_back_as_parameters():
    P = 300
    mask = torch.from_numpy(_masks(P)["alternating"]).to(DEV)
    p_grad = torch.nn.Parameter(mr.tagged_tensor(P, (3,), 1, DEV), requires_grad=True)
    p_fixed = torch.nn.Parameter(mr.tagged_tensor(P, (4,), 2, DEV), requires_grad=False)
    plain = mr.tagged_tensor(P, (1,), 3, DEV)
    stack = me.SegmentStack(P, DEV)
    given = [p_grad, p_fixed, plain]
    new, kept, inverted = stack.cut(mask, given)      # grad mode is on: a cut has no backward, its results are new leaves
    assert kept == 150 and not inverted
    assert isinstance(new[0], torch.nn.Parameter) and new[0].requires_grad and new[0].is_leaf
    assert isinstance(new[1], torch.nn.Parameter) and not new[1].requires_grad
    assert not isinstance(new[2], torch.nn.Parameter) and not new[2].requires_grad
    back = stack.roll_back()
    assert all(b is g for b, g in zip(back, given)) and len(back) == 3      # the very objects, no copy
    assert bool(stack.current_mask().all()) and stack.times == 0
