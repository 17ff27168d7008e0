"""CPU checks of the model cut (seganygaussians_amd/model_edit.py): the restatement of tests/model_edit_ref.py
against the fixture written from the reference's own methods, the argument checks before the library is loaded, the refusals of
the C entry points before any HIP call, where the ABI lives, and the opt-in patch of install_model_edit.  No GPU."""
import ctypes as C
import importlib
import os
import re
import sys

import pytest
import torch

import seganygaussians_amd
from seganygaussians_amd import _lib, build
from seganygaussians_amd import model_edit as me
from tests import model_edit_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = ("scene", "scene.gaussian_model", "scene.gaussian_model_ff")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def test_fixture_holds_what_the_issue_lists():
    cases = mr.load_cases()
    assert sorted({c["P0"] for c in cases}) == [1, 37, 257, 1000] and all(6 <= len(c["ops"]) <= 10 for c in cases)
    ops = [op for c in cases for op in c["ops"]]
    cuts = [op for op in ops if op["op"] == mr.CUT]
    assert any(not op["mask"].any() for op in cuts) and any(op["mask"].all() and op["mask"].numel() > 1 for op in cuts)
    assert any(op["mask"].dim() == 2 and op["mask"].shape[1] == 1 for op in cuts)
    assert any(0 < int(op["mask"].sum()) < op["mask"].numel() for op in cuts)
    assert {mr.CUT, mr.ROLL_BACK, mr.CLEAR} == {op["op"] for op in ops}
    assert os.path.getsize(mr.GOLDEN) < 100_000


def test_restatement_agrees_with_the_reference_after_every_operation():
    for case in mr.load_cases():
        state = mr.CutState(case["P0"])
        for k, op in enumerate(case["ops"]):
            state.apply(op["op"], op["mask"])
            where = (case["P0"], k)
            assert torch.equal(state.rows, op["rows"]), where
            assert torch.equal(state.level, op["level"]), where
            assert (state.times, len(state.earlier)) == (op["times"], op["depth"]), where
            # the rows a model holds are the original rows with _mask == segment_times + 1, in order: what the GUI saves
            assert torch.equal(torch.nonzero(state.level == state.times + 1).reshape(-1), op["rows"]), where


def test_tagged_tensors_carry_their_rows_and_every_special_pattern():
    t = mr.tagged_tensor(1000, (15, 3), 3)
    assert t.shape == (1000, 15, 3) and torch.equal(mr.row_ids(t), torch.arange(1000))
    bits = set(t.view(torch.int32).reshape(-1).tolist())
    assert all((b - (1 << 32) if b >= 1 << 31 else b) in bits for b in mr.SPECIAL_BITS)
    assert mr.tagged_tensor(5, (0, 3), 1).shape == (5, 0, 3) and mr.bits_equal(t, t.clone())
    assert not mr.bits_equal(torch.zeros(2), -torch.zeros(2))


def test_python_arguments_refused_before_the_library_is_loaded(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    level, t = torch.ones(6), torch.zeros(6, 3)
    mask = torch.ones(6, dtype=torch.bool)
    with pytest.raises(ValueError, match="cut_rows: mask must be a bool tensor, got torch.uint8"):
        me.cut_rows(level, 0, mask.to(torch.uint8), [t])
    with pytest.raises(ValueError, match=r"cut_rows: tensors\[0\] has 6 rows, mask has 5 entries"):
        me.cut_rows(level, 0, mask[:5], [t])
    with pytest.raises(ValueError, match=r"cut_rows: mask must be \(n,\) or \(n, 1\)"):
        me.cut_rows(level, 0, mask.reshape(2, 3), [t])
    with pytest.raises(ValueError, match=r"cut_rows: mask must be on a GPU, got cpu \(there is no CPU fallback\)"):
        me.cut_rows(level, 0, mask, [t])
    with pytest.raises(ValueError, match="cut_rows: 33 tensors, need 1 to 32"):
        me.cut_rows(level, 0, mask, [t] * 33)
    with pytest.raises(ValueError, match="cut_rows: 0 tensors, need 1 to 32"):
        me.cut_rows(level, 0, mask, [])
    with pytest.raises(ValueError, match=r"cut_rows: tensors\[1\] must be a float32 tensor, got torch.float64"):
        me.cut_rows(level, 0, mask, [t, t.double()])
    with pytest.raises(ValueError, match=r"cut_rows: tensors\[0\] must be contiguous"):
        me.cut_rows(level, 0, mask, [torch.zeros(3, 6).t()])
    with pytest.raises(ValueError, match="cut_rows: level must be a float32 tensor"):
        me.cut_rows(level.double(), 0, mask, [t])
    with pytest.raises(ValueError, match=r"cut_rows: level must be a contiguous float32 \(P0,\) tensor with P0 >= 6 rows"):
        me.cut_rows(level[:4], 0, mask, [t])
    with pytest.raises(ValueError, match="cut_rows: segment_times is negative"):
        me.cut_rows(level, -1, mask, [t])
    stack = me.SegmentStack(6, "cpu")
    with pytest.raises(ValueError, match="cut_rows: mask must be on a GPU"):
        stack.cut(mask, [t])
    assert stack.times == 0 and stack.depth == 0 and stack.roll_back() is None and stack.clear() is None
    assert stack.current_mask().all() and stack.current_mask().dtype == torch.bool
    with pytest.raises(ValueError, match="P0 >= 1"):
        me.SegmentStack(0)


def test_entry_points_refuse_before_any_hip_call(lib):
    wsb = lib.mi_edit_workspace_bytes
    assert wsb(0) == 0 and wsb(-5) == 0 and wsb(1 << 30) == 0
    assert wsb(1) > 0 and 5 * 1000 <= wsb(1000) < 5 * 1000 + 8 * 256 and wsb(1 << 20) < 6 * (1 << 20)
    need = wsb(1000)

    def refused(fn, args, msg):
        assert fn(*args.values()) != 0 and _lib.last_error() == "model edit: " + msg, _lib.last_error()

    plan = dict(P0=1000, level=1 << 20, times=0, n_rows=900, mask=2 << 20, ws=8 << 20, ws_bytes=need, stream=None)
    refused(lib.mi_edit_plan, dict(plan, P0=0), "need 1 <= P0 < 2^30 rows")
    refused(lib.mi_edit_plan, dict(plan, P0=1 << 30), "need 1 <= P0 < 2^30 rows")
    refused(lib.mi_edit_plan, dict(plan, ws=None), "null pointer")
    refused(lib.mi_edit_plan, dict(plan, ws_bytes=need - 1), "workspace smaller than mi_edit_workspace_bytes(P0)")
    refused(lib.mi_edit_plan, dict(plan, level=None), "null pointer")
    refused(lib.mi_edit_plan, dict(plan, mask=None), "null pointer")
    refused(lib.mi_edit_plan, dict(plan, times=-1), "need 0 <= segment_times < 2^24")
    refused(lib.mi_edit_plan, dict(plan, times=1 << 24), "need 0 <= segment_times < 2^24")
    refused(lib.mi_edit_plan, dict(plan, n_rows=0), "need 1 <= n_rows <= P0")
    refused(lib.mi_edit_plan, dict(plan, n_rows=1001), "need 1 <= n_rows <= P0")
    refused(lib.mi_edit_plan, dict(plan, mask=(8 << 20) + need - 1), "the workspace overlaps another tensor of the call")
    counts = (C.c_int * 3)(900, 300, 300)
    refused(lib.mi_edit_counts, dict(P0=1000, ws=8 << 20, ws_bytes=need, counts=None, stream=None), "null pointer")
    refused(lib.mi_edit_counts, dict(P0=1000, ws=8 << 20, ws_bytes=16, counts=counts, stream=None), "workspace smaller than mi_edit_workspace_bytes(P0)")
    tab = lambda vals: (C.c_void_p * len(vals))(*vals)
    src, dst, cols = tab([(32 + k) << 20 for k in range(3)]), tab([(64 + k) << 20 for k in range(3)]), (C.c_int * 3)(3, 45, 0)
    ap = dict(P0=1000, n_rows=900, counts=counts, level=1 << 20, n=3, src=src, dst=dst, cols=cols, ws=8 << 20, ws_bytes=need, stream=None)
    refused(lib.mi_edit_apply, dict(ap, counts=None), "null table")
    refused(lib.mi_edit_apply, dict(ap, n=0), "need 1 <= n_tensors <= 32")
    refused(lib.mi_edit_apply, dict(ap, n=33), "need 1 <= n_tensors <= 32")
    refused(lib.mi_edit_apply, dict(ap, n_rows=0), "need 1 <= n_rows <= P0")
    not_a_plans = "counts are not those of a plan whose current rows are the n_rows of the tensors"
    refused(lib.mi_edit_apply, dict(ap, counts=(C.c_int * 3)(899, 300, 300)), not_a_plans)      # current rows != n_rows
    refused(lib.mi_edit_apply, dict(ap, counts=(C.c_int * 3)(900, 901, 901)), not_a_plans)
    refused(lib.mi_edit_apply, dict(ap, counts=(C.c_int * 3)(900, 300, 900)), not_a_plans)      # kept is neither selected nor, with none, current
    refused(lib.mi_edit_apply, dict(ap, counts=(C.c_int * 3)(900, 0, 0)), not_a_plans)
    refused(lib.mi_edit_apply, dict(ap, cols=(C.c_int * 3)(3, 4097, 0)), "need 0 <= cols <= 4096")
    refused(lib.mi_edit_apply, dict(ap, cols=(C.c_int * 3)(3, -1, 0)), "need 0 <= cols <= 4096")
    refused(lib.mi_edit_apply, dict(ap, src=tab([32 << 20, None, 34 << 20])), "null pointer")
    refused(lib.mi_edit_apply, dict(ap, dst=tab([64 << 20, 32 << 20, 66 << 20])), "an output overlaps another tensor of the call")
    refused(lib.mi_edit_apply, dict(ap, level=(64 << 20) + 8), "an output overlaps another tensor of the call")
    # a tensor without columns is skipped: its null pointers are not looked at (this one is refused later, for its overlap)
    refused(lib.mi_edit_apply, dict(ap, src=tab([32 << 20, 33 << 20, None]), dst=tab([64 << 20, 8 << 20, None])), "an output overlaps another tensor of the call")


def test_the_abi_is_a_public_header_of_its_own_and_lib_alone_binds_it(lib):
    names = ["mi_edit_workspace_bytes", "mi_edit_plan", "mi_edit_counts", "mi_edit_apply"]
    # a public header like every other: _lib binds what it declares, and the module keeps no binder of its own
    assert _lib.DECLARED["mi_model_edit.h"] == names and [n for n in _lib.ALL_EXPORTS if n.startswith("mi_edit_")] == names
    assert {n: v for n, v in _lib.CONSTANTS.items() if n.startswith("MI_EDIT_")} == {
        "MI_EDIT_MAX_TENSORS": 32, "MI_EDIT_MAX_COLS": 4096, "MI_EDIT_CURRENT": 0, "MI_EDIT_SELECTED": 1, "MI_EDIT_KEPT": 2, "MI_EDIT_NCOUNTS": 3}
    header = [h for h in build.HEADERS if os.path.basename(h) == "mi_model_edit.h"]
    assert len(header) == 1 and "mi_model_edit.h" not in build.SOURCES and not [s for s in build.SOURCES if s.startswith("mi_") and s.endswith(".h")]
    assert not [n for n in ("load", "FUNCTIONS", "HEADER", "CONSTANTS", "_bound") if hasattr(me, n)]
    # bound from the parsed header: int / size_t returns, pointers as void*, and every symbol resolves
    for name in names:
        fn, (restype, argtypes) = getattr(lib, name), _lib.SIGNATURES[name]
        assert C.cast(fn, C.c_void_p).value and fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert lib.mi_edit_workspace_bytes.restype is C.c_size_t and lib.mi_edit_plan.restype is C.c_int
    assert lib.mi_edit_apply.argtypes == [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_size_t, C.c_void_p]
    hdr = open(header[0]).read()
    assert "#define MI_EDIT_MAX_TENSORS 32\n" in hdr
    assert (me.MAX_TENSORS, me.MAX_COLS, _lib.MI_EDIT_NCOUNTS) == (32, 4096, 3) and me.COUNTS == ("current", "selected", "kept")
    assert me.COUNTS == tuple(_lib.MI_EDIT_COUNTS)      # whose order _lib checks against the enumerators when it is imported
    # a C++ compiler reads the header as the parser does (the declarations are used by mi_model_edit.hip itself: a mismatch with
    # the definitions there would not compile)
    sources = {f: open(os.path.join(build.SRC_DIR, f)).read() for f in build.SOURCES}
    assert {"model_edit.h", "mi_model_edit.hip", "row_compact.h"} <= set(sources)
    assert [f for f, text in sources.items() if 'include/mi_model_edit.h"' in text] == ["mi_model_edit.hip"]
    assert [f for f, text in sources.items() if '"model_edit.h"' in text] == ["mi_model_edit.hip"]
    assert [f for f, text in sources.items() if '"train_step.h"' in text] == ["mi_train_step.hip"]
    # the rank, the scan and the gather exist once, in the header both users include
    assert sorted(f for f, text in sources.items() if '"row_compact.h"' in text) == ["model_edit.h", "train_step.h"]
    for what in (r"\bint block_rank\(", r"\bvoid __launch_bounds__\(\w+\) block_scan_kernel\(", r"\bvoid __launch_bounds__\(\w+\) row_gather_kernel\("):
        assert [f for f, text in sources.items() if re.search(what, text)] == ["row_compact.h"], what


def _finders(module):
    return [f for f in sys.meta_path if isinstance(f, seganygaussians_amd._PatchOnImport) and f.module_name == module]


@pytest.fixture
def stand_ins(tmp_path, monkeypatch):
    mr.write_stand_ins(tmp_path)
    monkeypatch.syspath_prepend(str(tmp_path))

    def forget():
        sys.meta_path[:] = [f for f in sys.meta_path if not isinstance(f, seganygaussians_amd._PatchOnImport)]
        for k in MODULES:
            sys.modules.pop(k, None)
        importlib.invalidate_caches()
    forget()
    yield forget
    forget()


def _is_patched(cls, smoothing=None):
    from seganygaussians_amd import knn_smooth
    assert cls.segment is me.fused_segment and cls.roll_back is me.fused_roll_back and cls.clear_segment is me.fused_clear_segment
    m = cls()
    cls._reference_segment(m, None), cls._reference_roll_back(m), cls._reference_clear_segment(m)
    assert m.calls == ["reference segment", "reference roll_back", "reference clear_segment"]
    if smoothing is not None:
        assert (cls.get_smoothed_point_features is knn_smooth.fused_get_smoothed_point_features) == smoothing
        if smoothing:
            assert cls._reference_get_smoothed_point_features(m) == "reference smoothing"


def test_install_model_edit_patches_both_stand_ins(stand_ins):
    for _ in range(2):
        seganygaussians_amd.install_model_edit()           # one finder per module, however often it is asked for
        assert [len(_finders(k)) for k in MODULES[1:]] == [1, 1]
    scene = importlib.import_module("scene.gaussian_model").GaussianModel
    assert not _finders("scene.gaussian_model") and len(_finders("scene.gaussian_model_ff")) == 1
    feature = importlib.import_module("scene.gaussian_model_ff").FeatureGaussianModel
    assert not _finders("scene.gaussian_model_ff")
    for _ in range(2):                                                     # already imported: patched at once, idempotently
        seganygaussians_amd.install_model_edit()
        _is_patched(scene)
        _is_patched(feature, smoothing=False)
    seganygaussians_amd.patch_model_edit(scene)
    _is_patched(scene)
    assert {"patch_model_edit", "install_model_edit"} <= set(seganygaussians_amd.__all__)


@pytest.mark.parametrize("order", ["smoothing first", "model edit first"])
@pytest.mark.parametrize("when", ["before the import", "after the import"])
def test_fuse_smoothing_and_model_edit_both_take_effect(stand_ins, order, when):
    smoothing, edit = (lambda: seganygaussians_amd.install_dropin(fuse_smoothing=True)), seganygaussians_amd.install_model_edit
    calls = [smoothing, edit] if order == "smoothing first" else [edit, smoothing]
    if when == "after the import":
        importlib.import_module("scene.gaussian_model_ff")
    for call in calls * 2:
        call()
        assert len(_finders("scene.gaussian_model_ff")) == (1 if when == "before the import" else 0)
        assert len(_finders("scene.gaussian_model")) <= 1
    if when == "before the import":
        assert len(_finders("scene.gaussian_model_ff")[0].patches) == 2
    feature = importlib.import_module("scene.gaussian_model_ff").FeatureGaussianModel
    assert not _finders("scene.gaussian_model_ff")
    _is_patched(feature, smoothing=True)
    _is_patched(importlib.import_module("scene.gaussian_model").GaussianModel)
    assert not _finders("scene.gaussian_model")


def test_a_model_with_an_optimizer_reaches_the_reference(stand_ins):
    seganygaussians_amd.install_model_edit()
    for module, name in (("scene.gaussian_model", "GaussianModel"), ("scene.gaussian_model_ff", "FeatureGaussianModel")):
        m = getattr(importlib.import_module(module), name)()
        m.optimizer = object()
        m.segment(torch.ones(3, dtype=torch.bool))
        assert m.calls == ["reference segment"]
        with pytest.raises(AssertionError):
            m.segment(None)
        # roll back and clear on an empty stack change nothing and need no device
        m._mask = marker = torch.ones(3)
        m.roll_back(), m.clear_segment()
        assert m._mask is marker and m.segment_times == 0 and m.calls == ["reference segment"]
    with pytest.raises(ValueError, match="segment_models: a model has an optimizer"):
        me.segment_models([m], torch.ones(3, dtype=torch.bool))
