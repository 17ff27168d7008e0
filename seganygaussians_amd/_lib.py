"""ctypes binding of the C-ABI library, read off its headers (include/*.h): what they declare is what is bound, and every MI_*
constant they define is an attribute of this module.  Fails loudly when the HIP extension is missing: there is NO CPU / PyTorch
fallback in the product path."""
from __future__ import annotations

import ctypes as C
import os
import re

from .build import HEADERS, LIB_PATH

RESIZE_FN = C.CFUNCTYPE(C.c_void_p, C.c_size_t, C.c_void_p)


class MiRastError(RuntimeError):
    pass


# ---- the grammar the headers keep; anything else is refused, never guessed ----
_SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "uint32_t": C.c_uint32}
_RETURNS = dict(_SCALARS, **{"void": None, "const char*": C.c_char_p})
_RESIZE_TYPEDEF = "typedef char* (*mi_rast_resize_fn)(size_t nbytes, void* user)"
_DIRECTIVES = re.compile(r"#\s*(include\b|ifndef\b|ifdef\s+__cplusplus$|endif$)")
_INT = r"(0|[1-9][0-9]*|0[xX][0-9a-fA-F]+)"


def _integer(text):
    """The value of a decimal or hex literal or of `(a << b)`; None for anything else."""
    m = re.fullmatch(rf"{_INT}|\(\s*{_INT}\s*<<\s*{_INT}\s*\)", text)
    return None if not m else int(m.group(1), 0) if m.group(1) else int(m.group(2), 0) << int(m.group(3), 0)


def _ctype(text):
    return re.sub(r"\s*\*\s*", "*", " ".join(text.split()))


def parse_header(text: str, header: str = "<header>"):
    """One header's text -> ([(function, restype, [argtypes])] in declaration order, {MI_* constant: value})."""
    def refuse(why, decl):
        raise MiRastError(f"{header}: {why}: {' '.join(decl.split())!r}")

    functions, constants, code, in_cplusplus = [], {}, [], False
    for line in re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S).split("\n"):
        line = line.strip()
        if not line.startswith("#"):
            if not in_cplusplus:     # an `#ifdef __cplusplus` block holds extern "C" { or its }
                code.append(line)
            continue
        m = re.fullmatch(r"#\s*define\s+(\w+)\s*(.*)", line)
        if m and m.group(2) and m.group(1).startswith("MI_"):     # a define without a value is an include guard
            value = _integer(m.group(2))
            if value is None or m.group(1) in constants:
                refuse("a define whose value is not an integer, or defined twice", line)
            constants[m.group(1)] = value
        elif not m and not _DIRECTIVES.match(line):
            refuse("an unknown directive", line)
        in_cplusplus = line.endswith("__cplusplus") or in_cplusplus and not line.endswith("endif")     # from its #ifdef to the next #endif
    for decl in " ".join(code).split(";"):
        decl = decl.strip()
        if not decl or " ".join(decl.split()) == _RESIZE_TYPEDEF:
            continue
        m = re.fullmatch(r"enum\s*\{([^{}]*)\}", decl)
        if m:
            value = -1
            for item in m.group(1).split(","):
                e = re.fullmatch(r"\s*(MI_\w+)\s*(?:=\s*(\S+)\s*)?", item)
                if e:
                    value = value + 1 if e.group(2) is None else _integer(e.group(2))
                if not e or value is None or e.group(1) in constants:
                    refuse("an enumerator that is not `MI_NAME` or `MI_NAME = integer`, or defined twice", decl)
                constants[e.group(1)] = value
            continue
        m = re.fullmatch(r"([\w\s*]+?)\b(\w+)\s*\(([^()]*)\)", decl)
        if not m or _ctype(m.group(1)) not in _RETURNS:
            refuse("not `ret name(params)` with a known return type, an anonymous enum or the resize callback's typedef", decl)
        argtypes = []
        for param in [] if m.group(3).strip() == "void" else m.group(3).split(","):
            p = re.fullmatch(r"\s*([\w\s*]+?)\b(\w+)\s*", param)
            if not p:
                refuse(f"parameter {param.strip()!r} is not `type name`", decl)
            t = _ctype(p.group(1))
            if "*" not in t and t != "mi_rast_resize_fn" and t not in _SCALARS:
                refuse(f"unknown type {t!r} of parameter {p.group(2)!r}", decl)
            argtypes.append(C.c_void_p if "*" in t else RESIZE_FN if t == "mi_rast_resize_fn" else _SCALARS[t])
        functions.append((m.group(2), _RETURNS[_ctype(m.group(1))], argtypes))
    return functions, constants


DECLARED = {}      # header base name -> its functions in declaration order
SIGNATURES = {}    # function -> (restype, [argtypes])
CONSTANTS = {}     # every MI_* define with an integer value and every enumerator
for _path in HEADERS:
    _header = os.path.basename(_path)
    with open(_path) as _f:
        _functions, _constants = parse_header(_f.read(), _header)
    DECLARED[_header] = [n for n, _, _ in _functions]
    _again = sorted(set(DECLARED[_header]) & set(SIGNATURES) | set(_constants) & set(CONSTANTS))
    if _again or len(set(DECLARED[_header])) != len(_functions):
        raise MiRastError(f"{_header}: declared twice: {_again or DECLARED[_header]}")
    SIGNATURES.update((n, (r, a)) for n, r, a in _functions)
    CONSTANTS.update(_constants)
globals().update(CONSTANTS)     # _lib.MI_RAST_FULL_LISTS, _lib.MI_SEGMENT_MAX_CHANNELS, ...
ALL_EXPORTS = [n for names in DECLARED.values() for n in names]   # every function the headers in include/ declare


def _named(prefix, *names):
    return {n: CONSTANTS[prefix + n.upper()] for n in names}


MI_VIEW_MODES = _named("MI_VIEW_", "rgb", "pca", "cluster", "similarity")
MI_MASK_SCORE_MODE = _named("MI_MASK_SCORE_", "sum", "mean", "max")
MI_CLIP_TILES_LAYOUT = _named("MI_CLIP_TILES_", "crop", "pad_square")
MI_CLUSTER_METRIC = _named("MI_CLUSTER_", "euclidean", "jaccard")
MI_SEGMENT_PRE = _named("MI_SEGMENT_PRE_", "none", "l2", "eps")
MI_SCALE_GATE = _named("MI_SCALE_GATE_", "none", "learned", "fixed")

# the fields of the layout, profile and count tables in the order of their enums: written out, for their case is not the enumerators'
MI_GEOM_FIELDS = ["depths", "means2D", "conic_opacity", "cov3D", "rgb", "clamped", "tiles_touched",
                  "depth_key", "index_rec", "cull_counter", "band_bits", "bwd_pack"]
MI_IMG_FIELDS = ["final_T", "n_contrib", "ranges", "tile_consumed", "tile_count", "tile_cursor", "num_rendered", "tile_nsurv"]
MI_BIN_FIELDS = ["entries", "scratch", "blend_list"]
MI_STAGES = ["preprocess", "tile_scan", "emit", "tile_sort", "blend_fwd", "blend_bwd", "geom_bwd"]
MI_TRAIN_COUNTS = ["clones", "splits", "kept_originals", "kept_clones", "kept_children"]
MI_EDIT_COUNTS = ["current", "selected", "kept"]
for _fields, _prefix, _count in ((MI_GEOM_FIELDS, "MI_GEOM_", "MI_GEOM_NFIELDS"), (MI_IMG_FIELDS, "MI_IMG_", "MI_IMG_NFIELDS"),
                                 (MI_BIN_FIELDS, "MI_BIN_", "MI_BIN_NFIELDS"), (MI_STAGES, "MI_STAGE_", "MI_STAGE_COUNT"),
                                 (MI_TRAIN_COUNTS, "MI_TRAIN_", "MI_TRAIN_NCOUNTS"), (MI_EDIT_COUNTS, "MI_EDIT_", "MI_EDIT_NCOUNTS")):
    if [CONSTANTS.get(_prefix + n.upper()) for n in _fields] != list(range(CONSTANTS[_count])):
        raise MiRastError(f"{_fields} are not the {_count} = {CONSTANTS[_count]} enumerators {_prefix}* of the headers, in order")

_lib = None


def load():
    """Returns the loaded library; raises MiRastError if libmi_rast.so is absent or unloadable."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm ships its own HIP runtime; load it first so that this library binds to the same one (loading
    # /opt/rocm's copy first leaves the process with a runtime that sees no device once torch initialises its own)
    import torch  # noqa: F401
    lib_path = os.environ.get("MI_RAST_LIB") or LIB_PATH   # MI_RAST_LIB: e.g. the profiling build (build.py), for tools/
    if not os.path.exists(lib_path):
        raise MiRastError(
            f"HIP extension {lib_path} is missing. Build it with `python -m seganygaussians_amd.build` "
            "(or __graft_entry__.build()). There is no CPU fallback.")
    try:
        L = C.CDLL(lib_path)
    except OSError as e:  # e.g. libamdhip64 missing
        raise MiRastError(f"cannot load {lib_path}: {e}") from e
    try:
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    except AttributeError:     # a library built from other sources than these headers
        raise MiRastError(f"the HIP library lacks {name} (rebuild it: python -m seganygaussians_amd.build)") from None
    _lib = L
    return L


def last_error() -> str:
    return load().mi_rast_last_error().decode("utf-8", "replace")


def geometry_layout(P: int):
    off = (C.c_size_t * len(MI_GEOM_FIELDS))()
    total = load().mi_rast_geometry_layout(int(P), off)
    return int(total), dict(zip(MI_GEOM_FIELDS, [int(o) for o in off]))


def image_layout(W: int, H: int):
    off = (C.c_size_t * len(MI_IMG_FIELDS))()
    total = load().mi_rast_image_layout(int(W), int(H), off)
    return int(total), dict(zip(MI_IMG_FIELDS, [int(o) for o in off]))


def binning_layout(R: int):
    off = (C.c_size_t * len(MI_BIN_FIELDS))()
    total = load().mi_rast_binning_layout(int(R), off)
    return int(total), dict(zip(MI_BIN_FIELDS, [int(o) for o in off]))


def profile_enable(on: bool) -> None:
    if load().mi_rast_profile_enable(1 if on else 0) != 0:
        raise MiRastError(last_error())


def profile_read() -> dict:
    ms = (C.c_float * len(MI_STAGES))()
    if load().mi_rast_profile_read(ms) != 0:
        raise MiRastError(last_error())
    return dict(zip(MI_STAGES, [float(x) for x in ms]))
