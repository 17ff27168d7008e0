"""Builds the HIP C-ABI library in-tree (seganygaussians_amd/libmi_rast.so) with hipcc for gfx950.

hipcc cross-compiles without a GPU, so this runs in the CPU-only build container; the resulting
.so is git-ignored but travels to the GPU box with the repo snapshot.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmi_rast.so")
PROF_LIB_PATH = os.path.join(_HERE, "libmi_rast_prof.so")
SRC_DIR = os.path.join(_HERE, "csrc")
_INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")
# what a library is built from, read off the directories (is_stale() and source_hash() both go by these): every kernel header and
# host file in csrc/, every public header in include/ (csrc/mi_X.hip defines what include/mi_X.h declares: tests/test_abi.py)
SOURCES = sorted(f for f in os.listdir(SRC_DIR) if f.endswith((".h", ".hip")))
HEADERS = [os.path.join(_INCLUDE_DIR, h) for h in sorted(os.listdir(_INCLUDE_DIR)) if h.endswith(".h")]

# -ffp-contract=off is part of the numeric contract: the geometry path that feeds the
# integer tile/sort results must round every binary32 op separately, like the oracle.
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-munsafe-fp-atomics",
               "-fPIC", "-shared", "-Wno-unused-result", "-fno-slp-vectorize"]


def source_hash(extra_flags=()) -> str:
    """Stamp of what a library is built from: the kernel sources, the C-ABI headers and the compiler flags.  Compiled into the
    library (mi_rast_version()) so that measurements taken with one build -- profiles/traffic_*.json, alu_*.json -- are never
    reported next to timings of another (bench.py prints null instead)."""
    import hashlib
    h = hashlib.sha256()
    for path in sorted([os.path.join(SRC_DIR, f) for f in SOURCES] + HEADERS):
        h.update(os.path.basename(path).encode())
        h.update(open(path, "rb").read())
    h.update(" ".join(list(HIPCC_FLAGS) + list(extra_flags)).encode())
    return h.hexdigest()[:12]


def _hash_flag(extra_flags=()):
    return ['-DMI_RAST_SRC_HASH="' + source_hash(extra_flags) + '"']


def find_hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (expected /opt/rocm/bin/hipcc)")


def is_stale(lib_path: str = None) -> bool:
    lib_path = lib_path or LIB_PATH
    if not os.path.exists(lib_path):
        return True
    t = os.path.getmtime(lib_path)
    deps = [os.path.join(SRC_DIR, s) for s in SOURCES] + HEADERS
    return any(os.path.getmtime(d) > t for d in deps)


def compile_library(out_path: str, extra_flags=(), verbose: bool = False) -> str:
    """The one compile path of every library: each csrc/*.hip to an object of its own (HIPCC_FLAGS + extra_flags, at most 16 at a
    time, in a temporary directory), then one link into <out_path>.tmp, renamed over out_path.  No object is kept between builds."""
    def run(cmd):
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    cc = [find_hipcc()] + [f for f in HIPCC_FLAGS if f != "-shared"] + list(extra_flags) + _hash_flag(extra_flags) + ["-c"]
    units = [s[:-4] for s in SOURCES if s.endswith(".hip")]
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(16) as pool:
        objs = [os.path.join(tmp, u + ".o") for u in units]
        list(pool.map(run, [cc + [os.path.join(SRC_DIR, u + ".hip"), "-o", o] for u, o in zip(units, objs)]))
        run([find_hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared", "-o", out_path + ".tmp"] + objs)
    os.replace(out_path + ".tmp", out_path)
    return out_path


def build_library(force: bool = False, verbose: bool = False) -> str:
    if not force and not is_stale():
        return LIB_PATH
    return compile_library(LIB_PATH, verbose=verbose)


def build_profiling_library(verbose: bool = False) -> str:
    """The same sources with -DMI_RAST_PROFILING: the comparison forward kernels selected by MI_RAST_TILE_FWD (tile-batched
    bf16x3 / RGB) and MI_RAST_F32_BLEND (f32 FMA chain, the tests' bit-exact reference), and per-wave XCD time stamps in the
    blend kernels (mi_rast_xcd_stamps, tools/xcd_stamps.py).  For tests and tools/ only; the product library carries none of
    it.  Select it with MI_RAST_LIB=<path> (seganygaussians_amd/_lib.py)."""
    return compile_library(PROF_LIB_PATH, ["-DMI_RAST_PROFILING"], verbose=verbose)


if __name__ == "__main__":
    import sys
    if "--profiling" in sys.argv:
        print(build_profiling_library(verbose=True))
    else:
        print(build_library(force=True, verbose=True))
