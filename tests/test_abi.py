"""CPU-side checks of the C-ABI boundary: the HIP library builds for gfx950, loads, and exports every
symbol the headers in include/ declare; what _lib.py reads off the headers (signatures, constants) is what a C++ compiler reads;
host-side helpers agree with the oracle.  No compute calls (no GPU)."""
import ctypes
import os
import re

import pytest

from oracle import saga_oracle as so
from seganygaussians_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def test_header_symbols_exported(lib):
    """Every function that a header in include/ declares is listed in _lib.ALL_EXPORTS and resolves in the library, and nothing else
    is listed; each is declared in exactly one header, the one _lib.DECLARED lists it under."""
    hdr = "".join(open(h).read() for h in build.HEADERS)
    declared = set(re.findall(r"\b(mi_[a-z_0-9]+)\s*\(", hdr)) - {"mi_rast_resize_fn"}
    assert len(build.HEADERS) == 15 and len(_lib.ALL_EXPORTS) == len(set(_lib.ALL_EXPORTS))
    assert declared == set(_lib.ALL_EXPORTS), declared ^ set(_lib.ALL_EXPORTS)
    code = {os.path.basename(h): re.sub(r"/\*.*?\*/", " ", open(h).read(), flags=re.S) for h in build.HEADERS}   # comments name functions too
    for name in declared:
        assert hasattr(lib, name), name
        assert ctypes.cast(getattr(lib, name), ctypes.c_void_p).value
        where = [h for h, text in code.items() for _ in re.findall(rf"\b{name}\s*\(", text)]
        assert len(where) == 1 and name in _lib.DECLARED[where[0]], (name, where)


def test_one_public_header_per_host_file():
    """For every csrc/mi_X.hip there is exactly one include/mi_X.h and the reverse, and mi_X.h declares exactly the extern "C" functions
    that mi_X.hip defines (read off the file: a definition is `type mi_name(...)` followed by its body, not by a semicolon)."""
    hips = [s for s in build.SOURCES if s.endswith(".hip")]
    assert {os.path.basename(h)[:-2] for h in build.HEADERS} == {s[:-4] for s in hips} and len(hips) == len(build.HEADERS) == 15
    assert not [s for s in build.SOURCES if s.startswith("mi_") and s.endswith(".h")]      # no public header is left among the kernels
    for hip in hips:
        text = open(os.path.join(build.SRC_DIR, hip)).read()
        assert 'extern "C"' in text, hip
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
        defined = re.findall(r"^[\w \t*]*?\b(mi_[a-z_0-9]+)\s*\([^;{}]*\)\s*\{", text, flags=re.M)
        assert sorted(defined) == sorted(_lib.DECLARED[hip[:-4] + ".h"]) and len(defined) == len(set(defined)), hip
        # its own public header is the first thing it includes after host.h: a definition that disagrees with its declaration does not compile
        includes = re.findall(r'^#include\s+"([^"]+)"', text, flags=re.M)
        assert includes[:2] == ["host.h", f"../../include/{hip[:-4]}.h"] or hip == "mi_rast.hip" and includes[0] == "host.h", hip
    assert '#include "../../include/mi_rast.h"' in open(os.path.join(build.SRC_DIR, "host.h")).read()      # mi_rast.h comes with host.h, for all


# ---- the compiler as witness: what a C++ compiler makes of the headers is what _lib read off them ----
_WITNESS = r"""
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <type_traits>
%(includes)s
template <class T, bool is_return> constexpr char code() {
    if constexpr (std::is_void_v<T>) return 'v';
    else if constexpr (is_return && std::is_same_v<T, const char*>) return 's';
    else if constexpr (std::is_same_v<T, mi_rast_resize_fn>) return 'c';
    else if constexpr (std::is_pointer_v<T>) return 'p';
    else if constexpr (std::is_same_v<T, int>) return 'i';
    else if constexpr (std::is_same_v<T, uint32_t>) return 'u';
    else if constexpr (std::is_same_v<T, size_t>) return 'z';
    else if constexpr (std::is_same_v<T, float>) return 'f';
    else if constexpr (std::is_same_v<T, double>) return 'd';
    else return '?';
}
template <class F> struct Sig;
template <class R, class... A> struct Sig<R (*)(A...)> {
    static void print(const char* name) { const char p[] = {code<A, false>()..., 0}; std::printf("F %%s %%c %%s\n", name, code<R, true>(), p); }
};
int main() {
%(body)s
}
"""
_CODES = {None: "v", ctypes.c_char_p: "s", _lib.RESIZE_FN: "c", ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_uint32: "u",
          ctypes.c_size_t: "z", ctypes.c_float: "f", ctypes.c_double: "d"}


def test_compiler_reads_the_headers_as_lib_does(tmp_path):
    """A host-only C++ program prints the class of the return type and of every parameter of each declared function, taken from
    decltype(&name) (nothing is linked against the library), and the value of every constant; both must be _lib's tables."""
    import shutil
    import subprocess
    cxx = shutil.which("c++") or next(p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p))
    body = [f'    Sig<decltype(&{n})>::print("{n}");' for n in _lib.ALL_EXPORTS]
    body += [f'    std::printf("C {n} %lld\\n", (long long)({n}));' for n in _lib.CONSTANTS]
    (src := tmp_path / "witness.cpp").write_text(_WITNESS % {"includes": "\n".join(f'#include "{os.path.basename(h)}"' for h in build.HEADERS), "body": "\n".join(body)})
    subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "witness")])
    lines = [line.split(" ") for line in subprocess.check_output([str(tmp_path / "witness")], text=True).splitlines()]
    seen = {l[1]: (l[2], l[3]) for l in lines if l[0] == "F"}     # "F name v " for an empty parameter list: l[3] == ""
    assert len(seen) == len(_lib.SIGNATURES) == 80 and len(lines) == 80 + len(_lib.CONSTANTS)
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        assert seen[name] == (_CODES[restype], "".join(_CODES[a] for a in argtypes)) and "?" not in "".join(seen[name]), name
    assert {l[1]: int(l[2]) for l in lines if l[0] == "C"} == _lib.CONSTANTS


@pytest.mark.parametrize("text, named", [
    ("int mi_f(int n, long double x);", "mi_f"), ("int mi_f(float v[3]);", "mi_f"), ("int mi_f(int n, mi_handle_t h);", "mi_f"),
    ("int mi_f(char* (*resize)(size_t nbytes, void* user), void* user);", "mi_f"), ("#define MI_X 1.5", "MI_X")])
def test_parser_refuses_what_it_does_not_understand(text, named):
    with pytest.raises(_lib.MiRastError, match=rf"mi_some\.h: .*\b{named}\b"):
        _lib.parse_header("int mi_ok(void);\n" + text + "\n", "mi_some.h")


def test_parser_skips_comments_and_guards_and_counts_enumerators():
    assert _lib.parse_header("/* int mi_f(int x); */\n// int mi_g(void);\n") == ([], {})
    functions, constants = _lib.parse_header(
        "#ifndef MI_T_H\n#define MI_T_H\n#define MI_E (1 << 4)   /* int mi_h(void); */\nenum { MI_A = 3, MI_B, MI_C = 0x10, MI_D };\n"
        "const char* mi_s(void);\nvoid mi_v(const float* const* t, uint32_t m, mi_rast_resize_fn f);\n#endif\n")
    assert constants == {"MI_E": 16, "MI_A": 3, "MI_B": 4, "MI_C": 16, "MI_D": 17}
    assert functions == [("mi_s", ctypes.c_char_p, []), ("mi_v", None, [ctypes.c_void_p, ctypes.c_uint32, _lib.RESIZE_FN])]


def test_lib_binds_in_one_loop_only():
    """_lib.py states no signature of its own: restype and argtypes are assigned once, in the loop over SIGNATURES, no header text is
    evaluated, and the hand-kept export lists are gone."""
    src = open(_lib.__file__).read().splitlines()
    hits = [k for k, line in enumerate(src) if re.search(r"\.(argtypes|restype)\b", line)]
    assert len(hits) == 1 and src[hits[0]].strip() == "fn.restype, fn.argtypes = restype, argtypes"
    assert src[hits[0] - 2].strip() == "for name, (restype, argtypes) in SIGNATURES.items():"
    assert not re.search(r"\b(eval|exec)\s*\(", "\n".join(src))
    assert [n for n in vars(_lib) if n.endswith("EXPORTS")] == ["ALL_EXPORTS"]
    # and _lib is the only binder: no other file of the package assigns a signature or parses a header
    package = os.path.dirname(_lib.__file__)
    for root, _, files in os.walk(package):
        for f in files:
            if f.endswith(".py") and os.path.join(root, f) != _lib.__file__:
                assert not re.search(r"\.(argtypes|restype)\b|\bparse_header\b", open(os.path.join(root, f)).read()), os.path.join(root, f)


def test_a_library_without_a_declared_symbol_is_refused_by_load(tmp_path, monkeypatch):
    """What the headers declare and a library does not export is an error when the library is loaded, named, not an AttributeError
    at the first call."""
    import shutil
    import subprocess
    cxx = shutil.which("c++") or next(p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p))
    (src := tmp_path / "empty.cpp").write_text('extern "C" int mi_unrelated(void) { return 0; }\n')
    subprocess.check_call([cxx, "-shared", "-fPIC", str(src), "-o", str(tmp_path / "libempty.so")])
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setenv("MI_RAST_LIB", str(tmp_path / "libempty.so"))
    with pytest.raises(_lib.MiRastError, match=rf"the HIP library lacks {_lib.ALL_EXPORTS[0]} \(rebuild it: python -m seganygaussians_amd\.build\)"):
        _lib.load()
    assert _lib._lib is None


# one call per host file of csrc/ that is refused for its arguments before any HIP call (the pointers are never read), and its message
REFUSED = [
    ("mi_rast_forward_reuse", (0, 3, 0, None, 16, 16) + (None,) * 6 + (0,) + (None,) * 4 + (0,) + (None,) * 3, "P, width and height must be positive"),
    ("mi_knn_query", (4, 8, 4, 8, 5, 0, 8, 8, None), "knn: K must be one of 1, 3, 4, 8, 16, 32"),
    ("mi_knn_smooth_forward", (4, 48, 8, 8, 0xFF, 8, 8, 0, None), "knn_smooth: need C in {32, 64} and 1 <= K <= 32"),
    ("mi_contrastive_pack_masks", (0, 4, 4, 8, 8, None), "contrastive loss: need 1 <= M <= 1024 masks and H, W >= 1"),
    ("mi_mask_erode", (0, 4, 4, 8, 4, 4, 4096, None), "mask scales: need 1 <= M <= 1024 masks and h, w >= 1"),
    ("mi_segment_scores", (2, 4, 4, 1, 8, 8, None, 0, 1, 8, None), "segment: layout must be MI_SEGMENT_IMAGE or MI_SEGMENT_POINTS"),
    ("mi_photo_loss_forward", (0, 3, 4, 4, 8, 8, 0.2, 3, None, 8, 1 << 20, 8, None), "photometric: need images, planes, H, W >= 1"),
    ("mi_cluster_core_distances", (2, 100, 32, 8, 10, 8, 8, 1 << 20, None), "cluster: metric must be MI_CLUSTER_EUCLIDEAN or MI_CLUSTER_JACCARD"),
    ("mi_vote_relevancy", (3, 1025, 1, 1, 4096, 0, 4096, 4096, 1, 4096, None), "vote graph: need N >= 1 rows and 1 <= D <= 1024"),
    ("mi_view_frame", (0, 4, 8, 8, None, None, 0, None, None, 0.5, 1, 0, 8, None, None, None), "view frame: need N >= 1 and 1 <= C <= 256"),
    ("mi_mask_nms_keep", (1025, 8, 8, 8, 0.7, 0.1, 0.8, 8, None), "mask nms: need 1 <= M <= 1024 masks"),
    ("mi_mask_index_map", (1025, 4, 4, 8, 0, 8, None), "clip tiles: need 1 <= M <= 1024 masks and H, W >= 1"),
    ("mi_train_densify_plan", (0, 1 << 20, 2 << 20, 3 << 20, 4 << 20, 2e-4, 0.005, 5.0, 0.01, 1, 8 << 20, 1 << 20, 16 << 20, None), "densify: need 1 <= P < 2^30 rows"),
    ("mi_scale_gate_forward", (0, 8, 4, 8, 8, 0, 1, None, None, 0, 8, None, None), "scale gate: need 1 <= n < 2^30 scales"),
    ("mi_edit_plan", (0, 8, 0, 1, 8, 8, 1 << 20, None), "model edit: need 1 <= P0 < 2^30 rows"),
]


def test_last_error_is_one_per_thread_for_every_host_file(lib):
    """The host side is one translation unit per public header: what any of them refuses must be what mi_rast_last_error()
    (mi_rast.hip) returns -- one thread-local string for the whole library, not one per file."""
    import threading
    owners = [next(h for h, names in _lib.DECLARED.items() if name in names) for name, _, _ in REFUSED]
    assert sorted(owners) == sorted(_lib.DECLARED) and len(owners) == 15      # one refused call of every host file
    for name, args, msg in REFUSED:
        assert getattr(lib, name)(*args) != 0, name
        assert _lib.last_error() == msg, name
    mine, seen = _lib.last_error(), []

    def other():
        seen.append(_lib.last_error())   # a new thread: no message yet
        seen.append(lib.mi_knn_query(4, 8, 4, 8, 5, 0, 8, 8, None))
        seen.append(_lib.last_error())
    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen[0] == "" and seen[1] != 0 and seen[2] == REFUSED[1][2]
    assert _lib.last_error() == mine == REFUSED[-1][2]   # the other thread's message is not visible here


def test_no_torch_types_in_abi():
    hdr = open(os.path.join(ROOT, "include", "mi_rast.h")).read()
    assert "torch" not in open(os.path.join(ROOT, "include", "mi_knn_smooth.h")).read().replace("torch.randperm", "").replace("PyTorch", "").replace("torch.nn", "")
    assert "torch" not in hdr.replace("torch glue", "").replace("torch::zeros", "").replace("torch.bool", "").replace("no torch", "")
    assert 'extern "C"' in hdr


def test_get_higher_msb_matches_oracle_and_reference_cases(lib):
    # CF/cuda_rasterizer/rasterizer_impl.cu:35-50; 1080p -> 8160 tiles -> 13 bits; 256x256 -> 256 tiles -> 9 bits
    assert lib.mi_rast_get_higher_msb(8160) == 13 == so.get_higher_msb(8160)
    assert lib.mi_rast_get_higher_msb(256) == 9 == so.get_higher_msb(256)
    for n in [1, 2, 3, 4, 7, 8, 9, 255, 256, 257, 6700, 65535, 65536, 1 << 20, (1 << 31) + 5]:
        assert lib.mi_rast_get_higher_msb(n) == so.get_higher_msb(n), n


def test_supported_channels(lib):
    arr = (ctypes.c_int * 300)()
    n = lib.mi_rast_supported_channels(arr, 300)
    assert list(arr[:n]) == list(range(1, 257))      # any width up to 256 (channel blocks of 64 / 32 / 16, the last one possibly partial)
    assert lib.mi_rast_supported_channels(arr, 2) == n and list(arr[:2]) == [1, 2]


def test_layouts_are_aligned_and_disjoint(lib):
    for P in (1, 1000, 1_000_000):
        total, off = _lib.geometry_layout(P)
        vals = sorted(off.values())
        assert all(v % 256 == 0 for v in vals) and len(set(vals)) == len(vals) and total >= vals[-1]
    total, off = _lib.binning_layout(12_345_678)
    assert off["blend_list"] == 0 and off["entries"] - off["blend_list"] >= 4 * 12_345_678   # the blend list first (mi_rast_forward_reuse)
    assert off["scratch"] - off["entries"] >= 8 * 12_345_678 and total - off["scratch"] >= 8 * 12_345_678
    total, off = _lib.image_layout(1920, 1080)
    assert off["n_contrib"] - off["final_T"] >= 4 * 1920 * 1080
    assert off["tile_count"] - off["tile_consumed"] >= 4 * 8160


def test_product_path_has_no_cpu_fallback():
    """The product package must never import the oracle, and must fail loudly without a GPU tensor."""
    import torch
    for root, _, files in os.walk(os.path.join(ROOT, "seganygaussians_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, os.path.join(root, f)
    import seganygaussians_amd
    seganygaussians_amd.install_dropin()
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    s = GaussianRasterizationSettings(16, 16, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0,
                                      torch.zeros(3), False, False)
    m = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        GaussianRasterizer(s)(means3D=m, means2D=m, opacities=torch.ones(4, 1), colors_precomp=torch.ones(4, 3),
                              scales=torch.ones(4, 3), rotations=torch.ones(4, 4))
