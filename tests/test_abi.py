"""CPU-side checks of the C-ABI boundary: the HIP library builds for gfx950, loads, and exports every
symbol the headers in include/ declare; host-side helpers agree with the oracle.  No compute calls (no GPU)."""
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
    is listed."""
    hdr = "".join(open(h).read() for h in build.HEADERS)
    declared = set(re.findall(r"\b(mi_[a-z_0-9]+)\s*\(", hdr)) - {"mi_rast_resize_fn"}
    assert len(build.HEADERS) == 7 and len(_lib.ALL_EXPORTS) == len(set(_lib.ALL_EXPORTS))
    assert declared == set(_lib.ALL_EXPORTS), declared ^ set(_lib.ALL_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
        assert ctypes.cast(getattr(lib, name), ctypes.c_void_p).value


# one call per host file of csrc/ that is refused for its arguments before any HIP call (the pointers are never read), and its message
REFUSED = [
    ("mi_rast_forward_reuse", (0, 3, 0, None, 16, 16) + (None,) * 6 + (0,) + (None,) * 4 + (0,) + (None,) * 3, "P, width and height must be positive"),
    ("mi_knn_query", (4, 8, 4, 8, 5, 0, 8, 8, None), "knn: K must be one of 1, 3, 4, 8, 16, 32"),
    ("mi_knn_smooth_forward", (4, 48, 8, 8, 0xFF, 8, 8, 0, None), "knn_smooth: need C in {32, 64} and 1 <= K <= 32"),
    ("mi_contrastive_pack_masks", (0, 4, 4, 8, 8, None), "contrastive loss: need 1 <= M <= 1024 masks and H, W >= 1"),
    ("mi_mask_erode", (0, 4, 4, 8, 4, 4, 4096, None), "mask scales: need 1 <= M <= 1024 masks and h, w >= 1"),
    ("mi_segment_scores", (2, 4, 4, 1, 8, 8, None, 0, 1, 8, None), "segment: layout must be MI_SEGMENT_IMAGE or MI_SEGMENT_POINTS"),
    ("mi_photo_loss_forward", (0, 3, 4, 4, 8, 8, 0.2, 3, None, 8, 1 << 20, 8, None), "photometric: need images, planes, H, W >= 1"),
]


def test_last_error_is_one_per_thread_for_every_host_file(lib):
    """The host side is one translation unit per public header: what any of them refuses must be what mi_rast_last_error()
    (mi_rast.hip) returns -- one thread-local string for the whole library, not one per file."""
    import threading
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
