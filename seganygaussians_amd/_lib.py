"""ctypes binding of the C-ABI library (include/mi_rast.h).  Fails loudly when the HIP extension is
missing: there is NO CPU / PyTorch fallback in the product path."""
from __future__ import annotations

import ctypes as C
import os

from .build import LIB_PATH

RESIZE_FN = C.CFUNCTYPE(C.c_void_p, C.c_size_t, C.c_void_p)

MI_GEOM_FIELDS = ["depths", "means2D", "conic_opacity", "cov3D", "rgb", "clamped", "tiles_touched",
                  "depth_key", "index_rec", "cull_counter", "band_bits", "bwd_pack"]
MI_IMG_FIELDS = ["final_T", "n_contrib", "ranges", "tile_consumed", "tile_count", "tile_cursor", "num_rendered", "tile_nsurv"]
MI_BIN_FIELDS = ["entries", "scratch", "blend_list"]
MI_RAST_FULL_LISTS, MI_RAST_F32_BLEND, MI_RAST_NO_CULL, MI_RAST_FAST_EXP, MI_RAST_VERIFY_LISTS, MI_RAST_TILE_FWD = 1, 2, 4, 8, 16, 32   # `flags` of mi_rast_forward (include/mi_rast.h)
MI_RAST_PREZERO_BWD = 64   # forward + the one backward of that forward (include/mi_rast.h)
MI_RAST_EXACT_EXP = 128    # forward blend with expf for every pair instead of the hybrid form (include/mi_rast.h)
MI_RAST_EQUAL_RUNS = 256   # A/B aid: XCD runs of equal tile counts in both blend kernels instead of equal modelled work (include/mi_rast.h)
MI_RAST_BWD_FEATURES_ONLY = 512   # mi_rast_backward: dL_dcolor alone (extension, include/mi_rast.h)
MI_STAGES = ["preprocess", "tile_scan", "emit", "tile_sort", "blend_fwd", "blend_bwd", "geom_bwd"]

# include/mi_segment.h, its clustering section (csrc/mi_cluster.hip); listed on its own and as the tail of EXPORTS
CLUSTER_EXPORTS = ["mi_cluster_workspace_bytes", "mi_cluster_core_distances", "mi_cluster_mst", "mi_cluster_mst_rounds", "mi_cluster_labels_host"]
# include/mi_rast.h, its score-lifting section (csrc/lift.h); listed on its own and as the tail of EXPORTS
LIFT_EXPORTS = ["mi_rast_lift", "mi_rast_lift_reuse"]
MI_RAST_LIFT_MAX_CHANNELS = 64
# include/mi_segment.h, its vote-graph section (csrc/mi_vote_graph.hip); listed on its own and as the tail of EXPORTS
VOTE_GRAPH_EXPORTS = ["mi_vote_mask_features_workspace_bytes", "mi_vote_mask_features", "mi_vote_anchor_bits", "mi_vote_relevancy"]
# include/mi_segment.h, its viewer-frame section (csrc/mi_viewer.hip); listed on its own and as the tail of EXPORTS
VIEWER_EXPORTS = ["mi_view_moments_workspace_bytes", "mi_view_moments_block", "mi_view_moments", "mi_view_frame"]
MI_VIEW_MODES = {"rgb": 1, "pca": 2, "cluster": 4, "similarity": 8}
EXPORTS = [
    "mi_rast_forward", "mi_rast_forward_reuse", "mi_rast_last_longest_run", "mi_rast_fingerprint", "mi_rast_features_only_supported", "mi_rast_backward", "mi_rast_mark_visible", "mi_rast_mask_forward",
    "mi_rast_mask_backward", "mi_rast_last_error", "mi_rast_version", "mi_rast_supported_channels",
    "mi_rast_get_higher_msb", "mi_rast_geometry_layout", "mi_rast_image_layout", "mi_rast_binning_layout",
    "mi_rast_profile_enable", "mi_rast_profile_read",
    "mi_knn_smooth_forward", "mi_knn_smooth_backward", "mi_knn_smooth_multi_forward", "mi_knn_smooth_multi_backward",  # include/mi_knn_smooth.h
    "mi_knn_workspace_bytes", "mi_knn_build", "mi_knn_query", "mi_knn_mean_dist2",  # include/mi_knn.h
    "mi_contrastive_forward", "mi_contrastive_backward",  # include/mi_contrastive.h
    "mi_contrastive_pack_masks", "mi_contrastive_cover", "mi_contrastive_targets", "mi_contrastive_loss_forward",
    "mi_contrastive_loss_backward",  # include/mi_contrastive.h: the loss itself
] + CLUSTER_EXPORTS + LIFT_EXPORTS + VOTE_GRAPH_EXPORTS + VIEWER_EXPORTS
# include/mi_mask_scales.h, its mask-sets section (csrc/mi_mask_sets.hip); listed on its own and as the tail of MASK_SCALES_EXPORTS
MASK_SETS_EXPORTS = ["mi_mask_overlaps", "mi_mask_boxes", "mi_mask_nms_keep", "mi_mask_score_images"]
MI_MASK_SCORE_MODE = {"sum": 0, "mean": 1, "max": 2}
MI_MASK_SCORE_MAX_COLUMNS = 64
# include/mi_mask_scales.h, its CLIP-tiles section (csrc/mi_clip_tiles.hip; mi_mask_resize in csrc/mi_mask_scales.hip)
CLIP_TILES_EXPORTS = ["mi_mask_resize", "mi_mask_clip_tiles", "mi_mask_index_map"]
MI_CLIP_TILES_LAYOUT = {"crop": 0, "pad_square": 1}
MI_CLIP_TILES_MAX_SIZE, MI_CLIP_TILES_MAX_SIDE = 512, 32768
MASK_SCALES_EXPORTS = ["mi_mask_scales_workspace_bytes", "mi_mask_erode", "mi_mask_erode_min_sum", "mi_mask_scales"] + MASK_SETS_EXPORTS + CLIP_TILES_EXPORTS   # include/mi_mask_scales.h
MI_VOTE_MAX_ANCHORS, MI_VOTE_MAX_EMBED_DIM, MI_VOTE_MAX_PROMPTS = 32768, 1024, 16
SEGMENT_EXPORTS = ["mi_segment_scores", "mi_segment_select", "mi_segment_assign", "mi_segment_assign_block"]   # include/mi_segment.h
MI_SEGMENT_IMAGE, MI_SEGMENT_POINTS = 0, 1
PHOTOMETRIC_EXPORTS = ["mi_photo_loss_workspace_bytes", "mi_photo_loss_window", "mi_photo_loss_forward", "mi_photo_loss_backward"]   # include/mi_photometric.h
MI_PHOTO_L1, MI_PHOTO_SSIM = 1, 2
# include/mi_rast.h, its training-step section (csrc/mi_train_step.hip)
TRAIN_STEP_EXPORTS = ["mi_train_adam_step", "mi_train_densify_stats", "mi_train_densify_workspace_bytes", "mi_train_densify_plan",
                      "mi_train_densify_counts", "mi_train_densify_apply"]
MI_TRAIN_COUNTS = ["clones", "splits", "kept_originals", "kept_clones", "kept_children"]
MI_TRAIN_COPY, MI_TRAIN_MOMENT, MI_TRAIN_XYZ, MI_TRAIN_SCALING, MI_TRAIN_ROTATION = 0, 1, 2, 3, 4
MI_TRAIN_ADAM_MAX_TENSORS, MI_TRAIN_DENSIFY_MAX_TENSORS = 16, 32
MI_CLUSTER_METRIC = {"euclidean": 0, "jaccard": 1}
MI_CLUSTER_MAX_POINTS, MI_CLUSTER_MAX_CHANNELS, MI_CLUSTER_MAX_WORDS, MI_CLUSTER_MAX_CORE_K = 1 << 20, 256, 1024, 64
ALL_EXPORTS = EXPORTS + MASK_SCALES_EXPORTS + SEGMENT_EXPORTS + PHOTOMETRIC_EXPORTS + TRAIN_STEP_EXPORTS   # every function the headers in include/ declare
MI_SEGMENT_PRE = {"none": 0, "l2": 1, "eps": 2}

_lib = None


class MiRastError(RuntimeError):
    pass


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
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    L.mi_rast_forward.restype = i
    L.mi_rast_forward.argtypes = [RESIZE_FN, vp, RESIZE_FN, vp, RESIZE_FN, vp, i, i, i, i, vp, i, i,
                                  vp, vp, vp, vp, vp, f, vp, vp, vp, vp, vp, f, f, i,
                                  vp, vp, vp, vp, vp, i, i, vp, vp, vp, C.POINTER(i)]
    L.mi_rast_forward_reuse.restype = i
    L.mi_rast_forward_reuse.argtypes = [i, i, i, vp, i, i, vp, vp, vp, vp, vp, vp, i, vp, vp, vp, vp, i, vp, vp, vp]
    L.mi_rast_fingerprint.restype = i
    L.mi_rast_fingerprint.argtypes = [i, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), vp]
    L.mi_rast_last_longest_run.restype = i
    L.mi_rast_last_longest_run.argtypes = []
    L.mi_rast_features_only_supported.restype = i
    L.mi_rast_features_only_supported.argtypes = [i]
    L.mi_rast_backward.restype = i
    L.mi_rast_backward.argtypes = [i, i, i, i, i, vp, i, i, vp, vp, vp, vp, f, vp, vp, vp, vp, vp, f, f,
                                   vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, vp]
    L.mi_rast_mark_visible.restype = i
    L.mi_rast_mark_visible.argtypes = [i, vp, vp, vp, vp, vp]
    L.mi_rast_mask_forward.restype = i
    L.mi_rast_mask_forward.argtypes = [RESIZE_FN, vp, RESIZE_FN, vp, RESIZE_FN, vp, i, i, i, vp, vp, vp, vp, f,
                                       vp, vp, vp, vp, f, f, i, vp, vp, i, i, vp, C.POINTER(i)]
    L.mi_rast_mask_backward.restype = i
    L.mi_rast_mask_backward.argtypes = [i, i, i, i, vp, vp, vp, vp, vp, i, i, vp]
    L.mi_rast_lift.restype = i
    L.mi_rast_lift.argtypes = [RESIZE_FN, vp, RESIZE_FN, vp, RESIZE_FN, vp, i, i, i, i, vp, vp, vp, f, vp, vp, vp, vp, f, f, i,
                               vp, vp, vp, i, i, vp, C.POINTER(i)]
    L.mi_rast_lift_reuse.restype = i
    L.mi_rast_lift_reuse.argtypes = [i, i, i, i, i, vp, vp, vp, vp, vp, i, vp]
    L.mi_rast_last_error.restype = C.c_char_p
    L.mi_rast_version.restype = C.c_char_p
    L.mi_rast_supported_channels.restype = i
    L.mi_rast_supported_channels.argtypes = [C.POINTER(i), i]
    L.mi_rast_get_higher_msb.restype = C.c_uint32
    L.mi_rast_get_higher_msb.argtypes = [C.c_uint32]
    for name, n in (("mi_rast_geometry_layout", 1), ("mi_rast_binning_layout", 1)):
        fn = getattr(L, name)
        fn.restype = C.c_size_t
        fn.argtypes = [i, C.POINTER(C.c_size_t)]
    L.mi_rast_image_layout.restype = C.c_size_t
    L.mi_rast_image_layout.argtypes = [i, i, C.POINTER(C.c_size_t)]
    L.mi_rast_profile_enable.restype = i
    L.mi_rast_profile_enable.argtypes = [i]
    L.mi_rast_profile_read.restype = i
    L.mi_rast_profile_read.argtypes = [C.POINTER(f)]
    u32 = C.c_uint32
    L.mi_knn_smooth_forward.restype = i
    L.mi_knn_smooth_forward.argtypes = [i, i, i, vp, u32, vp, vp, i, vp]
    L.mi_knn_smooth_backward.restype = i
    L.mi_knn_smooth_backward.argtypes = [i, i, i, vp, vp, vp, u32, vp, vp, vp, vp, i, vp]
    L.mi_knn_smooth_multi_forward.restype = i
    L.mi_knn_smooth_multi_forward.argtypes = [i, i, i, C.POINTER(i), vp, vp, i, vp, vp, i, vp]
    L.mi_knn_smooth_multi_backward.restype = i
    L.mi_knn_smooth_multi_backward.argtypes = [i, i, i, C.POINTER(i), vp, vp, vp, vp, i, vp, vp, vp, vp, vp, i, vp]
    L.mi_knn_workspace_bytes.restype = C.c_size_t
    L.mi_knn_workspace_bytes.argtypes = [i]
    L.mi_knn_build.restype = i
    L.mi_knn_build.argtypes = [i, vp, vp, C.c_size_t, vp]
    L.mi_knn_query.restype = i
    L.mi_knn_query.argtypes = [i, vp, i, vp, i, i, vp, vp, vp]
    L.mi_knn_mean_dist2.restype = i
    L.mi_knn_mean_dist2.argtypes = [i, vp, vp, C.c_size_t, vp, vp]
    L.mi_contrastive_forward.restype = i
    L.mi_contrastive_forward.argtypes = [i, i, i, vp, i, i, i, vp, i, vp, vp, vp, vp, vp, vp, vp]
    L.mi_contrastive_backward.restype = i
    L.mi_contrastive_backward.argtypes = [i, i, i, vp, i, i, i, vp, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mi_contrastive_pack_masks.restype = i
    L.mi_contrastive_pack_masks.argtypes = [i, i, i, vp, vp, vp]
    L.mi_contrastive_cover.restype = i
    L.mi_contrastive_cover.argtypes = [i, i, i, vp, vp, f, vp, vp, vp]
    L.mi_contrastive_targets.restype = i
    L.mi_contrastive_targets.argtypes = [i, i, i, vp, vp, i, vp, i, vp, vp, vp, vp, vp, vp]
    L.mi_contrastive_loss_forward.restype = i
    L.mi_contrastive_loss_forward.argtypes = [i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mi_contrastive_loss_backward.restype = i
    L.mi_contrastive_loss_backward.argtypes = [i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mi_mask_scales_workspace_bytes.restype = C.c_size_t
    L.mi_mask_scales_workspace_bytes.argtypes = [i, i, i]
    L.mi_mask_erode.restype = i
    L.mi_mask_erode.argtypes = [i, i, i, vp, i, i, vp, vp]
    L.mi_mask_erode_min_sum.restype = i
    L.mi_mask_erode_min_sum.argtypes = [i, i, i, vp, i, i, f, vp, vp]
    L.mi_mask_scales.restype = i
    L.mi_mask_scales.argtypes = [i, i, i, vp, vp, C.c_double, C.c_double, vp, C.c_size_t, vp, vp, vp]
    L.mi_mask_overlaps.restype = i
    L.mi_mask_overlaps.argtypes = [i, i, i, vp, vp, vp, vp, vp]
    L.mi_mask_boxes.restype = i
    L.mi_mask_boxes.argtypes = [i, i, i, vp, vp, vp, vp]
    L.mi_mask_nms_keep.restype = i
    L.mi_mask_nms_keep.argtypes = [i, vp, vp, vp, f, f, f, vp, vp]
    L.mi_mask_score_images.restype = i
    L.mi_mask_score_images.argtypes = [i, i, i, i, vp, vp, i, vp, vp]
    L.mi_mask_resize.restype = i
    L.mi_mask_resize.argtypes = [i, i, i, vp, i, i, f, vp, vp]
    L.mi_mask_clip_tiles.restype = i
    L.mi_mask_clip_tiles.argtypes = [i, i, i, vp, vp, vp, i, f, i, C.POINTER(f), C.POINTER(f), i, i, i, vp, vp]
    L.mi_mask_index_map.restype = i
    L.mi_mask_index_map.argtypes = [i, i, i, vp, i, vp, vp]
    L.mi_segment_scores.restype = i
    L.mi_segment_scores.argtypes = [i, i, i, i, vp, vp, vp, i, i, vp, vp]
    L.mi_segment_select.restype = i
    L.mi_segment_select.argtypes = [i, i, i, i, vp, vp, vp, i, i, f, vp, vp, vp]
    L.mi_segment_assign.restype = i
    L.mi_segment_assign.argtypes = [i, i, i, i, vp, vp, vp, i, vp, vp, vp]
    L.mi_segment_assign_block.restype = i
    L.mi_segment_assign_block.argtypes = [i]
    L.mi_photo_loss_workspace_bytes.restype = C.c_size_t
    L.mi_photo_loss_workspace_bytes.argtypes = [i, i, i]
    L.mi_photo_loss_window.restype = None
    L.mi_photo_loss_window.argtypes = [C.POINTER(f), C.POINTER(C.c_double)]
    L.mi_photo_loss_forward.restype = i
    L.mi_photo_loss_forward.argtypes = [i, i, i, i, vp, vp, C.c_double, i, vp, vp, C.c_size_t, vp, vp]
    L.mi_photo_loss_backward.restype = i
    L.mi_photo_loss_backward.argtypes = [i, i, i, i, vp, vp, vp, vp, i, f, f, vp, vp]
    pp, d = C.POINTER(C.c_void_p), C.c_double
    L.mi_train_adam_step.restype = i
    L.mi_train_adam_step.argtypes = [i, pp, pp, pp, pp, C.POINTER(C.c_size_t), C.POINTER(d), d, d, d, d, vp]
    L.mi_train_densify_stats.restype = i
    L.mi_train_densify_stats.argtypes = [i, vp, vp, vp, vp, vp, vp]
    L.mi_train_densify_workspace_bytes.restype = C.c_size_t
    L.mi_train_densify_workspace_bytes.argtypes = [i]
    L.mi_train_densify_plan.restype = i
    L.mi_train_densify_plan.argtypes = [i, vp, vp, vp, vp, d, d, d, d, i, vp, C.c_size_t, vp, vp]
    L.mi_train_densify_counts.restype = i
    L.mi_train_densify_counts.argtypes = [i, vp, C.c_size_t, C.POINTER(i), vp]
    L.mi_train_densify_apply.restype = i
    L.mi_train_densify_apply.argtypes = [i, C.POINTER(i), i, pp, pp, C.POINTER(i), C.POINTER(i), vp, vp, C.c_size_t, vp]
    L.mi_cluster_workspace_bytes.restype = C.c_size_t
    L.mi_cluster_workspace_bytes.argtypes = [i, i, i, i]
    L.mi_cluster_core_distances.restype = i
    L.mi_cluster_core_distances.argtypes = [i, i, i, vp, i, vp, vp, C.c_size_t, vp]
    L.mi_cluster_mst.restype = i
    L.mi_cluster_mst.argtypes = [i, i, i, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.mi_cluster_mst_rounds.restype = i
    L.mi_cluster_mst_rounds.argtypes = []
    L.mi_cluster_labels_host.restype = i
    L.mi_cluster_labels_host.argtypes = [i, i, vp, vp, vp, i, d, i, vp, C.POINTER(i)]
    L.mi_vote_mask_features_workspace_bytes.restype = C.c_size_t
    L.mi_vote_mask_features_workspace_bytes.argtypes = [i, i, i, i]
    L.mi_vote_mask_features.restype = i
    L.mi_vote_mask_features.argtypes = [i, i, i, i, vp, i, i, vp, vp, vp, C.c_size_t, vp, vp, vp]
    L.mi_vote_anchor_bits.restype = i
    L.mi_vote_anchor_bits.argtypes = [i, i, i, vp, vp, vp, f, vp, vp, vp]
    L.mi_vote_relevancy.restype = i
    L.mi_vote_relevancy.argtypes = [i, i, i, i, vp, i, vp, vp, i, vp, vp]
    L.mi_view_moments_workspace_bytes.restype = C.c_size_t
    L.mi_view_moments_workspace_bytes.argtypes = [i, i]
    L.mi_view_moments_block.restype = i
    L.mi_view_moments_block.argtypes = []
    L.mi_view_moments.restype = i
    L.mi_view_moments.argtypes = [i, i, i, vp, vp, i, i, vp, C.c_size_t, vp, vp, vp]
    L.mi_view_frame.restype = i
    L.mi_view_frame.argtypes = [i, i, vp, vp, vp, vp, i, vp, vp, f, i, i, vp, vp, vp, vp]
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
