"""MI355X-native differentiable Gaussian-splatting (feature) rasterizer -- the one hot path of
Jumpat/SegAnyGAussians, behind the reference's Python extension API.

    from seganygaussians_amd import install_dropin
    install_dropin()          # makes diff_gaussian_rasterization{,_contrastive_f,_depth} importable
    from diff_gaussian_rasterization_contrastive_f import GaussianRasterizationSettings, GaussianRasterizer
"""
import os
import sys

__version__ = "0.1.0"

DROPIN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin")
CLUSTERING_DROPIN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin_clustering")


def install_dropin(fuse_smoothing: bool = False, fuse_training_step: bool = False, fuse_clustering: bool = False) -> str:
    """Puts the drop-in packages (same import names as the reference's pip-installed submodules,
    environment.yml:18-21) at the FRONT of sys.path.

    fuse_smoothing=True (opt-in) additionally rebinds `FeatureGaussianModel.get_smoothed_point_features`
    (scene/gaussian_model_ff.py:338-364) to the fused HIP gather kernels (knn_smooth.py, include/mi_knn_smooth.h): at once
    if `scene.gaussian_model_ff` is already imported, otherwise right after it is imported.  Same signature, same column
    draw from the CPU generator, same values and gradients; the reference's own PyTorch expression is no longer executed.
    `FeatureGaussianModel.get_multi_resolution_smoothed_point_features` (:366-400, the renderer's smooth_type='multi_res') is
    rebound with it: same state and subset draws, gradients for the features and for `smooth_weights`; outside the fused
    kernels' limits (more than 4 levels, sum(Ks) > 32, a subset smaller than its K, a width other than 32 / 64) the
    reference's own method runs.

    fuse_training_step=True (opt-in) patches `scene.gaussian_model.GaussianModel` in the same manner (training_step.py, DESIGN.md
    section 18): `training_setup` swaps the optimizer it built for a FusedAdam over the same groups, and
    `add_densification_stats` and `densify_and_prune` run the HIP kernels.  The originals stay reachable as `_reference_*`.

    fuse_clustering=True (opt-in) additionally puts a second directory at the front of sys.path, whose only package is `hdbscan`
    (clustering.py): `from hdbscan import HDBSCAN` then resolves to the HIP implementation, euclidean only.
    It is a directory of its own so that a plain install_dropin() never shadows an installed `hdbscan`."""
    if DROPIN_DIR not in sys.path:
        sys.path.insert(0, DROPIN_DIR)
    if fuse_smoothing:
        _patch_now_or_on_import(_FF_MODULE, "FeatureGaussianModel", patch_feature_model)
    if fuse_training_step:
        _patch_now_or_on_import(_GM_MODULE, "GaussianModel", patch_gaussian_model)
    if fuse_clustering and CLUSTERING_DROPIN_DIR not in sys.path:
        sys.path.insert(0, CLUSTERING_DROPIN_DIR)
    return DROPIN_DIR


def install_model_edit() -> None:
    """Opt-in, a call of its own next to install_dropin: rebinds `segment`, `roll_back` and `clear_segment` of both
    `scene.gaussian_model.GaussianModel` and `scene.gaussian_model_ff.FeatureGaussianModel` to the HIP cut (model_edit.py, DESIGN.md
    section 26), at once for a module that is already imported, otherwise right after its import: same attributes maintained
    (`old_*`, `_mask`, `segment_times`), one host read per cut.  The originals stay reachable as `_reference_*`; a model with an
    optimizer runs the reference's own `segment`.  Idempotent; combines with install_dropin(fuse_smoothing=True) and
    (fuse_training_step=True), which patch the same two modules, in any order."""
    _patch_now_or_on_import(_GM_MODULE, "GaussianModel", patch_model_edit)
    _patch_now_or_on_import(_FF_MODULE, "FeatureGaussianModel", patch_model_edit)


# the viewer frame (viewer.py), resolved on first use so that importing the package stays free of torch
_VIEWER_NAMES = ("ViewerFrame", "feature_covariance", "feature_pca_basis", "gui_pca_sample", "prompt_features", "viewer_frame")
__all__ = ["install_dropin", "install_model_edit", "patch_feature_model", "patch_gaussian_model", "patch_model_edit"] + list(_VIEWER_NAMES)


def __getattr__(name):
    if name in _VIEWER_NAMES:
        from . import viewer
        return getattr(viewer, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


_FF_MODULE = "scene.gaussian_model_ff"
_GM_MODULE = "scene.gaussian_model"


def _patch_now_or_on_import(module_name: str, class_name: str, patch) -> None:
    mod = sys.modules.get(module_name)
    if mod is not None and hasattr(mod, class_name):
        patch(getattr(mod, class_name))
        return
    # one finder per module name, however many patches wait for that module and however often each is asked for
    finder = next((f for f in sys.meta_path if isinstance(f, _PatchOnImport) and f.module_name == module_name), None)
    if finder is None:
        sys.meta_path.insert(0, _PatchOnImport(module_name, class_name, patch))
    elif (class_name, patch) not in finder.patches:
        finder.patches.append((class_name, patch))


def patch_feature_model(cls) -> None:
    """Rebinds cls.get_smoothed_point_features and, where the class has one, cls.get_multi_resolution_smoothed_point_features
    (the reference's FeatureGaussianModel) to the fused HIP paths; idempotent.  The originals stay reachable as
    cls._reference_get_smoothed_point_features and cls._reference_get_multi_resolution_smoothed_point_features."""
    if getattr(cls, "_mi_fused_smoothing", False):
        return
    from .knn_smooth import fused_get_multi_resolution_smoothed_point_features, fused_get_smoothed_point_features
    cls._reference_get_smoothed_point_features = cls.get_smoothed_point_features
    cls.get_smoothed_point_features = fused_get_smoothed_point_features
    multi_res = getattr(cls, "get_multi_resolution_smoothed_point_features", None)
    if multi_res is not None and multi_res is not fused_get_multi_resolution_smoothed_point_features:
        cls._reference_get_multi_resolution_smoothed_point_features = cls.get_multi_resolution_smoothed_point_features
        cls.get_multi_resolution_smoothed_point_features = fused_get_multi_resolution_smoothed_point_features
    cls._mi_fused_smoothing = True


def patch_gaussian_model(cls) -> None:
    """Rebinds training_setup, add_densification_stats and densify_and_prune of cls (the reference's GaussianModel) to the fused
    training step; idempotent.  The originals stay reachable as cls._reference_<name>."""
    if getattr(cls, "_mi_fused_training_step", False):
        return
    from . import training_step as ts
    for name, fn in (("training_setup", ts.fused_training_setup), ("add_densification_stats", ts.fused_add_densification_stats),
                     ("densify_and_prune", ts.fused_densify_and_prune)):
        setattr(cls, "_reference_" + name, getattr(cls, name))
        setattr(cls, name, fn)
    cls._mi_fused_training_step = True


def patch_model_edit(cls) -> None:
    """Rebinds segment, roll_back and clear_segment of cls (the reference's GaussianModel or FeatureGaussianModel) to the HIP cut
    (model_edit.py); idempotent.  The originals stay reachable as cls._reference_<name>."""
    if vars(cls).get("_mi_fused_model_edit", False):      # of cls itself: the patch serves two classes
        return
    from . import model_edit as me
    for name, fn in (("segment", me.fused_segment), ("roll_back", me.fused_roll_back), ("clear_segment", me.fused_clear_segment)):
        setattr(cls, "_reference_" + name, getattr(cls, name))
        setattr(cls, name, fn)
    cls._mi_fused_model_edit = True


class _PatchOnImport:
    """sys.meta_path finder: lets the normal machinery find `module_name`, then calls patch(module.<class name>) for every
    (class name, patch) pair of `patches` once the module has been executed."""

    def __init__(self, module_name: str = _FF_MODULE, class_name: str = "FeatureGaussianModel", patch=patch_feature_model):
        self.module_name, self.patches = module_name, [(class_name, patch)]

    def find_spec(self, name, path=None, target=None):
        if name != self.module_name:
            return None
        import importlib.util
        sys.meta_path.remove(self)
        try:
            spec = importlib.util.find_spec(name)
        finally:
            sys.meta_path.insert(0, self)
        if spec is None or spec.loader is None or not hasattr(spec.loader, "exec_module"):
            return spec
        inner = spec.loader.exec_module

        def exec_module(module, _inner=inner):
            _inner(module)
            for class_name, patch in self.patches:
                if hasattr(module, class_name):
                    patch(getattr(module, class_name))
            if self in sys.meta_path:
                sys.meta_path.remove(self)

        spec.loader.exec_module = exec_module
        return spec
