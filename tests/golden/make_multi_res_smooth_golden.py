#!/usr/bin/env python
"""Generates tests/golden/multi_res_smooth/multi_res_smooth.npz: inputs and results of the REFERENCE'S OWN
FeatureGaussianModel.get_multi_resolution_smoothed_point_features (scene/gaussian_model_ff.py:366-400), called in float64 on the
CPU on a stub object that carries what the method reads (get_xyz, _point_features, multi_res_feature_smooth_map), with an
exhaustive-search stand-in for pytorch3d.ops.knn_points.  P = 300, C = 32, default rates and Ks, once without weights and once
with (P, 3) softmax weights; the subset draws are the method's own `torch.rand(P) < r` after torch.manual_seed(SEED).
tests/test_multi_res_smooth_host.py pins tests/multi_res_smooth_ref.py's restatement to it on a machine without the reference.
The file lies in a subdirectory of its own: tests/test_golden.py takes every tests/golden/*.npz for a rasterizer case.

    python tests/golden/make_multi_res_smooth_golden.py      # needs the reference sources (tests/reference_helpers.py: REF_ROOT)
"""
import collections
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import reference_helpers as rh  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "multi_res_smooth", "multi_res_smooth.npz")
P, C, SEED = 300, 32, 2024
RATES, KS = (0.1, 0.5, 1.5), (4, 4, 16)


def knn_points(p1, p2, K=1, **_):
    """pytorch3d.ops.knn_points for one cloud, by exhaustive search: .idx (1, N, K), nearest first."""
    d = torch.cdist(p1[0].double(), p2[0].double())
    return collections.namedtuple("_KNN", "dists idx knn")(None, d.topk(K, dim=1, largest=False).indices[None], None)


def reference_class():
    """scene/gaussian_model_ff.py executed where it lies, with stand-ins for the packages it imports but this method does not use
    (plyfile, simple_knn) and for pytorch3d.ops; `utils.*` are the reference's own modules."""
    stubs = {"pytorch3d": types.ModuleType("pytorch3d"), "pytorch3d.ops": types.ModuleType("pytorch3d.ops"),
             "plyfile": types.ModuleType("plyfile"), "simple_knn": types.ModuleType("simple_knn"),
             "simple_knn._C": types.ModuleType("simple_knn._C")}
    stubs["pytorch3d"].ops = stubs["pytorch3d.ops"]
    stubs["pytorch3d.ops"].knn_points = knn_points
    stubs["plyfile"].PlyData = stubs["plyfile"].PlyElement = type("Unavailable", (), {})
    stubs["simple_knn"]._C = stubs["simple_knn._C"]
    stubs["simple_knn._C"].distCUDA2 = None
    sys.modules.update(stubs)
    sys.path.insert(0, rh.REF_ROOT)     # utils.general_utils, utils.system_utils, utils.sh_utils, utils.graphics_utils
    spec = importlib.util.spec_from_file_location("saga_reference_gaussian_model_ff", os.path.join(rh.REF_ROOT, "scene", "gaussian_model_ff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.FeatureGaussianModel


def main():
    method = reference_class().get_multi_resolution_smoothed_point_features
    torch.set_num_threads(1)
    g = torch.Generator().manual_seed(SEED)
    xyz = torch.randn(P, 3, generator=g)
    F = torch.randn(P, C, generator=g) * (0.1 + 2.9 * torch.rand(P, 1, generator=g))
    weights = torch.softmax(torch.randn(P, len(KS), generator=g), dim=1)
    grad_out = torch.randn(P, C, generator=g)

    pc = types.SimpleNamespace(get_xyz=xyz, _point_features=F.double().requires_grad_(True), multi_res_feature_smooth_map=[])
    torch.manual_seed(SEED)
    out = {"xyz": xyz.numpy(), "features": F.numpy(), "weights": weights.numpy(), "grad_out": grad_out.numpy(),
           "rates": np.array(RATES), "Ks": np.array(KS)}
    for tag, w in (("none", None), ("weighted", weights.double().requires_grad_(True))):
        pc._point_features.grad = None
        ret = method(pc, RATES, KS, w)          # the second call finds the maps of the first: one set of maps for both
        ret.backward(grad_out.double())
        out[f"{tag}.out"], out[f"{tag}.dF"] = ret.detach().numpy(), pc._point_features.grad.numpy().copy()
        if w is not None:
            out[f"{tag}.dw"] = w.grad.numpy()
    assert len(pc.multi_res_feature_smooth_map) == len(KS)
    for l, mrf in enumerate(pc.multi_res_feature_smooth_map):
        assert (mrf["rate"], mrf["K"]) == (RATES[l], KS[l])
        out[f"level{l}.point_mask"], out[f"level{l}.m"] = mrf["point_mask"].numpy(), mrf["m"].numpy().astype(np.int32)
    out["seed"] = np.int64(SEED)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
