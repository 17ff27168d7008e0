#!/usr/bin/env python
"""Generates tests/golden/helpers/reference_helpers.npz: inputs and outputs of the REFERENCE'S OWN Python helpers
(tests/reference_helpers.py: eval_sh, build_rotation, build_scaling_rotation, getWorld2View2, getProjectionMatrix), so that
tests/test_oracle_dense.py can pin tests/dense_ref.py's restatements of them on a machine without the reference.
The file lies in a subdirectory of its own: tests/test_golden.py takes every tests/golden/*.npz for a rasterizer case.

    python tests/golden/make_helpers_golden.py      # needs the reference sources (tests/reference_helpers.py: REF_ROOT)
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from seganygaussians_amd import scenes  # noqa: E402
from tests import reference_helpers as rh  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "reference_helpers.npz")


def main():
    h = rh.ReferenceHelpers()
    g = torch.Generator().manual_seed(0)
    q = torch.randn(64, 4, dtype=torch.float64, generator=g)
    q = q / q.norm(dim=1, keepdim=True)
    s = torch.rand(64, 3, dtype=torch.float64, generator=g) + 0.1
    sh = torch.randn(64, 16, 3, dtype=torch.float64, generator=g)
    d = torch.randn(64, 3, dtype=torch.float64, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    out = {"q": q, "s": s, "sh": sh, "dirs": d, "build_rotation": h.build_rotation(q), "build_scaling_rotation": h.build_scaling_rotation(s, q)}
    for deg in range(4):
        out[f"eval_sh{deg}"] = h.eval_sh(deg, sh, d)
    # the cameras of tests/test_oracle_dense.py: the reference's world-to-view and full projection matrices (scene/cameras.py)
    gu = h.graphics_utils
    for i, cam in enumerate((scenes.look_at_camera(64, 48, 50.0), scenes.orbit_camera(64, 48, 50.0, 0.3, 0.1))):
        fovx, fovy = 2 * math.atan(64 / 100.0), 2 * math.atan(48 / 100.0)
        proj = gu.getProjectionMatrix(znear=0.01, zfar=100.0, fovX=fovx, fovY=fovy).transpose(0, 1)
        view = torch.tensor(gu.getWorld2View2(cam.R, cam.T)).transpose(0, 1)
        out[f"cam{i}_view"] = view
        out[f"cam{i}_full"] = view.unsqueeze(0).bmm(proj.unsqueeze(0)).squeeze(0)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **{k: np.asarray(v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()})
    print("wrote", OUT)


if __name__ == "__main__":
    main()
