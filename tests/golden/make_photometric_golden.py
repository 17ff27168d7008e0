#!/usr/bin/env python
"""Generates tests/golden/photometric/photometric.npz: inputs and results of the REFERENCE'S OWN utils/loss_utils.py (l1_loss, ssim
with both size_average settings, and train_scene.py:101-102's combined loss with its gradient) in float32 and in float64, so that
tests/test_photometric_host.py can pin tests/photometric_ref.py's restatement on a machine without the reference.
The file lies in a subdirectory of its own: tests/test_golden.py takes every tests/golden/*.npz for a rasterizer case.

    python tests/golden/make_photometric_golden.py      # needs the reference sources (tests/reference_helpers.py: REF_ROOT)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import photometric_ref as ref  # noqa: E402
from tests import reference_helpers as rh  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "photometric", "photometric.npz")
LAMBDA = 0.2

# name -> (class of the target, shape, seed, what the image is)
CASES = {
    "noise_c3": ("noise", (3, 24, 40), 1, "noisy"),
    "smooth_c3": ("smooth", (3, 23, 37), 2, "noisy"),
    "constant_c1": ("constant", (1, 40, 56), 3, "noisy"),
    "zero_target_c3": ("zero", (3, 24, 31), 4, "noisy"),
    "equal_c3": ("noise", (3, 20, 33), 5, "equal"),
    "short_h_c3": ("noise", (3, 7, 40), 6, "noisy"),
    "narrow_w_c1": ("smooth", (1, 40, 9), 7, "noisy"),
    "batch2_c3": ("noise", (2, 3, 21, 30), 8, "noisy"),
}


def main():
    spec = importlib.util.spec_from_file_location("saga_reference_loss_utils", os.path.join(rh.REF_ROOT, "utils", "loss_utils.py"))
    lu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lu)
    torch.set_num_threads(1)
    out = {"lambda_dssim": np.float64(LAMBDA), "names": np.array(sorted(CASES))}
    for name, (kind, shape, seed, what) in CASES.items():
        x, g = ref.make_pair(kind, shape, seed)
        if what == "equal":
            x = g.clone()
        out[f"{name}.image"], out[f"{name}.target"] = x.numpy(), g.numpy()
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            xd, gd = x.to(dt).detach().clone().requires_grad_(True), g.to(dt)
            ll1, ss = lu.l1_loss(xd, gd), lu.ssim(xd, gd)
            loss = (1.0 - LAMBDA) * ll1 + LAMBDA * (1.0 - ss)      # train_scene.py:101-102
            loss.backward()
            out[f"{name}.{tag}.l1"], out[f"{name}.{tag}.ssim"] = ll1.detach().numpy(), ss.detach().numpy()
            out[f"{name}.{tag}.loss"], out[f"{name}.{tag}.grad"] = loss.detach().numpy(), xd.grad.numpy()
            if len(shape) == 4:
                out[f"{name}.{tag}.ssim_per_image"] = lu.ssim(xd, gd, size_average=False).detach().numpy()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
