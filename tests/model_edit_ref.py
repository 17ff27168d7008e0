"""The model cut (seganygaussians_amd/model_edit.py) restated in plain torch, the loader of its golden fixture
(tests/golden/model_edit/model_edit.npz, written by tests/golden/make_model_edit_golden.py from the reference's own methods), and
what the host and the GPU tests share: test tensors whose first column carries the original row number, and stand-ins for the
reference's two classes.  Runs anywhere."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_edit", "model_edit.npz")
CUT, ROLL_BACK, CLEAR = 0, 1, 2


class CutState:
    """Which original rows a model holds after a sequence of cuts.  level[i] - 1 is the number of cuts in force that original row i
    has survived; the rows held are those that survived all `times` of them."""

    def __init__(self, P0):
        self.level = torch.ones(P0, dtype=torch.float32)
        self.times = 0
        self.rows = torch.arange(P0)
        self.earlier = []

    def cut(self, mask):
        mask = mask.reshape(-1)
        if not bool(mask.any()):
            mask = torch.ones_like(mask)
        self.earlier.append(self.rows)
        self.rows = self.rows[mask]
        self.level[self.rows] += 1
        self.times += 1

    def roll_back(self):
        if self.earlier:
            self.level[self.rows] -= 1
            self.rows = self.earlier.pop()
            self.times -= 1

    def clear(self):
        if self.earlier:
            self.rows = self.earlier[0]
            self.earlier = []
            self.times = 0
            self.level = torch.ones_like(self.level)

    def apply(self, op, mask=None):
        {CUT: lambda: self.cut(mask), ROLL_BACK: self.roll_back, CLEAR: self.clear}[op]()


def load_cases(path=GOLDEN):
    """[{"P0", "ops": [{"op", "mask" (bool tensor, (n,) or (n, 1), or None), "rows" (int64), "level" (float32), "times", "depth"}]}]"""
    z = np.load(path)
    cases, op_at, bit_at, row_at, level_at = [], 0, 0, 0, 0
    mask_bits = np.unpackbits(z["mask_bits"])
    for P0, n_ops in zip(z["case_P0"].tolist(), z["case_ops"].tolist()):
        ops = []
        for k in range(op_at, op_at + n_ops):
            mask, n = None, int(z["mask_len"][k])
            if int(z["op"][k]) == CUT:
                mask = torch.from_numpy(mask_bits[bit_at:bit_at + n].astype(bool))
                bit_at += n
                if z["mask_column"][k]:
                    mask = mask.reshape(n, 1)
            n_rows = int(z["n_rows"][k])
            ops.append({"op": int(z["op"][k]), "mask": mask, "rows": torch.from_numpy(z["rows"][row_at:row_at + n_rows].astype(np.int64)),
                        "level": torch.from_numpy(z["level"][level_at:level_at + P0].astype(np.float32)), "times": int(z["times"][k]),
                        "depth": int(z["depth"][k])})
            row_at += n_rows
            level_at += P0
        op_at += n_ops
        cases.append({"P0": P0, "ops": ops})
    assert op_at == len(z["op"]) and row_at == len(z["rows"]) and level_at == len(z["level"])
    return cases


# ---- test tensors ------------------------------------------------------------------------------------------------------------

# int32 patterns a copy must not touch: NaNs with payloads (quiet and signalling, both signs), +-inf, -0.0, denormals
SPECIAL_BITS = [0x7FC00001, 0x7F800001, 0xFFC12345, 0xFFBFFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000]

LAYOUTS = {     # attribute -> trailing shape; sh_rest: the (degree + 1)^2 - 1 coefficients past the first
    "scene": lambda sh_rest=15: {"_xyz": (3,), "_features_dc": (1, 3), "_features_rest": (sh_rest, 3), "_opacity": (1,), "_scaling": (3,),
                                 "_rotation": (4,)},
    "feature": lambda dim=32: {"_xyz": (3,), "_point_features": (dim,), "_opacity": (1,), "_scaling": (3,), "_rotation": (4,)},
}


def tagged_tensor(P, trailing, seed, device="cpu"):
    """float32 (P, *trailing): random bits with the special patterns strewn in; the first value of row i is float(i)."""
    cols = int(np.prod(trailing)) if len(trailing) else 1
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 1 << 32, (P, cols), dtype=np.uint64).astype(np.uint32)
    where = rng.random((P, cols)) < 0.25
    bits[where] = np.asarray(SPECIAL_BITS, np.uint32)[rng.integers(0, len(SPECIAL_BITS), int(where.sum()))]
    if cols:
        bits[:, 0] = np.arange(P, dtype=np.float32).view(np.uint32)
    return torch.from_numpy(bits.view(np.int32).reshape((P,) + tuple(trailing))).view(torch.float32).to(device)


def bits_equal(a, b) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def row_ids(t):
    """The original row numbers the first column of a tagged tensor carries."""
    return t.detach().reshape(t.shape[0], -1)[:, 0].to(torch.int64).cpu()


# ---- stand-ins for the reference's two classes: the attributes its three methods work on, and methods that say they ran -----------

STAND_IN_SOURCE = {
    "scene.gaussian_model": (
        "class GaussianModel:\n"
        "    def __init__(self):\n"
        "        self.optimizer = None\n        self.segment_times = 0\n        self.calls = []\n"
        "        for n in ('xyz', 'mask', 'features_dc', 'features_rest', 'opacity', 'scaling', 'rotation'):\n"
        "            setattr(self, 'old_' + n, [])\n"
        "    def segment(self, mask=None):\n        self.calls.append('reference segment')\n"
        "    def roll_back(self):\n        self.calls.append('reference roll_back')\n"
        "    def clear_segment(self):\n        self.calls.append('reference clear_segment')\n"),
    "scene.gaussian_model_ff": (
        "class FeatureGaussianModel:\n"
        "    def __init__(self):\n"
        "        self.optimizer = None\n        self.segment_times = 0\n        self.calls = []\n"
        "        for n in ('xyz', 'point_features', 'opacity', 'scaling', 'rotation'):\n"
        "            setattr(self, 'old_' + n, [])\n"
        "    def segment(self, mask=None):\n        self.calls.append('reference segment')\n"
        "    def roll_back(self):\n        self.calls.append('reference roll_back')\n"
        "    def clear_segment(self):\n        self.calls.append('reference clear_segment')\n"
        "    def get_smoothed_point_features(self, K=16, dropout=0.5):\n        return 'reference smoothing'\n"),
}


def write_stand_ins(directory):
    """A `scene` package with the two stand-in modules under `directory` (a pathlib.Path)."""
    pkg = directory / "scene"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    for name, source in STAND_IN_SOURCE.items():
        (pkg / (name.split(".")[1] + ".py")).write_text(source)


def fill_model(model, layout, P0, seed, device, parameters=True):
    """Gives a stand-in (or any object) the tensors of `layout`, tagged, and an all-ones _mask."""
    for k, (field, trailing) in enumerate(layout.items()):
        t = tagged_tensor(P0, trailing, 100 * seed + k, device)
        setattr(model, field, torch.nn.Parameter(t, requires_grad=True) if parameters else t)
    model._mask = torch.ones((P0,), dtype=torch.float32, device=device)
    return {field: getattr(model, field).detach().clone() for field in layout}
