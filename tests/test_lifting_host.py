"""CPU checks of the score lifting (include/mi_rast.h: mi_rast_lift, mi_rast_lift_reuse; seganygaussians_amd/lifting.py): every
refusal comes with its one message before any HIP call -- the pointers handed over are never read --, and the Python layer refuses
what it can see without a device.  No GPU."""
import ctypes

import pytest
import torch

from seganygaussians_amd import _lib
from seganygaussians_amd import lifting

FAKE = 8   # a "pointer" no refusal may read


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@_lib.RESIZE_FN
def _never(_nbytes, _user):
    raise AssertionError("a refused call asked for a buffer")


def _lift(lib, P=4, K=1, W=16, H=16, scores=FAKE, votes=FAKE, radii=FAKE, n=True, cb=_never):
    num = ctypes.c_int(-1)
    rc = lib.mi_rast_lift(cb, None, cb, None, cb, None, P, K, W, H, FAKE, FAKE, FAKE, 1.0, FAKE, None, FAKE, FAKE, 1.0, 1.0, 0,
                          scores, votes, radii, 0, 0, None, ctypes.byref(num) if n else None)
    return rc, num.value


def _reuse(lib, P=4, K=1, R=5, W=16, H=16, geom=FAKE, binning=FAKE, img=FAKE, scores=FAKE, votes=FAKE):
    return lib.mi_rast_lift_reuse(P, K, R, W, H, geom, binning, img, scores, votes, 0, None)


SIZES = "P, width and height must be positive"
CHANNELS = "lift: need 1 <= K <= 64 score channels"

LIFT_REFUSED = [
    (dict(P=0), SIZES), (dict(P=-3), SIZES), (dict(W=0), SIZES), (dict(H=-1), SIZES),
    (dict(K=0), CHANNELS), (dict(K=65), CHANNELS), (dict(K=-1), CHANNELS),
    (dict(scores=None), "lift: null scores or votes"), (dict(votes=None), "lift: null scores or votes"),
    (dict(radii=None), "null output pointer"), (dict(n=False), "null output pointer"),
    (dict(cb=_lib.RESIZE_FN()), "lift: null buffer callback"),
]
REUSE_REFUSED = [
    (dict(P=0), SIZES), (dict(W=0), SIZES), (dict(H=0), SIZES),
    (dict(K=0), CHANNELS), (dict(K=65), CHANNELS),
    (dict(scores=None), "lift: null scores or votes"), (dict(votes=None), "lift: null scores or votes"),
    (dict(R=-1), "lift: R must not be negative"),
    (dict(geom=None), "lift: null buffer"), (dict(binning=None), "lift: null buffer"), (dict(img=None), "lift: null buffer"),
]


@pytest.mark.parametrize("kw,msg", LIFT_REFUSED, ids=[f"{i}-{list(k)[0]}" for i, (k, _) in enumerate(LIFT_REFUSED)])
def test_lift_refuses_before_any_hip_call(lib, kw, msg):
    rc, num = _lift(lib, **kw)
    assert rc != 0 and _lib.last_error() == msg
    assert num in (0, -1)   # *num_rendered is cleared where it was given


@pytest.mark.parametrize("kw,msg", REUSE_REFUSED, ids=[f"{i}-{list(k)[0]}" for i, (k, _) in enumerate(REUSE_REFUSED)])
def test_lift_reuse_refuses_before_any_hip_call(lib, kw, msg):
    assert _reuse(lib, **kw) != 0 and _lib.last_error() == msg


def test_first_refusal_wins(lib):
    """One message per call, in the documented order: sizes, channels, pointers."""
    assert _lift(lib, P=0, K=0, scores=None)[0] != 0 and _lib.last_error() == SIZES
    assert _lift(lib, K=0, scores=None)[0] != 0 and _lib.last_error() == CHANNELS
    assert _reuse(lib, P=0, K=99, geom=None) != 0 and _lib.last_error() == SIZES


def test_exports_and_limit():
    assert [n for n in _lib.DECLARED["mi_rast.h"] if n.startswith("mi_rast_lift")] == ["mi_rast_lift", "mi_rast_lift_reuse"]
    assert {"mi_rast_lift", "mi_rast_lift_reuse"} <= set(_lib.ALL_EXPORTS)
    assert lifting.MAX_CHANNELS == _lib.MI_RAST_LIFT_MAX_CHANNELS == 64


class _Cam:
    FoVx = FoVy = 1.0
    image_height = image_width = 16
    world_view_transform = full_proj_transform = torch.eye(4)


def test_vote_3d_mask_rejects_mismatched_lengths():
    m, o = torch.zeros(5, 3), torch.zeros(5, 1)
    with pytest.raises(ValueError, match="2 cameras but 1 score images"):
        lifting.vote_3d_mask([_Cam(), _Cam()], [None], m, o, scales=torch.zeros(5, 3), rotations=torch.zeros(5, 4))


def test_vote_3d_mask_without_a_view_is_all_false():
    m, o = torch.zeros(5, 3), torch.zeros(5, 1)
    mask, votes = lifting.vote_3d_mask([_Cam(), _Cam()], [None, None], m, o, scales=torch.zeros(5, 3), rotations=torch.zeros(5, 4))
    assert mask.shape == votes.shape == (5, 1) and not mask.any() and (votes == 0).all()


def test_lift_scores_python_refusals():
    m, o = torch.zeros(5, 3), torch.zeros(5, 1)
    s, r, c = torch.zeros(5, 3), torch.zeros(5, 4), torch.zeros(5, 6)
    view = dict(viewmatrix=torch.eye(4), projmatrix=torch.eye(4), tanfovx=1.0, tanfovy=1.0)
    msg = "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"
    for kw in (dict(), dict(scales=s), dict(scales=s, rotations=r, cov3D_precomp=c), dict(rotations=r, cov3D_precomp=c)):
        with pytest.raises(Exception, match=msg):
            lifting.lift_scores(torch.zeros(4, 4), m, o, **kw, **view)
    with pytest.raises(ValueError, match="1 <= K <= 64"):
        lifting.lift_scores(torch.zeros(65, 4, 4), m, o, scales=s, rotations=r, **view)
    with pytest.raises(ValueError, match=r"\(K, H, W\) or \(H, W\)"):
        lifting.lift_scores(torch.zeros(4), m, o, scales=s, rotations=r, **view)
    with pytest.raises(ValueError, match="out must be"):
        lifting.lift_scores(torch.zeros(2, 4, 4), m, o, scales=s, rotations=r, out=torch.zeros(5, 3), **view)


def test_no_gaussians_needs_no_library_call():
    """P = 0 returns (0, K) votes and an empty state without touching the device."""
    e3, e1 = torch.zeros(0, 3), torch.zeros(0, 1)
    votes, st = lifting.lift_scores(torch.ones(2, 4, 6), e3, e1, scales=e3, rotations=torch.zeros(0, 4), viewmatrix=torch.eye(4),
                                    projmatrix=torch.eye(4), tanfovx=1.0, tanfovy=1.0, return_state=True)
    assert votes.shape == (0, 2) and st.num_rendered == 0 and (st.width, st.height) == (6, 4)
    assert lifting.lift_scores(torch.ones(4, 6), e3, e1, state=st).shape == (0, 1)
