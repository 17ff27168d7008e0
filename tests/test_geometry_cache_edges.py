"""Frozen-geometry reuse at its edges (seganygaussians_amd/geometry_cache.py: GeometryCache; include/mi_rast.h: mi_rast_forward_reuse,
mi_rast_fingerprint).  tests/test_geometry_cache.py checks one render per backward, one step after the other; here the renders of
cached views interleave -- a miss and its hits in one loss, backwards in either order, no-grad renders between a forward and its
backward, retained graphs, gradient accumulation -- at several widths, in the three packages, with P below and above H W.

The reference of every case is the same Python program with the cache disabled (each uncached forward has buffers of its own; the
uncached path is pinned against the oracle and the reference elsewhere).  Images, masks, depths and radii must be equal bit for bit,
every gradient within 2e-5 of the largest reference element (the order of the atomic sums).  Each render of a loss weights its
outputs with a dL image of its own, so that wrongly shared or missing contributions cannot cancel.  Images have 70 tiles: every
XCD run of the blend kernels has queued tiles (xcd_runs.h: xcd_grab_runs).

The fingerprint kernel, which decides whether a cached state is reused, is checked word for word against a host restatement."""
import ctypes as C

import numpy as np
import pytest
import torch

import seganygaussians_amd
from seganygaussians_amd import _lib
from seganygaussians_amd import rasterizer as R
from seganygaussians_amd import scenes
from tests import helpers as hp
from tests.test_geometry_cache import _settings, _t

seganygaussians_amd.install_dropin()
pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
W, H = 160, 112                  # 10 x 7 tiles
P_SMALL, P_LARGE = 9000, 24000   # P <= H W: the forward pre-zeroes dL_dcolors as well; P > H W: the backward allocates it
PACKAGES = {"cf": "diff_gaussian_rasterization_contrastive_f", "sh": "diff_gaussian_rasterization",
            "depth": "diff_gaussian_rasterization_depth"}
# a log-scale spread of 0.4 (make_inputs' default: 0.6): the default leaves a tail of Gaussians covering most of the image, whose scale
# and rotation gradients differ between two UNCACHED runs of these programs by up to twice the bound (atomic order alone); at 0.4
# two uncached runs stay within a tenth of it
SCENE_KW = dict(log_scale_std=0.4)


@pytest.fixture()
def cache():
    c = R.enable_geometry_cache(8 << 30)
    c.clear()
    yield c
    R.disable_geometry_cache(drop=True)


class Scene:
    """One scene, two cameras (A, B), in one package: `cf` (contrastive_f, C-channel features), `sh` (C = 3, SH colours of degree 3)
    or `depth` (colours, a mask, the mask and depth outputs).  A program renders through `render` and differentiates as it likes;
    `run` executes it with fresh leaves, cached or not, and returns what it recorded and the leaves' gradients."""

    def __init__(self, kind="cf", C=32, P=P_SMALL, seed=71, requires=None):
        self.kind, self.C = kind, (C if kind == "cf" else 3)
        self.inp = hp.make_inputs(P, W, H, self.C, seed=seed, camera="orbit", with_shs=kind == "sh", sh_degree=3 if kind == "sh" else 0,
                                  use_mask=kind == "depth", bg="random", **SCENE_KW)
        self.mod = __import__(PACKAGES[kind])
        camB = scenes.orbit_camera(W, H, 0.85 * W, 0.35, 0.1)
        self.rs = {"A": _settings(self.mod, self.inp, DEV),
                   "B": _settings(self.mod, self.inp, DEV, cam=(camB.viewmatrix, camB.projmatrix, camB.campos))}
        self.requires = requires
        self._dl = {}

    def leaves(self):
        i = self.inp
        L = {"means3D": i.means3D, "opacities": i.opacities, "scales": i.scales, "rotations": i.rotations}
        if self.kind == "sh":
            L["shs"] = i.shs
        else:
            L["colors"] = i.colors_precomp
        if self.kind == "depth":
            L["mask"] = i.mask
            L["mask2"] = i.mask[::-1].copy()
        if self.kind == "cf":
            L["colors16"] = np.ascontiguousarray(i.colors_precomp[:, :16][::-1] * 0.5)   # another width, other values
        L = {k: _t(v, DEV) for k, v in L.items()}
        for k, v in L.items():
            v.requires_grad_(self.requires is None or k in self.requires)
        return L

    def dl(self, shape, k):
        key = (tuple(shape), k)
        if key not in self._dl:
            self._dl[key] = _t(scenes.make_grad_image(shape[0], shape[1], shape[2], seed=100 + k), DEV)
        return self._dl[key]

    def render(self, L, view="A", k=0, rs=None, colors=None, mask=None):
        """One render; returns (loss term weighted with dL images of seed k, outputs).  Records clones of the outputs."""
        rs = rs if rs is not None else self.rs[view]
        m2 = torch.zeros_like(L["means3D"], requires_grad=L["means3D"].requires_grad)
        self.means2D.append(m2)
        rast = self.mod.GaussianRasterizer(raster_settings=rs)
        kw = dict(means3D=L["means3D"], means2D=m2, opacities=L["opacities"], scales=L["scales"], rotations=L["rotations"],
                  cov3D_precomp=None)
        if self.kind == "depth":
            outs = rast(mask=L["mask"] if mask is None else mask, shs=None, colors_precomp=L["colors"], **kw)
            loss = (outs[0] * self.dl(outs[0].shape, k)).sum() + (outs[1] * self.dl(outs[1].shape, 50 + k)).sum()
        elif self.kind == "sh":
            outs = rast(shs=L["shs"], colors_precomp=None, **kw)
            loss = (outs[0] * self.dl(outs[0].shape, k)).sum()
        else:
            outs = rast(shs=None, colors_precomp=L["colors"] if colors is None else colors, **kw)
            loss = (outs[0] * self.dl(outs[0].shape, k)).sum()
        for j, o in enumerate(outs):
            self.rec.append(("exact", f"render {len(self.means2D) - 1} output {j}", o.detach().clone()))
        return loss, outs

    def snap(self, L, what):
        """Records the gradients as they are now (between two backwards of a program)."""
        for name, v in list(L.items()) + [(f"means2D[{j}]", m) for j, m in enumerate(self.means2D)]:
            if v.grad is not None:
                self.rec.append(("grad", f"{what}: {name}", v.grad.clone()))

    def run(self, prog, cached):
        if cached:
            R.enable_geometry_cache(8 << 30).clear()
        else:
            R.disable_geometry_cache()
        self.rec, self.means2D = [], []
        L = self.leaves()
        prog(self, L)
        self.snap(L, "end")
        torch.cuda.synchronize()
        stats = R.geometry_cache().stats() if cached else None
        return self.rec, stats


def _close(a, b, what):
    scale = float(b.abs().max()) if b.numel() else 0.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    assert err <= 2e-5 * max(scale, 1e-30), f"{what} differs beyond atomic order: {err:.3g} vs max {scale:.3g}"


def _check(sc, prog, hits, misses):
    ref, _ = sc.run(prog, cached=False)
    got, stats = sc.run(prog, cached=True)
    assert (stats["hits"], stats["misses"]) == (hits, misses), stats
    assert [(k, n, tuple(t.shape)) for k, n, t in got] == [(k, n, tuple(t.shape)) for k, n, t in ref]
    for (kind, name, a), (_, _, b) in zip(got, ref):
        if kind == "exact":
            assert torch.equal(a, b), f"{name} differs"
        else:
            _close(a, b, name)
    assert any(kind == "grad" and float(t.abs().max()) > 0 for kind, _, t in ref), "the program produced no gradient"


# ---- interleavings ---------------------------------------------------------------------------------------------------------------
def miss_hit_one_backward(sc, L):                      # 1: the miss's backward runs after the hit's, on the shared scratch
    (sc.render(L, "A", 0)[0] + sc.render(L, "A", 1)[0]).backward()


def hit_hit_one_backward(sc, L):                       # 2
    sc.render(L, "A", 0)[0].backward()
    sc.snap(L, "after the miss")
    (sc.render(L, "A", 1)[0] + sc.render(L, "A", 2)[0]).backward()


def miss_hit_backward_hit_then_miss(sc, L):            # 2
    l0, _ = sc.render(L, "A", 0)
    l1, _ = sc.render(L, "A", 1)
    l1.backward()
    sc.snap(L, "after the hit's backward")
    l0.backward()


def no_grad_hit_between(sc, L):                        # 3: render.py-style evaluation between a forward and its backward
    l0, _ = sc.render(L, "A", 0)
    with torch.no_grad():
        sc.render(L, "A", 1)
    l0.backward()


def two_views_interleaved(sc, L):                      # 4
    sum(sc.render(L, v, k)[0] for k, v in enumerate("ABAB")).backward()


def accumulate_two_steps(sc, L):                       # 5: .grad not cleared between the steps
    sc.render(L, "A", 0)[0].backward()
    sc.render(L, "A", 1)[0].backward()


def hit_retained_graph(sc, L):                         # 6
    sc.render(L, "A", 0)[0].backward()
    l1, _ = sc.render(L, "A", 1)
    l1.backward(retain_graph=True)
    sc.snap(L, "after the first backward of the hit")
    l1.backward()


INTERLEAVINGS = {f.__name__: (f, h, m) for f, h, m in (
    (miss_hit_one_backward, 1, 1), (hit_hit_one_backward, 2, 1), (miss_hit_backward_hit_then_miss, 1, 1),
    (no_grad_hit_between, 1, 1), (two_views_interleaved, 2, 2), (accumulate_two_steps, 1, 1), (hit_retained_graph, 1, 1))}


@pytest.mark.parametrize("P", [P_SMALL, P_LARGE])
@pytest.mark.parametrize("name", list(INTERLEAVINGS))
def test_interleavings_equal_uncached(cache, name, P):
    prog, hits, misses = INTERLEAVINGS[name]
    _check(Scene("cf", 32, P), prog, hits, misses)


@pytest.mark.parametrize("P", [P_SMALL, P_LARGE])
@pytest.mark.parametrize("pkg", ["cf16", "cf48", "cf64", "sh", "depth"])
@pytest.mark.parametrize("name", ["miss_hit_one_backward", "two_views_interleaved"])
def test_widths_and_packages(cache, name, pkg, P):
    prog, hits, misses = INTERLEAVINGS[name]
    sc = Scene("cf", int(pkg[2:]), P) if pkg.startswith("cf") else Scene(pkg, P=P)
    _check(sc, prog, hits, misses)


@pytest.mark.parametrize("P", [P_SMALL, P_LARGE])
@pytest.mark.parametrize("form", ["automatic", "opt_in"])
def test_features_only_backward_miss_and_hit(cache, form, P):   # 7
    sc = Scene("cf", 32, P, requires=("colors",) if form == "automatic" else None)
    prev = R.enable_features_only_backward(form == "opt_in")
    try:
        _check(sc, miss_hit_one_backward, 1, 1)
        if form == "opt_in":
            got, _ = sc.run(miss_hit_one_backward, cached=True)
            assert {n.split(": ")[1] for k, n, _ in got if k == "grad"} == {"colors"}
    finally:
        R.enable_features_only_backward(prev)


# ---- what the key leaves out, what it holds --------------------------------------------------------------------------------------
def test_key_leaves_out_bg_mask_and_width(cache):
    """bg, the DEPTH mask and the channel width are not in the key: a hit must still render what an uncached call renders."""
    sc = Scene("cf", 32)
    bg2 = sc.rs["A"]._replace(bg=_t(np.linspace(0.1, 0.9, 32), DEV))
    _check(sc, lambda s, L: (s.render(L, "A", 0)[0] + s.render(L, rs=bg2, k=1)[0]).backward(), 1, 1)
    rs16 = sc.rs["A"]._replace(bg=_t(np.linspace(0.2, 0.7, 16), DEV))
    _check(sc, lambda s, L: (s.render(L, "A", 0)[0] + s.render(L, rs=rs16, k=1, colors=L["colors16"])[0]).backward(), 1, 1)
    _check(sc, lambda s, L: (s.render(L, rs=rs16, k=0, colors=L["colors16"])[0] + s.render(L, "A", 1)[0]).backward(), 1, 1)
    sd = Scene("depth")
    _check(sd, lambda s, L: (s.render(L, "A", 0)[0] + s.render(L, "A", 1, mask=L["mask2"])[0]).backward(), 1, 1)


@pytest.mark.parametrize("change", ["scale_modifier", "sh_degree", "tanfovx", "image_size"])
def test_key_holds_settings(cache, change):
    sc = Scene("sh" if change == "sh_degree" else "cf", 32)
    rs = sc.rs["A"]
    rs2 = {"scale_modifier": lambda: rs._replace(scale_modifier=1.15), "sh_degree": lambda: rs._replace(sh_degree=2),
           "tanfovx": lambda: rs._replace(tanfovx=rs.tanfovx * 1.05),
           "image_size": lambda: rs._replace(image_width=W + 16, image_height=H - 16)}[change]()
    _check(sc, lambda s, L: (s.render(L, "A", 0)[0] + s.render(L, rs=rs2, k=1)[0]).backward(), 0, 2)


@pytest.mark.parametrize("rebinds", [1, 2])
def test_rebinding_data_misses(cache, rebinds):
    """`p.data = new` keeps the tensor object and its version; twice without a render in between, the caching allocator can hand
    the first address back."""
    def prog(s, L):
        s.render(L, "A", 0)[0].backward()
        for _ in range(rebinds):
            L["means3D"].data = L["means3D"].data + 0.01
        s.render(L, "A", 1)[0].backward()
    sc = Scene("cf", 32)
    _check(sc, prog, 0, 2)
    got, _ = sc.run(prog, cached=True)
    images = [t for k, n, t in got if n.endswith("output 0")]
    assert not torch.equal(images[0], images[1])


def test_radii_changed_in_place_do_not_reach_later_hits(cache):
    def prog(s, L):
        l, o = s.render(L, "A", 0)        # miss
        l.backward()
        with torch.no_grad():
            o[1].zero_()
        l, o = s.render(L, "A", 1)        # hit
        l.backward()
        with torch.no_grad():
            o[1].add_(3)
        s.render(L, "A", 2)[0].backward()   # hit: reads the cached radii, so does its backward
    _check(Scene("cf", 32), prog, 2, 1)


# ---- validation before any fingerprint -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["cpu_rotations", "f16_scales"])
def test_bad_inputs_raise_as_uncached(cache, monkeypatch, bad):
    """The cached path refuses what the uncached one refuses, with its message, before a kernel sees a host pointer or a tensor of
    another type.  The wrapper checks in Python: not even the unfixed code lets a host pointer reach the GPU here."""
    inp = hp.make_inputs(4001, W, H, 32, seed=72)   # odd P: a float16 (P, 3) is 2 (mod 4) bytes long
    import diff_gaussian_rasterization_contrastive_f as mod
    g = {k: _t(getattr(inp, k), DEV) for k in ("means3D", "colors_precomp", "opacities", "scales", "rotations")}
    if bad == "cpu_rotations":
        g["rotations"] = g["rotations"].cpu()
    else:
        g["scales"] = g["scales"].half()
    rast = mod.GaussianRasterizer(raster_settings=_settings(mod, inp, DEV))

    def render():
        rast(means3D=g["means3D"], means2D=torch.zeros_like(g["means3D"]), shs=None, colors_precomp=g["colors_precomp"],
             opacities=g["opacities"], scales=g["scales"], rotations=g["rotations"], cov3D_precomp=None)
    R.disable_geometry_cache()
    with pytest.raises(RuntimeError) as plain:
        render()
    c = R.enable_geometry_cache(8 << 30)
    real = c.fingerprints

    def checked(tensors, dev):
        for t in tensors:
            if t is not None and t.numel() != 0:   # (empty tensors are never read)
                assert t.is_cuda and t.dtype == torch.float32, f"a {t.dtype} tensor on {t.device} reached the fingerprint kernel"
        return real(tensors, dev)
    monkeypatch.setattr(c, "fingerprints", checked)
    with pytest.raises(RuntimeError) as cached:
        render()
    assert str(cached.value) == str(plain.value)


# ---- the fingerprint against a host restatement of fingerprint_kernel (csrc/fingerprint.h) -------------------------------------------
def _fp_ref(w):
    """sum over i of fmix32(w[i] ^ (u32(i) * 0x9E3779B1 + u32(i >> 32))) * 0x9E3779B97F4A7C15 + i, mod 2^64."""
    w = np.asarray(w, np.uint32)
    i = np.arange(w.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = w ^ ((i & np.uint64(0xFFFFFFFF)).astype(np.uint32) * np.uint32(0x9E3779B1) + (i >> np.uint64(32)).astype(np.uint32))
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x85EBCA6B)
        x ^= x >> np.uint32(13)
        x *= np.uint32(0xC2B2AE35)
        x ^= x >> np.uint32(16)
        return int((x.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + i).sum(dtype=np.uint64))


def _fp_call(ptrs, nbytes):
    n = len(ptrs)
    out = (C.c_uint64 * max(n, 1))()
    rc = _lib.load().mi_rast_fingerprint(n, (C.c_void_p * max(n, 1))(*ptrs), (C.c_size_t * max(n, 1))(*nbytes), out,
                                         torch.cuda.current_stream(DEV).cuda_stream)
    return rc, list(out)[:n]


def _fp(*ts):
    rc, out = _fp_call([t.data_ptr() for t in ts], [t.numel() * t.element_size() for t in ts])
    assert rc == 0, _lib.last_error()
    return out


def _words(n, seed):
    w = np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint32)
    return w, torch.from_numpy(w.view(np.int32)).to(DEV)


def test_fingerprint_restatement_is_the_formula():
    w = np.array([0, 1, 0xFFFFFFFF], np.uint32)   # the restatement's arithmetic, done by hand in Python integers
    M32, M64 = (1 << 32) - 1, (1 << 64) - 1
    want = 0
    for i, v in enumerate(w.tolist()):
        x = v ^ ((i * 0x9E3779B1 + (i >> 32)) & M32)
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & M32
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & M32
        x ^= x >> 16
        want = (want + x * 0x9E3779B97F4A7C15 + i) & M64
    assert _fp_ref(w) == want


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 32767, 32768, 32769, 65537, 1_000_003])
def test_fingerprint_equals_host_restatement(n):
    w, t = _words(n, seed=n)
    assert _fp(t) == [_fp_ref(w)]


def test_fingerprint_of_an_offset_view_and_of_signed_zeros():
    w, t = _words(40000, seed=5)
    v = t[1:]
    assert v.data_ptr() - t.data_ptr() == 4
    assert _fp(v) == [_fp_ref(w[1:])]
    z = torch.zeros(1000, device=DEV)
    assert _fp(z) == [_fp_ref(np.zeros(1000, np.uint32))]
    assert _fp(z) != _fp(-z)
    assert _fp(-z) == [_fp_ref(np.full(1000, 0x80000000, np.uint32))]


def test_fingerprint_of_several_arrays_equals_single_calls():
    arrays = [_words(n, seed=10 + n)[1] for n in (1, 257, 32768, 32769, 5, 65537, 100, 3)]
    single = [_fp(t)[0] for t in arrays]
    for n in range(1, 9):
        assert _fp(*arrays[:n]) == single[:n]


def test_fingerprint_refuses():
    t = torch.zeros(64, device=DEV)
    rc, _ = _fp_call([t.data_ptr()] * 9, [256] * 9)
    assert rc != 0 and "at most 8 arrays" in _lib.last_error()
    rc, _ = _fp_call([t.data_ptr()], [4 * 10 + 2])
    assert rc != 0 and "arrays of 4-byte words" in _lib.last_error()
