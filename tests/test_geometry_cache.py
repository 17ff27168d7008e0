"""Frozen-geometry reuse (seganygaussians_amd/geometry_cache.py: GeometryCache; include/mi_rast.h: mi_rast_forward_reuse,
mi_rast_fingerprint): a forward of the same geometry from the same camera runs the blend stage alone over what the first visit
left.  The opt-in must change nothing: images, radii and every gradient bit for bit those of an uncached run (the atomic sums of
the backward: up to their order), whatever tensors carry the geometry -- the same objects again (bench.py), or activation outputs
recomputed per call (the reference's renderer, gaussian_renderer/__init__.py:337-348) -- and ANY change of a geometry or camera
tensor must miss."""
import numpy as np
import pytest
import torch

import seganygaussians_amd
from seganygaussians_amd import rasterizer as R
from seganygaussians_amd import scenes
from tests import helpers as hp

seganygaussians_amd.install_dropin()
pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(dev)


def _settings(mod, inp, dev, cam=None):
    vm, pm, cp = (inp.viewmatrix, inp.projmatrix, inp.campos) if cam is None else cam
    return mod.GaussianRasterizationSettings(
        image_height=inp.image_height, image_width=inp.image_width, tanfovx=inp.tanfovx, tanfovy=inp.tanfovy,
        bg=_t(inp.bg, dev), scale_modifier=inp.scale_modifier, viewmatrix=_t(vm, dev), projmatrix=_t(pm, dev),
        sh_degree=inp.sh_degree, campos=_t(cp, dev), prefiltered=False, debug=False)


@pytest.fixture()
def cache():
    c = R.enable_geometry_cache(8 << 30)
    c.clear()
    yield c
    R.disable_geometry_cache(drop=True)


def _step(rast, means3D, feats, opac, scales, rots, dL):
    for l in (means3D, feats, opac, scales, rots):
        l.grad = None
    means2D = torch.zeros_like(means3D, requires_grad=True)
    color, radii = rast(means3D=means3D, means2D=means2D, shs=None, colors_precomp=feats, opacities=opac, scales=scales,
                        rotations=rots, cov3D_precomp=None)
    color.backward(dL)
    return (color.detach().clone(), radii.clone(), feats.grad.clone(), means3D.grad.clone(), opac.grad.clone(), scales.grad.clone(),
            rots.grad.clone(), means2D.grad.clone())


def _same(a, b, what):
    assert torch.equal(a[0], b[0]), f"{what}: image differs"
    assert torch.equal(a[1], b[1]), f"{what}: radii differ"
    for x, y, name in zip(a[2:], b[2:], ("dL_dfeatures", "dL_dmeans3D", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dmeans2D")):
        # float atomics: equal up to the order of the sums
        scale = float(y.abs().max())
        assert float((x - y).abs().max()) <= 2e-5 * max(scale, 1e-30), f"{what}: {name} differs beyond atomic order"


def test_cached_equals_uncached_and_changes_miss(cache):
    import diff_gaussian_rasterization_contrastive_f as mod
    dev = torch.device("cuda:0")
    inp = hp.make_inputs(20000, 320, 208, 32, seed=61, camera="orbit")
    leaf = lambda a: _t(a, dev).requires_grad_(True)
    means3D, feats, opac, scales, rots = leaf(inp.means3D), leaf(inp.colors_precomp), leaf(inp.opacities), leaf(inp.scales), leaf(inp.rotations)
    dL = _t(scenes.make_grad_image(32, 208, 320, seed=3), dev)
    rast = mod.GaussianRasterizer(raster_settings=_settings(mod, inp, dev))
    R.disable_geometry_cache()
    plain = _step(rast, means3D, feats, opac, scales, rots, dL)
    c = R.enable_geometry_cache(8 << 30)
    c.clear()
    first = _step(rast, means3D, feats, opac, scales, rots, dL)           # first visit: a miss that fills the cache
    assert c.stats()["misses"] == 1 and c.stats()["hits"] == 0 and c.stats()["views"] == 1
    again = _step(rast, means3D, feats, opac, scales, rots, dL)           # same tensor objects: a hit without a fingerprint kernel
    assert c.stats()["hits"] == 1
    _same(first, plain, "first visit")
    _same(again, plain, "cached visit")
    # other features, same geometry: still a hit, and equal to an uncached run on those features
    with torch.no_grad():
        feats.mul_(0.5).add_(0.25)
    hit2 = _step(rast, means3D, feats, opac, scales, rots, dL)
    assert c.stats()["hits"] == 2
    R.disable_geometry_cache()
    plain2 = _step(rast, means3D, feats, opac, scales, rots, dL)
    _same(hit2, plain2, "cached visit with new features")
    R.enable_geometry_cache(8 << 30)
    # an in-place change of a geometry tensor: a miss, and the render is the moved geometry's
    with torch.no_grad():
        means3D.add_(0.01)
    moved = _step(rast, means3D, feats, opac, scales, rots, dL)
    assert c.stats()["misses"] == 2 and c.stats()["views"] == 2
    R.disable_geometry_cache()
    plain3 = _step(rast, means3D, feats, opac, scales, rots, dL)
    _same(moved, plain3, "after means3D.add_")
    assert not torch.equal(moved[0], plain2[0])
    R.enable_geometry_cache(8 << 30)
    # another camera: a miss; back to the first camera (new tensor objects holding the same matrices): a hit by content
    vm2 = np.array(inp.viewmatrix, np.float32).copy()
    vm2[3, 0] += 0.05
    rast2 = mod.GaussianRasterizer(raster_settings=_settings(mod, inp, dev, cam=(vm2, inp.projmatrix, inp.campos)))
    _step(rast2, means3D, feats, opac, scales, rots, dL)
    assert c.stats()["misses"] == 3
    rast3 = mod.GaussianRasterizer(raster_settings=_settings(mod, inp, dev))
    back = _step(rast3, means3D, feats, opac, scales, rots, dL)
    assert c.stats()["hits"] == 3
    _same(back, plain3, "same camera in new tensors")
    assert c.stats()["bytes_cached"] > 0


def test_activation_outputs_hit_by_content(cache):
    """The reference's renderer passes exp(_scaling), normalize(_rotation), sigmoid(_opacity): new tensors every call."""
    import diff_gaussian_rasterization_contrastive_f as mod
    dev = torch.device("cuda:0")
    inp = hp.make_inputs(12000, 256, 160, 32, seed=62, camera="orbit")
    xyz = _t(inp.means3D, dev)
    log_s, raw_r = _t(np.log(inp.scales), dev), _t(inp.rotations * 1.7, dev)
    raw_o = torch.logit(_t(inp.opacities, dev).clamp(1e-4, 1 - 1e-4))
    feats = _t(inp.colors_precomp, dev).requires_grad_(True)
    rast = mod.GaussianRasterizer(raster_settings=_settings(mod, inp, dev))

    def render():
        return rast(means3D=xyz, means2D=torch.zeros_like(xyz), shs=None, colors_precomp=feats, opacities=torch.sigmoid(raw_o),
                    scales=torch.exp(log_s), rotations=torch.nn.functional.normalize(raw_r), cov3D_precomp=None)[0]
    a = render()
    b = render()
    assert cache.stats() == {**cache.stats(), "hits": 1, "misses": 1}
    assert torch.equal(a, b)
    with torch.no_grad():
        log_s[5] += 0.3           # one Gaussian's scale: the fingerprint of exp(log_s) changes
    c3 = render()
    assert cache.stats()["misses"] == 2
    assert not torch.equal(c3, a)


def test_lru_eviction_and_modes_that_bypass(cache):
    import diff_gaussian_rasterization_contrastive_f as mod
    dev = torch.device("cuda:0")
    inp = hp.make_inputs(3000, 128, 96, 32, seed=63)
    g = [_t(x, dev) for x in (inp.means3D, inp.colors_precomp, inp.opacities, inp.scales, inp.rotations)]
    cache.max_bytes = 1   # room for one view only (the newest is always kept)
    for k in range(3):
        vm = np.array(inp.viewmatrix, np.float32).copy()
        vm[3, 0] += 0.01 * k
        rast = mod.GaussianRasterizer(raster_settings=_settings(mod, inp, dev, cam=(vm, inp.projmatrix, inp.campos)))
        rast(means3D=g[0], means2D=torch.zeros_like(g[0]), shs=None, colors_precomp=g[1], opacities=g[2], scales=g[3], rotations=g[4],
             cov3D_precomp=None)
    assert cache.stats()["views"] == 1 and cache.stats()["misses"] == 3
    # full lists (parity tests) are never cached
    with R.forward_flags(full_lists=True):
        rast(means3D=g[0], means2D=torch.zeros_like(g[0]), shs=None, colors_precomp=g[1], opacities=g[2], scales=g[3], rotations=g[4],
             cov3D_precomp=None)
    assert cache.stats()["misses"] == 3 and cache.stats()["hits"] == 0


def test_fingerprint_is_content_and_position_dependent():
    import ctypes as C
    from seganygaussians_amd import _lib
    dev = torch.device("cuda:0")
    L = _lib.load()

    def fp(*ts):
        n = len(ts)
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        sizes = (C.c_size_t * n)(*[t.numel() * t.element_size() for t in ts])
        out = (C.c_uint64 * n)()
        assert L.mi_rast_fingerprint(n, ptrs, sizes, out, torch.cuda.current_stream(dev).cuda_stream) == 0
        return list(out)
    a = torch.randn(100003, device=dev)
    b = a.clone()
    assert fp(a) == fp(b) == fp(a, b)[:1]
    b[77] += 1e-6
    assert fp(a) != fp(b)
    c = a.clone()
    c[[3, 4]] = c[[4, 3]]          # same multiset of words, another order
    assert fp(a) != fp(c)
    assert fp(a[:50000].contiguous()) != fp(a[:50001].contiguous())
