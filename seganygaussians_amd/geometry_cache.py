"""Frozen-geometry reuse for the rasterizer's forward (opt-in; an extension: the reference recomputes everything per call).
rasterizer.py asks three things of the cache: whether a call may use it (`eligible`), the call's content key (`key`), and, after a
miss, the entry to keep (`capture`)."""
from __future__ import annotations

import collections
import ctypes as C
import os
import threading
import weakref

import torch

from . import _lib
from ._ffi import check, dev_ptr, stream_ptr

# forward modes of the tests and the profiling build whose lists or kernels differ from the product's: never cached
_NOCACHE_FLAGS = _lib.MI_RAST_FULL_LISTS | _lib.MI_RAST_NO_CULL | _lib.MI_RAST_VERIFY_LISTS | _lib.MI_RAST_TILE_FWD | _lib.MI_RAST_F32_BLEND

# The image buffer's num_rendered field (include/mi_rast.h): 64 partial sums of R, one per 128-byte line, then 16 words
# {lean entries, longest list, -, key bits, XCD run boundaries} that mi_rast_forward_reuse reads.
_R_SUMS_BYTES = 64 * 128
_WORDS_BYTES = 16 * 4


class GeometryCache:
    """Per-camera cache of what the geometry-only stages of a forward produce (preprocess, binning, per-tile sort): the geometry
    buffer, the blend lists, the tile ranges + XCD run boundaries, radii and num_rendered.  A later forward of the SAME geometry
    from the SAME camera runs the blend stage alone (include/mi_rast.h: mi_rast_forward_reuse).  Meant for SAGA's contrastive
    feature training, which optimises the feature rows only (scene/gaussian_model_ff.py:154-162) and revisits each of ~200 cameras
    ~50 times (train_contrastive_feature.py:231).

    The key is CONTENT: 64-bit fingerprints (mi_rast_fingerprint) of means3D, opacities, scales, rotations, cov3D_precomp, shs (when
    they colour the Gaussians), view / projection matrix and camera position, next to the scalar settings.  The reference's
    renderer passes activation OUTPUTS (gaussian_renderer/__init__.py:337-348: pc.get_opacity, get_scaling, get_rotation), new
    tensors per call, so storage identity alone would never hit -- and a freed tensor's address can be handed to another one.  A
    fingerprint is memoised per tensor OBJECT (weak reference), version counter, storage (weak reference) and data_ptr(): a
    parameter or camera tensor that is passed again unchanged costs nothing, any in-place change (`means3D.add_(...)`, an optimizer
    step on a geometry tensor) bumps `_version`, and rebinding (`p.data = new`, which keeps the object and the version) replaces the
    storage; either gets a new fingerprint and misses.  Writes through `.data` that keep the storage (`p.data.copy_(...)`,
    `p.data[:] = ...`) change neither and CANNOT be seen: call `clear()` after them.  Tensors seen for the first time are
    fingerprinted by one kernel, behind which the calling thread waits for the stream.

    Bytes kept per view: the geometry buffer (139 bytes per Gaussian), 4 bytes per blend-list entry, 8 bytes per tile, radii (4 bytes
    per Gaussian).  Least recently used views are dropped beyond `max_bytes`.

    The cached buffers are SHARED between the forwards of a view, the packed-gradient scratch of the geometry buffer included.  Each
    entry carries an epoch that every hit bumps: the miss forward's pre-zeroed scratch is taken by its backward only while no hit of
    that view came in between (otherwise the backward zero-fills it itself, as a hit's backward always does).  So any interleaving
    of forwards and backwards of cached views on one stream -- several renders of a view in one loss, no-grad renders between a
    forward and its backward, retained graphs -- gives the uncached results (tests/test_geometry_cache_edges.py).  Two backward
    passes of the same cached view must not run at the same time on different streams.  `debug=True` forwards and the full-list /
    verify modes of the tests are never cached."""

    def __init__(self, max_bytes=64 << 30):
        self.max_bytes = int(max_bytes)
        self.enabled = True
        self.entries = collections.OrderedDict()
        self.bytes = 0
        self.hits = self.misses = 0
        self._memo = {}          # id(tensor) -> (weakref, _version, storage weakref, data_ptr, fingerprint)
        self.lock = threading.Lock()

    def stats(self):
        n = self.hits + self.misses
        return {"hits": self.hits, "misses": self.misses, "hit_rate": (self.hits / n) if n else 0.0, "views": len(self.entries),
                "bytes_cached": self.bytes}

    def clear(self):
        with self.lock:
            self.entries.clear()
            self._memo.clear()
            self.bytes = 0
            self.hits = self.misses = 0

    def eligible(self, debug, prefiltered, flags):
        """May a forward with these settings look its geometry up (and fill an entry on a miss)?"""
        return self.enabled and not debug and not (int(flags) & _NOCACHE_FLAGS) and not prefiltered

    def fingerprints(self, tensors, dev):
        """One 64-bit content fingerprint per tensor (None for an absent one); memoised per (tensor object, version, storage,
        data_ptr).  The caller has checked that every tensor is a float32 GPU tensor."""
        out = [None] * len(tensors)
        todo = []
        for k, t in enumerate(tensors):
            if t is None or t.numel() == 0:
                continue
            m = self._memo.get(id(t))
            if (m is not None and m[0]() is t and m[1] == t._version and m[2]() is t.untyped_storage()
                    and m[3] == t.data_ptr()):
                out[k] = m[4]
            else:
                todo.append(k)
        for g0 in range(0, len(todo), 8):
            grp = todo[g0:g0 + 8]
            n = len(grp)
            ptrs = (C.c_void_p * n)(*[tensors[k].data_ptr() for k in grp])
            sizes = (C.c_size_t * n)(*[tensors[k].numel() * tensors[k].element_size() for k in grp])
            res = (C.c_uint64 * n)()
            with torch.cuda.device(dev):
                check(_lib.load().mi_rast_fingerprint(n, ptrs, sizes, res, stream_ptr(dev)))
            for k, v in zip(grp, res):
                t = tensors[k]
                out[k] = (int(v), tuple(t.shape), str(t.dtype))
                self._memo[id(t)] = (weakref.ref(t), t._version, weakref.ref(t.untyped_storage()), t.data_ptr(), out[k])
        if len(self._memo) > 4096:   # forget tensors that are gone
            self._memo = {i: m for i, m in self._memo.items() if m[0]() is not None}
        return out

    def key(self, dev, P, H, W, tan_fovx, tan_fovy, scale_modifier, degree, M, flags, bg, means3D, sh, colors, opacities, scales,
            rotations, cov3D_precomp, viewmatrix, projmatrix, campos):
        """The content key of one forward; the tensors are the contiguous ones the library call would get."""
        colours_from_sh = colors is None or colors.numel() == 0
        # the uncached call's device / dtype checks, in its order and with its messages, before a fingerprint kernel reads data_ptr()
        for x, name in ((bg, "bg"), (means3D, "means3D"), (sh, "sh"), (colors, "colors_precomp"), (opacities, "opacities"),
                        (scales, "scales"), (rotations, "rotations"), (cov3D_precomp, "cov3D_precomp"), (viewmatrix, "viewmatrix"),
                        (projmatrix, "projmatrix"), (campos, "campos")):
            dev_ptr(x, name, dev)
        fps = self.fingerprints([means3D, opacities, scales, rotations, cov3D_precomp, sh if colours_from_sh else None, viewmatrix,
                                 projmatrix, campos], dev)
        return (dev.index, P, H, W, float(tan_fovx), float(tan_fovy), float(scale_modifier), int(degree),
                int(M) if colours_from_sh else -1, int(flags), tuple(fps))

    def lookup(self, key):
        with self.lock:
            e = self.entries.get(key)
            if e is not None:
                self.entries.move_to_end(key)
                self.hits += 1
            else:
                self.misses += 1
            return e

    def insert(self, key, entry):
        with self.lock:
            old = self.entries.pop(key, None)
            if old is not None:
                self.bytes -= old["bytes"]
            self.entries[key] = entry
            self.bytes += entry["bytes"]
            while self.bytes > self.max_bytes and len(self.entries) > 1:
                _, dropped = self.entries.popitem(last=False)
                self.bytes -= dropped["bytes"]

    def capture(self, key, W, H, rendered, radii, geom, binning, img):
        """First visit of this (geometry, camera): keeps what the geometry-only stages of the forward that just returned produced
        and returns the new entry.  The blend list (first field of the binning buffer, include/mi_rast.h) is copied at its real
        length, tile ranges and the 16 words behind the R partial sums likewise; the geometry buffer is kept as it is (this
        forward's backward shares it)."""
        _, ioff = _lib.image_layout(W, H)
        tiles = ((W + 15) // 16) * ((H + 15) // 16)
        w0 = ioff["num_rendered"] + _R_SUMS_BYTES
        words = img[w0:w0 + _WORDS_BYTES].clone()
        n_list = int(words.view(torch.int32)[0].item()) if rendered > 0 else 0   # entries the lists hold (lean: <= num_rendered)
        entry = {"geom": geom, "num_rendered": rendered, "radii": radii.clone(), "img_bytes": int(img.numel()),
                 "blend_list": binning[:max(4 * n_list, 4)].clone(), "ranges": img[ioff["ranges"]:ioff["ranges"] + 8 * tiles].clone(),
                 "words": words, "longest_run": int(_lib.load().mi_rast_last_longest_run()), "epoch": [0]}
        entry["bytes"] = sum(int(entry[k].numel()) * entry[k].element_size() for k in ("geom", "blend_list", "ranges", "words", "radii"))
        self.insert(key, entry)
        return entry


_geometry_cache = None


def enable_geometry_cache(max_bytes=64 << 30):
    """Switches the frozen-geometry reuse on for every forward of this process (GeometryCache); returns the cache (`.stats()`).
    Also switched on by MI_RAST_GEOMETRY_CACHE=<GiB> (or 1: 64 GiB) in the environment, for unchanged reference scripts."""
    global _geometry_cache
    if _geometry_cache is None:
        _geometry_cache = GeometryCache(max_bytes)
    else:
        _geometry_cache.max_bytes = int(max_bytes)
    _geometry_cache.enabled = True
    return _geometry_cache


def disable_geometry_cache(drop=False):
    """Forwards recompute everything again; the cached views are kept for a later enable_geometry_cache() unless `drop`."""
    global _geometry_cache
    if _geometry_cache is not None:
        _geometry_cache.enabled = False
        if drop:
            _geometry_cache = None


def geometry_cache():
    return _geometry_cache


if os.environ.get("MI_RAST_GEOMETRY_CACHE", "") not in ("", "0"):
    try:
        _gib = float(os.environ["MI_RAST_GEOMETRY_CACHE"])
    except ValueError:
        _gib = 1.0
    enable_geometry_cache(int((64 if _gib == 1.0 else _gib) * (1 << 30)))
