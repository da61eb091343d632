"""Sparse tracking on the device (csrc/foto_sparse.hip; include/foto.h, "sparse tracking"):
feature points, a classical tracker for them, and dense flows read at them.

``corners``   Shi-Tomasi corners of a device frame: an (max_count, 2) device array of (x, y),
              the points buffer ``BBSolver.track_device`` / ``foto.device.bb_track`` take as it is
``LK``        pyramidal Lucas-Kanade with fixed counts for one frame size: ``set_frames`` once,
              then any number of ``track`` calls, with the forward-backward check on the device
``sample``    a flow buffer (a dense solver's result, a ground truth) read at the points

Everything stays in device memory; nothing here waits for the device but ``corners`` when it
returns the count as an int.
"""
import ctypes
import sys

import numpy as np

from . import _lib
from . import device as D
from ._lib import check, lib

CORNER_DEFAULTS = dict(quality=0.01, window=3, nms=5, margin=8)
LK_DEFAULTS = dict(radius=7, levels=4, min_size=16, iters=10, min_eig=1e-7)
FLAT, OUT, NONFINITE, INCONSISTENT = (_lib.FOTO_LK_FLAT, _lib.FOTO_LK_OUT, _lib.FOTO_LK_NONFINITE,
                                      _lib.FOTO_LK_INCONSISTENT)
_U8 = {"uint8": _lib.FOTO_U8}


def device_count(count):
    """The int of the 4-byte device count ``corners(..., wait=False)`` returns (waits)."""
    return int(count.to_numpy().view(np.int32)[0])


def corners(frame, max_count=1024, quality=CORNER_DEFAULTS["quality"], window=CORNER_DEFAULTS["window"],
            nms=CORNER_DEFAULTS["nms"], margin=CORNER_DEFAULTS["margin"], return_response=False, *, dtype="float32",
            out=None, wait=True, count_out=None, divisor=None, stream=None):
    """The ``max_count`` strongest Shi-Tomasi corners of a device frame (anything
    foto.device.as_image accepts), in raster order: (points, count), or (points, count, response)
    with ``return_response``.  points: a (max_count, 2) float32 | float64 DeviceArray (or ``out``)
    of (x, y), NaN from the count on.  count: an int -- the call then waits for the device -- or,
    with ``wait=False``, a 4-byte device array holding the int32 (``device_count``; ``count_out``: the
    caller's own (4,) uint8 device array for it)."""
    im = D.as_image(frame, divisor)
    h, w = im.shape
    max_count = int(max_count)
    if max_count < 1:
        raise ValueError(f"max_count = {max_count} must be >= 1")
    out, ptr, code = D._shaped_target(out, dtype, D._OUT_DTYPES, (max_count, 2), "points")
    o = _lib.CornerOpts(float(quality), int(window), int(nms), int(margin), 0)
    cnt, cptr, _ = D._shaped_target(count_out, "uint8", _U8, (4,), "count bytes")
    host = ctypes.c_int(0)
    resp = D.DeviceArray((h, w), np.float64) if return_response else None
    check(lib().foto_corners_dev(ctypes.byref(im), w, h, ctypes.byref(o), max_count, ctypes.c_void_p(ptr), code,
                                 ctypes.c_void_p(cptr), ctypes.byref(host) if wait else None,
                                 ctypes.c_void_p(resp.ptr) if return_response else None,
                                 ctypes.c_void_p(D.stream_handle(stream, frame))))
    count = host.value if wait else cnt
    return (out, count, resp) if return_response else (out, count)


class LK:
    """Pyramidal Lucas-Kanade for one (w, h) and one set of options (LK_DEFAULTS): the plan owns
    both frames' pyramids.  ``set_frames`` builds them; every ``track`` after it reads them."""

    def __init__(self, w, h, radius=LK_DEFAULTS["radius"], levels=LK_DEFAULTS["levels"], iters=LK_DEFAULTS["iters"],
                 min_size=LK_DEFAULTS["min_size"], min_eig=LK_DEFAULTS["min_eig"]):
        self.w, self.h = int(w), int(h)
        self._o = _lib.LKOpts(int(radius), int(levels), int(min_size), int(iters), float(min_eig))
        self.opts = {k: getattr(self._o, k) for k in LK_DEFAULTS}
        self._p = ctypes.c_void_p()
        check(lib().foto_lk_create(self.w, self.h, ctypes.byref(self._o), ctypes.byref(self._p)))

    def set_frames(self, f0, f1, stream=None, divisor=None):
        a, b = D._pair(f0, f1, divisor)
        if a.shape != (self.h, self.w):
            raise ValueError(f"frames of shape {a.shape}; this tracker was made for {(self.h, self.w)}")
        check(lib().foto_lk_set_frames_dev(self._p, ctypes.byref(a), ctypes.byref(b),
                                           ctypes.c_void_p(D.stream_handle(stream, f0, f1))))
        return self

    def track_raw(self, points, *, direction=0, prior=None, fb_tol=0.5, dtype="float32", out=None, status=None,
                  err=True, fb=False, stream=None):
        """One foto_lk_track_dev call: (disp, status, err or None, fb or None), all device arrays.
        ``prior``: an (M, 2) device array of ``dtype``; with it ``status`` must be the buffer of
        the track that made the prior, and gains INCONSISTENT unless fb <= fb_tol."""
        pptr, pcode, M = D.track_source(points)
        out, optr, code = D._shaped_target(out, dtype, D._OUT_DTYPES, (M, 2), "displacements")
        prptr = None
        if prior is not None:
            _, prptr, _ = D._shaped_target(prior, dtype, D._OUT_DTYPES, (M, 2), "priors")
            if status is None:
                raise ValueError("a prior needs the status buffer of the track that made it")
        elif fb:
            raise ValueError("fb is the length of the round trip and needs a prior")
        status, sptr, _ = D._shaped_target(status, "uint8", _U8, (M,), "status bytes")
        e = D.DeviceArray((M,), np.float64) if err else None
        f = D.DeviceArray((M,), np.float64) if fb else None
        check(lib().foto_lk_track_dev(self._p, ctypes.c_void_p(pptr), pcode, M, int(direction),
                                      ctypes.c_void_p(prptr) if prior is not None else None, float(fb_tol),
                                      ctypes.c_void_p(optr), code, ctypes.c_void_p(sptr),
                                      ctypes.c_void_p(e.ptr) if err else None, ctypes.c_void_p(f.ptr) if fb else None,
                                      ctypes.c_void_p(D.stream_handle(stream, points))))
        return out, status, e, f

    def track(self, points, *, check=False, fb_tol=0.5, dtype="float32", stream=None):
        """The displacements of the device points ``points`` ((M, 2) float32 | float64) from frame 0
        to frame 1: (disp (M, 2), status uint8 (M,), err float64 (M,)), and with ``check`` the
        forward-backward check -- a second track from the end points back into frame 0, which ORs
        INCONSISTENT into status where the round trip misses the start by more than ``fb_tol``
        pixels -- and its length fb float64 (M,) as a fourth result.  Nothing is downloaded."""
        disp, status, err, _ = self.track_raw(points, dtype=dtype, stream=stream)
        if not check:
            return disp, status, err
        _, status, _, fb = self.track_raw(points, direction=1, prior=disp, fb_tol=fb_tol, dtype=dtype, status=status,
                                          err=False, fb=True, stream=stream)
        return disp, status, err, fb

    def close(self):
        if self._p:
            lib().foto_lk_destroy(self._p)
            self._p = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        if sys is None or sys.is_finalizing():   # (as foto.gn.Plan.__del__)
            return
        try:
            self.close()
        except Exception:
            pass


def sample(flow, points, *, layout="planar", dtype=None, out=None, stream=None):
    """A device flow buffer (foto.render.flow_arg's shapes) read at the device points ``points``
    ((M, 2)) with the clamped bilinear sample: an (M, 2) device array of (u, v), (R, M, 2) for a
    flow with a record axis; ``dtype`` None: the flow's own."""
    from .render import flow_arg
    fl, R, h, w, batched = flow_arg(flow, layout)
    pptr, pcode, M = D.track_source(points)
    if dtype is None:
        dtype = "float32" if fl.dtype == _lib.FOTO_F32 else "float64"
    shape = (R, M, 2) if batched else (M, 2)
    out, optr, code = D._shaped_target(out, dtype, D._OUT_DTYPES, shape, "flow samples")
    check(lib().foto_flow_sample_dev(ctypes.byref(fl), w, h, ctypes.c_void_p(pptr), pcode, M, ctypes.c_void_p(optr),
                                     code, ctypes.c_void_p(D.stream_handle(stream, flow, points))))
    return out


CACHE_SIZE = 4
_trackers = {}


def cached_lk(w, h, **opts):
    """A process-wide LK for (w, h, options), the least recently used of CACHE_SIZE dropped
    (foto.tvl1.cached_tvl1's rule)."""
    unknown = set(opts) - set(LK_DEFAULTS)
    if unknown:
        raise TypeError(f"Lucas-Kanade options are {sorted(LK_DEFAULTS)}; got {sorted(unknown)}")
    o = dict(LK_DEFAULTS, **opts)
    key = (int(w), int(h)) + tuple(o[k] for k in LK_DEFAULTS)
    p = _trackers.pop(key, None)
    if p is None:
        p = LK(w, h, **o)
        while len(_trackers) >= CACHE_SIZE:
            _trackers.pop(next(iter(_trackers))).close()
    _trackers[key] = p
    return p


def clear_cache():
    while _trackers:
        _trackers.popitem()[1].close()
