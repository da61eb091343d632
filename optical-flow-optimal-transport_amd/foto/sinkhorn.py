"""Entropic optimal transport between two frames on the GPU (csrc/foto_sinkhorn.hip; include/foto.h
has the arithmetic): convolutional Sinkhorn with the cost |x - y|^2 / 2, the static counterpart of
the Benamou-Brenier solver.  The plan's barycentric projection is a flow, its cost a W2, and the
debiased divergence removes the entropic blur from that W2."""
import collections
import ctypes
import sys

import numpy as np

from . import _lib
from ._lib import check, dptr, f64, lib

MAX_RADIUS = _lib.FOTO_SINKHORN_MAX_RADIUS
TILE_W, TILE_H = _lib.FOTO_SINKHORN_TILE_W, _lib.FOTO_SINKHORN_TILE_H   # the fused kernel's tile (csrc: SK_TX x SK_TY)
_DIRECTIONS = {"forward": 0, "backward": 1}

Info = collections.namedtuple("Info", "mass0 mass1 marginal_error cost w2 bad unreachable iterations")
Divergence = collections.namedtuple("Divergence", "divergence w2_debiased cost01 cost00 cost11 mass0 mass1")


def _args(eps, radius):
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)) or not 0 <= radius <= MAX_RADIUS:
        raise ValueError(f"radius = {radius!r} must be an int in 0 .. {MAX_RADIUS}")
    eps = float(eps)
    if not (np.isfinite(eps) and eps > 0):
        raise ValueError(f"eps = {eps!r} must be finite and > 0")
    return eps, int(radius)


def tables(eps, R):
    """The host tables of the solver, float64 (3, R + 1) for d = 0 .. R: k[d] = exp(-d d / (2 eps)),
    k1[d] = d k[d], k2[d] = (0.5 (d d)) k[d].  The device never evaluates exp."""
    eps, R = _args(eps, R)
    d = np.arange(R + 1, dtype=np.float64)
    k = np.exp(-(d * d) / (2.0 * np.float64(eps)))
    return np.stack([k, d * k, (0.5 * (d * d)) * k])


def _count(n, what="n"):
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or n < 0:
        raise ValueError(f"{what} = {n!r} must be an int >= 0")
    return int(n)


def _frame(f, h=None, w=None):
    """A device frame of anything: device arrays and descriptors as they are, host arrays uploaded
    (uint8 / float32 / float64 kept, everything else as float64; a flat array takes (h, w))."""
    from . import device as D
    if isinstance(f, _lib.Image) or hasattr(f, "__cuda_array_interface__"):
        return f
    a = np.asarray(f)
    if a.dtype not in (np.uint8, np.float32, np.float64):
        a = a.astype(np.float64)
    if a.ndim == 1 and h is not None and a.size == h * w:
        a = a.reshape(h, w)
    return D.DeviceArray.from_numpy(a)


class Sinkhorn:
    """A reusable entropic-transport solver for one (w, h), eps and window radius: the frames, the
    two scalings and one stream, made once.  ``set_frames`` starts from b = 1; ``iterate(n)`` runs n
    Sinkhorn iterations (two launches each, no stop test) and may be called again to go on."""

    def __init__(self, w, h, eps=2.0, radius=16):
        self.eps, self.radius = _args(eps, radius)
        self.w, self.h = int(w), int(h)
        if self.w < 1 or self.h < 1:
            raise ValueError(f"w = {w}, h = {h}: both must be >= 1")
        self.tables = tables(self.eps, self.radius)
        self._p = ctypes.c_void_p()
        o = _lib.SinkhornOpts(self.radius, 0, self.eps)
        check(lib().foto_sinkhorn_create(self.w, self.h, ctypes.byref(o), dptr(self.tables), ctypes.byref(self._p)))

    def _pair(self, f0, f1):
        from . import device as D
        a, b = D._pair(_frame(f0, self.h, self.w), _frame(f1, self.h, self.w))
        if a.shape != (self.h, self.w):
            raise ValueError(f"frames of shape {a.shape}; this solver was made for {(self.h, self.w)}")
        return a, b

    def set_frames(self, f0, f1, stream=None):
        """The two frames (anything foto.device.as_image accepts, or host arrays); b = 1 and the
        iteration count 0 again."""
        from . import device as D
        a, b = self._pair(f0, f1)
        check(lib().foto_sinkhorn_set_frames_dev(self._p, ctypes.byref(a), ctypes.byref(b),
                                                 ctypes.c_void_p(D.stream_handle(stream, f0, f1))))
        return self

    def iterate(self, n, stream=None):
        from . import device as D
        n = _count(n)
        check(lib().foto_sinkhorn_iterate_dev(self._p, n, ctypes.c_void_p(D.stream_handle(stream))))
        return self

    def flow(self, direction="forward", dtype="float32", layout="planar", valid=False, out=None, stream=None):
        """The barycentric projection of the plan as a flow record on the device: frame 0 -> frame 1
        ("forward") or frame 1 -> frame 0 ("backward"); "planar" [3][h][w] = u, v, m (m = 0) or
        "interleaved" [h][w][2] = (u, v).  With ``valid`` returns (flow, valid), valid a uint8 (h, w)
        DeviceArray: 1 where the pixel has mass and the window reaches some."""
        from . import device as D
        if direction not in _DIRECTIONS:
            raise ValueError(f"direction {direction!r}: 'forward' or 'backward'")
        out, ptr, dcode, lcode = D.export_target(out, dtype, layout, self.h, self.w)
        mask = D.DeviceArray((self.h, self.w), np.uint8) if valid else None
        check(lib().foto_sinkhorn_flow_dev(self._p, _DIRECTIONS[direction], ctypes.c_void_p(ptr), dcode, lcode,
                                           ctypes.c_void_p(mask.ptr if valid else None),
                                           ctypes.c_void_p(D.stream_handle(stream))))
        return (out, mask) if valid else out

    def info_device(self, out=None, stream=None):
        """The float64 (8,) record left on the device: sum mu, sum nu, marginal error, sharp cost, bad,
        unreachable, iterations, 0."""
        from . import device as D
        out, ptr, _ = D._shaped_target(out, "float64", {"float64": _lib.FOTO_F64}, (8,), "records")
        check(lib().foto_sinkhorn_info_dev(self._p, ctypes.c_void_p(ptr), ctypes.c_void_p(D.stream_handle(stream))))
        return out

    def info(self):
        """The record downloaded: an ``Info`` (w2 = sqrt(2 cost), not divided by the mass).  The
        download goes through the null stream: a caller with a non-blocking stream of its own takes
        ``info_device`` and reads it after that stream."""
        r = self.info_device().to_numpy()
        return Info(float(r[0]), float(r[1]), float(r[2]), float(r[3]), float(np.sqrt(2.0 * r[3])), int(r[4]), int(r[5]),
                    int(r[6]))

    def scalings(self, stream=None):
        """(a, b): the two scalings as float64 (h, w) DeviceArrays."""
        from . import device as D
        a, b = D.DeviceArray((self.h, self.w)), D.DeviceArray((self.h, self.w))
        check(lib().foto_sinkhorn_scalings_dev(self._p, ctypes.c_void_p(a.ptr), ctypes.c_void_p(b.ptr),
                                               ctypes.c_void_p(D.stream_handle(stream))))
        return a, b

    def solve(self, f0, f1, iters):
        """One shot on host arrays (foto_sinkhorn_solve): (u, v, m) as float64 vectors, m = 0."""
        n = self.w * self.h
        a, b = f64(f0, n, "f0"), f64(f1, n, "f1")
        out = np.empty(3 * n)
        u, v, m = out[:n], out[n:2 * n], out[2 * n:]
        check(lib().foto_sinkhorn_solve(self._p, dptr(a), dptr(b), _count(iters, "iters"), dptr(u), dptr(v), dptr(m)))
        return u, v, m

    def solve_device(self, f0, f1, iters, out=None, dtype="float32", layout="planar", stream=None):
        """One shot on device frames, the forward flow left on the device (foto_sinkhorn_solve_dev)."""
        from . import device as D
        a, b = self._pair(f0, f1)
        out, ptr, dcode, lcode = D.export_target(out, dtype, layout, self.h, self.w)
        check(lib().foto_sinkhorn_solve_dev(self._p, ctypes.byref(a), ctypes.byref(b), _count(iters, "iters"),
                                            ctypes.c_void_p(ptr), dcode, lcode,
                                            ctypes.c_void_p(D.stream_handle(stream, f0, f1))))
        return out

    def close(self):
        if self._p:
            lib().foto_sinkhorn_destroy(self._p)
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


def divergence(f0, f1, eps=2.0, radius=16, iters=100):
    """The debiased Sinkhorn divergence of two frames of one shape: the three solves (f0, f1),
    (f0, f0), (f1, f1) on one context; a ``Divergence`` with divergence = cost01 - cost00 / 2 -
    cost11 / 2 and w2_debiased = sqrt(2 max(divergence, 0)), in TransportReport.w2's units (not
    divided by the mass)."""
    from . import device as D
    eps, radius = _args(eps, radius)
    iters = _count(iters, "iters")
    a, b = _frame(f0), _frame(f1)
    ia, ib = D._pair(a, b)
    h, w = ia.shape
    with Sinkhorn(w, h, eps, radius) as s:
        recs = [s.set_frames(x, y).iterate(iters).info() for x, y in ((a, b), (a, a), (b, b))]
    c01, c00, c11 = (r.cost for r in recs)
    d = c01 - 0.5 * c00 - 0.5 * c11
    return Divergence(d, float(np.sqrt(2.0 * max(d, 0.0))), c01, c00, c11, recs[0].mass0, recs[0].mass1)


CACHE_SIZE = 4
_solvers = collections.OrderedDict()


def cached_sinkhorn(w, h, eps=2.0, radius=16):
    """A process-wide Sinkhorn for (w, h, eps, radius), the least recently used of CACHE_SIZE
    dropped (foto.tvl1.cached_tvl1's rule)."""
    eps, radius = _args(eps, radius)
    key = (int(w), int(h), eps, radius)
    p = _solvers.pop(key, None)
    if p is None:
        p = Sinkhorn(w, h, eps, radius)
        while len(_solvers) >= CACHE_SIZE:
            _solvers.popitem(last=False)[1].close()
    _solvers[key] = p
    return p


def clear_cache():
    while _solvers:
        _solvers.popitem()[1].close()
