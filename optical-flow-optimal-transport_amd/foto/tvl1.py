"""Duality-based TV-L1 optical flow with an illumination channel on the GPU (csrc/foto_tvl1.hip;
include/foto.h has the algorithm): the classical baseline that keeps motion boundaries sharp."""
import collections
import ctypes
import sys

import numpy as np

from ._lib import check, dptr, f64, lib

DEFAULTS = dict(lam=38.0, theta=0.3, tau=0.25, gamma=0.1, levels=4, warps=5, iters=30, min_size=16, per_launch=5)
TILE_W, TILE_H = 64, 4   # the iteration kernel's tile (csrc: TX x TY): the tests' frame sizes derive from it
# with per_launch = K > 1 a block works on a REGION_W x REGION_H region and stores the
# (REGION_W - 2 K) x (REGION_H - 2 K) tile in its middle (csrc: TR_W x TR_H)
REGION_W, REGION_H = 32, 24


def _opts(kw):
    """The foto_tvl1_opts of DEFAULTS updated by ``kw`` (``lambda_`` is accepted for ``lam``)."""
    from ._lib import TVL1Opts
    kw = dict(kw)
    if "lambda_" in kw:
        kw["lam"] = kw.pop("lambda_")
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"TV-L1 options are {sorted(DEFAULTS)}; got {sorted(unknown)}")
    o = dict(DEFAULTS, **kw)
    return TVL1Opts(float(o["lam"]), float(o["theta"]), float(o["tau"]), float(o["gamma"]), int(o["levels"]),
                    int(o["warps"]), int(o["iters"]), int(o["min_size"]), int(o["per_launch"]))


def coeffs(f1, f2, u, v, w, h, gamma):
    """One warp's (a1, a2, a3, n2, rc) at U0 = (u, v) (k_tvl1_coeffs)."""
    n = w * h
    a, b, uu, vv = f64(f1, n, "f1"), f64(f2, n, "f2"), f64(u, n, "u"), f64(v, n, "v")
    out = np.empty(5 * n)
    check(lib().foto_tvl1_coeffs(dptr(a), dptr(b), dptr(uu), dptr(vv), w, h, float(gamma), dptr(out)))
    return tuple(out[k * n:(k + 1) * n] for k in range(5))


def iterate(co, U, P, w, h, lam, theta, tau, n, per_launch=1):
    """``n`` inner iterations from co = (a1, a2, a3, n2, rc), U = (u, v, w) and P = the six dual
    fields, at most ``per_launch`` of them in one kernel launch (1: k_tvl1_iter, more: k_tvl1_tile);
    returns (U, P) as lists of new arrays."""
    N = w * h
    c = np.concatenate([f64(x, N, "coefficient") for x in co])
    uu = np.concatenate([f64(x, N, "U") for x in U])
    pp = np.concatenate([f64(x, N, "P") for x in P])
    if (len(co), len(U), len(P)) != (5, 3, 6):
        raise ValueError("iterate takes 5 coefficient fields, 3 of U and 6 of P")
    check(lib().foto_tvl1_iterate(dptr(c), dptr(uu), dptr(pp), w, h, float(lam), float(theta), float(tau), int(n),
                                  int(per_launch)))
    return [uu[k * N:(k + 1) * N] for k in range(3)], [pp[k * N:(k + 1) * N] for k in range(6)]


class TVL1:
    """A reusable TV-L1 solver for one (w, h) and one set of options (DEFAULTS): the level frames,
    the primal and dual fields and one stream, made once.  The flow is the pyramid's,
    f1(x) ~ (1 - m) f2(x + u), with m = gamma w; gamma = 0 leaves m exactly zero."""

    def __init__(self, w, h, **opts):
        from .gn import pyramid_sizes
        self.w, self.h = int(w), int(h)
        self._o = _opts(opts)
        self.opts = {k: getattr(self._o, k) for k in DEFAULTS}
        self._p = ctypes.c_void_p()
        check(lib().foto_tvl1_create(self.w, self.h, ctypes.byref(self._o), ctypes.byref(self._p)))
        self.sizes = pyramid_sizes(self.w, self.h, self._o.levels, self._o.min_size)

    def _stats(self):
        from ._lib import TVL1Stats
        cap = len(self.sizes)
        keep = ((ctypes.c_int * cap)(), (ctypes.c_int * cap)(), (ctypes.c_int * cap)(), (ctypes.c_double * cap)())
        return TVL1Stats(cap, *keep), keep

    @staticmethod
    def _report(st, keep):
        wl, hl, launches, ms = keep
        L = st.levels
        return {"levels": L, "sizes": [(wl[l], hl[l]) for l in range(L)], "launches": [launches[l] for l in range(L)],
                "launches_total": st.launches_total, "ms_level": [ms[l] for l in range(L)], "ms_total": st.ms_total}

    def solve(self, f1, f2):
        """Returns (u, v, m, stats): stats = {levels, sizes, launches, launches_total, ms_level,
        ms_total}, levels finest first."""
        n = self.w * self.h
        a, b = f64(f1, n, "f1"), f64(f2, n, "f2")
        out = np.empty(3 * n)
        u, v, m = out[:n], out[n:2 * n], out[2 * n:]
        st, keep = self._stats()
        check(lib().foto_tvl1_solve(self._p, dptr(a), dptr(b), dptr(u), dptr(v), dptr(m), ctypes.byref(st)))
        return u, v, m, self._report(st, keep)

    def solve_device(self, f1, f2, out=None, dtype="float32", layout="planar", stream=None, stats=False):
        """solve() on two device frames (anything foto.device.as_image accepts), the flow left on
        the device (foto_tvl1_solve_dev): returns (out, stats) with out a DeviceArray (or the given
        contiguous device array) -- "planar" [3][h][w] = u, v, m or "interleaved" [h][w][2] =
        (u, v).  stats is None unless asked for: reading the per-level times waits for the last
        level."""
        from . import device as D
        a, b = D._pair(f1, f2)
        if a.shape != (self.h, self.w):
            raise ValueError(f"frames of shape {a.shape}; this solver was made for {(self.h, self.w)}")
        sh = D.stream_handle(stream, f1, f2)
        out, ptr, dcode, lcode = D.export_target(out, dtype, layout, self.h, self.w)
        st, keep = self._stats() if stats else (None, None)
        check(lib().foto_tvl1_solve_dev(self._p, ctypes.byref(a), ctypes.byref(b), ctypes.c_void_p(ptr), dcode, lcode,
                                        ctypes.c_void_p(sh), ctypes.byref(st) if stats else None))
        return out, (self._report(st, keep) if stats else None)

    def close(self):
        if self._p:
            lib().foto_tvl1_destroy(self._p)
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


CACHE_SIZE = 4
_solvers = collections.OrderedDict()


def cached_tvl1(w, h, **opts):
    """A process-wide TVL1 for (w, h, options), the least recently used of CACHE_SIZE dropped
    (foto.gn.cached_pyramid's rule)."""
    o = _opts(opts)
    key = (int(w), int(h)) + tuple(getattr(o, k) for k in DEFAULTS)
    p = _solvers.pop(key, None)
    if p is None:
        p = TVL1(w, h, **{k: getattr(o, k) for k in DEFAULTS})
        while len(_solvers) >= CACHE_SIZE:
            _solvers.popitem(last=False)[1].close()
    _solvers[key] = p
    return p


def clear_cache():
    while _solvers:
        _solvers.popitem()[1].close()
