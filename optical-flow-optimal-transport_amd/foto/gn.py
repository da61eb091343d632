"""Gennert-Negahdaripour baseline on the GPU (classical.py:25-130 semantics)."""
import collections
import os
import ctypes
import sys

import numpy as np

from ._lib import check, dptr, f64, lib

GN_RTOL = 1e-10      # PCG relative residual; matches SuperLU's spsolve to ~1e-8
GN_MAXITER = 200000


def apply(f1, f2, w, h, alpha, lam, x):
    n = w * h
    a, b, xx = f64(f1, n, "f1"), f64(f2, n, "f2"), f64(x, 3 * n, "x")
    y = np.empty(3 * n)
    check(lib().foto_gn_apply(dptr(a), dptr(b), w, h, float(alpha), float(lam), dptr(xx), dptr(y)))
    return y


def rhs(f1, f2, w, h):
    n = w * h
    a, b = f64(f1, n, "f1"), f64(f2, n, "f2")
    out = np.empty(3 * n)
    check(lib().foto_gn_rhs(dptr(a), dptr(b), w, h, dptr(out)))
    return out


def _outputs(n):
    """u, v, m as three views of one array: at 640x480 one 7.4 MB allocation, which numpy backs
    with transparent huge pages (it advises them from 4 MB), so copying the solution out faults
    in a few 2 MB pages instead of ~1800 4 KB ones (0.4-0.9 ms of a 4.4 ms solve, FOTO_GN_TRACE)."""
    out = np.empty(3 * n)
    return out[:n], out[n:2 * n], out[2 * n:]


def solve(f1, f2, w, h, alpha, lam, rtol=GN_RTOL, maxiter=GN_MAXITER):
    """Returns (u, v, m, info, iterations)."""
    n = w * h
    a, b = f64(f1, n, "f1"), f64(f2, n, "f2")
    u, v, m = _outputs(n)
    its = ctypes.c_int(0)
    info = check(lib().foto_gn_solve(dptr(a), dptr(b), w, h, float(alpha), float(lam), float(rtol), int(maxiter),
                                     dptr(u), dptr(v), dptr(m), ctypes.byref(its)))
    return u, v, m, info, its.value


def solve_ex(f1, f2, w, h, alpha, lam, rtol=GN_RTOL, maxiter=GN_MAXITER):
    """foto_gn_solve_ex (include/foto.h): solve() with the per-solve report -- returns
    (u, v, m, stats) with stats = {iterations, info, plan_reused, levels, ms_setup, ms_pcg,
    ms_total, alg_bytes_per_iter}."""
    from ._lib import GNStats
    n = w * h
    a, b = f64(f1, n, "f1"), f64(f2, n, "f2")
    u, v, m = _outputs(n)
    st = GNStats()
    check(lib().foto_gn_solve_ex(dptr(a), dptr(b), w, h, float(alpha), float(lam), float(rtol), int(maxiter),
                                 dptr(u), dptr(v), dptr(m), ctypes.byref(st)))
    return u, v, m, {f: getattr(st, f) for f, _ in GNStats._fields_}


class Plan:
    """A reusable GN solver for one (w, h, alpha, lambda): classical.GLLOpticalFlow after
    setAlpha/setLambda (classical.py:25-66).  Buffers, the multigrid hierarchy and the replayed
    PCG graph are made once; solve(f1, f2) is one process() (classical.py:68-130)."""

    def __init__(self, w, h, alpha, lam, rtol=GN_RTOL, maxiter=GN_MAXITER):
        self.w, self.h, self.alpha, self.lam = int(w), int(h), float(alpha), float(lam)
        self._p = ctypes.c_void_p()
        check(lib().foto_gn_plan_create(self.w, self.h, self.alpha, self.lam, float(rtol), int(maxiter),
                                        ctypes.byref(self._p)))

    def solve(self, f1, f2):
        """Returns (u, v, m, info, iterations), like solve()."""
        n = self.w * self.h
        a, b = f64(f1, n, "f1"), f64(f2, n, "f2")
        u, v, m = _outputs(n)
        its = ctypes.c_int(0)
        info = check(lib().foto_gn_plan_solve(self._p, dptr(a), dptr(b), dptr(u), dptr(v), dptr(m),
                                              ctypes.byref(its)))
        return u, v, m, info, its.value

    def solve_device(self, f1, f2, out=None, dtype="float32", layout="planar", stream=None):
        """solve() on two device frames (anything foto.device.as_image accepts), the solution
        left on the device (foto_gn_plan_solve_dev): returns (out, info, iterations) with out a
        DeviceArray (or the given contiguous device array) -- "planar" [3][h][w] = u, v, m or
        "interleaved" [h][w][2] = (u, v).  No pinned staging, no host copies."""
        from . import device as D
        a, b = D._pair(f1, f2)
        if a.shape != (self.h, self.w):
            raise ValueError(f"frames of shape {a.shape}; this plan was made for {(self.h, self.w)}")
        st = D.stream_handle(stream, f1, f2)
        out, ptr, dcode, lcode = D.export_target(out, dtype, layout, self.h, self.w)
        its = ctypes.c_int(0)
        info = check(lib().foto_gn_plan_solve_dev(self._p, ctypes.byref(a), ctypes.byref(b), ctypes.c_void_p(ptr),
                                                  dcode, lcode, ctypes.c_void_p(st), ctypes.byref(its)))
        return out, info, its.value

    def timing(self):
        """{ms_setup, ms_pcg, iterations, launched} of the last solve (device events)."""
        out = np.zeros(4)
        check(lib().foto_gn_plan_timing(self._p, dptr(out)))
        return {"ms_setup": float(out[0]), "ms_pcg": float(out[1]), "iterations": int(out[2]),
                "launched": int(out[3])}

    def close(self):
        if self._p:
            lib().foto_gn_plan_destroy(self._p)
            self._p = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        # at interpreter shutdown the HIP runtime may already be torn down: leave the plan
        # to process exit (foto_capi.cpp's cached plan does the same)
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


PLAN_CACHE_SIZE = 4
_plans = collections.OrderedDict()


def cached_plan(w, h, alpha, lam, rtol=GN_RTOL, maxiter=GN_MAXITER):
    """A process-wide Plan for (w, h, alpha, lambda, rtol, maxiter), shared by every
    GLLOpticalFlow instance (least recently used of PLAN_CACHE_SIZE dropped): a batch of frames
    of one size -- run.sh's per-sequence GN runs -- makes its buffers, multigrid hierarchy and
    graph once, and instances that come and go do not each hold device memory."""
    key = (int(w), int(h), float(alpha), float(lam), float(rtol), int(maxiter))
    env = tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("FOTO_GN")))   # read at plan build
    p = _plans.pop(key + (env,), None)
    if p is None:
        p = Plan(*key)
        while len(_plans) >= PLAN_CACHE_SIZE:
            _plans.popitem(last=False)[1].close()
    _plans[key + (env,)] = p
    return p


def clear_plan_cache():
    while _plans:
        _plans.popitem()[1].close()
    while _pyramids:
        _pyramids.popitem()[1].close()


# ----------------------------------------------------------------------------- coarse-to-fine

def pyramid_sizes(w, h, levels, min_size=16):
    """The level sizes [(w_0, h_0), ...], finest first (foto_gn_pyr_sizes; host only)."""
    from ._lib import GN_PYR_MAX_LEVELS
    wl = (ctypes.c_int * GN_PYR_MAX_LEVELS)()
    hl = (ctypes.c_int * GN_PYR_MAX_LEVELS)()
    n = ctypes.c_int(0)
    check(lib().foto_gn_pyr_sizes(int(w), int(h), int(levels), int(min_size), wl, hl, GN_PYR_MAX_LEVELS,
                                  ctypes.byref(n)))
    return [(wl[l], hl[l]) for l in range(n.value)]


def pyr_down(f1, f2, w, h):
    """Both frames of a w x h level restricted to ceil(w/2) x ceil(h/2) (k_pyr_down)."""
    n, nc = w * h, ((w + 1) // 2) * ((h + 1) // 2)
    a, b = f64(f1, n, "f1"), f64(f2, n, "f2")
    c1, c2 = np.empty(nc), np.empty(nc)
    check(lib().foto_pyr_down(dptr(a), dptr(b), w, h, dptr(c1), dptr(c2)))
    return c1, c2


def pyr_up(u, v, m, wc, hc, w, h):
    """u, v, m prolonged from wc x hc to w x h with the displacement scales (k_pyr_up)."""
    nc, n = wc * hc, w * h
    a, b, c = f64(u, nc, "u"), f64(v, nc, "v"), f64(m, nc, "m")
    uo, vo, mo = _outputs(n)
    check(lib().foto_pyr_up(dptr(a), dptr(b), dptr(c), wc, hc, w, h, dptr(uo), dptr(vo), dptr(mo)))
    return uo, vo, mo


def warp_prior(f2, u, v, m, w, h):
    """g = (1 - m) S(f2; x + u, y + v) (k_pyr_warp)."""
    n = w * h
    a, uu, vv, mm = f64(f2, n, "f2"), f64(u, n, "u"), f64(v, n, "v"), f64(m, n, "m")
    g = np.empty(n)
    check(lib().foto_gn_warp_prior(dptr(a), dptr(uu), dptr(vv), dptr(mm), w, h, dptr(g)))
    return g


def solve_prior(f1, g, w, h, alpha, lam, prior=None, rtol=GN_RTOL, maxiter=GN_MAXITER):
    """One increment solve of the pyramid: A(f1, g) d = b(f1, g) - [alpha N u0; alpha N v0;
    lambda N m0] with prior = (u0, v0, m0) (None: no prior, Plan.solve); returns the total flow
    (u, v, m, info, iterations)."""
    n = w * h
    a, b = f64(f1, n, "f1"), f64(g, n, "g")
    held = [] if prior is None else [f64(p, n, "prior") for p in prior]
    pr = [dptr(p) for p in held] or [None, None, None]   # (None travels as a null pointer)
    u, v, m = _outputs(n)
    its = ctypes.c_int(0)
    info = check(lib().foto_gn_solve_prior(dptr(a), dptr(b), w, h, float(alpha), float(lam), float(rtol),
                                           int(maxiter), *pr, dptr(u), dptr(v), dptr(m), ctypes.byref(its)))
    return u, v, m, info, its.value


class Pyramid:
    """Coarse-to-fine GN for one (w, h, alpha, lambda): an image pyramid, warping of the second
    frame by the flow found so far and a re-solve for the increment with the total flow
    regularised (include/foto.h has the algorithm).  One Plan per level on one stream,
    made once.  levels = 1, warps = 1 is Plan.solve, bit for bit.  The flow is the reference's,
    f1(x) ~ (1 - m) f2(x + u); drawing it with foto.render.reconstruct is a first-order
    identification."""

    def __init__(self, w, h, alpha, lam, levels=4, warps=3, min_size=16, rtol=GN_RTOL, maxiter=GN_MAXITER):
        from ._lib import GNPyrOpts
        self.w, self.h, self.alpha, self.lam = int(w), int(h), float(alpha), float(lam)
        self.levels, self.warps, self.min_size = int(levels), int(warps), int(min_size)
        self._p = ctypes.c_void_p()
        o = GNPyrOpts(self.levels, self.warps, self.min_size, float(rtol), int(maxiter))
        check(lib().foto_gn_pyr_create(self.w, self.h, self.alpha, self.lam, ctypes.byref(o), ctypes.byref(self._p)))
        self.sizes = pyramid_sizes(self.w, self.h, self.levels, self.min_size)

    def _stats(self):
        from ._lib import GNPyrStats
        cap = len(self.sizes) * self.warps
        its, info = (ctypes.c_int * cap)(), (ctypes.c_int * cap)()
        st = GNPyrStats(cap=cap, its=its, info=info)
        return st, its, info

    @staticmethod
    def _report(st, its, info):
        L = st.levels
        return {"levels": L, "solves": st.solves, "sizes": [(st.wl[l], st.hl[l]) for l in range(L)],
                "iterations": [its[k] for k in range(st.solves)], "info": [info[k] for k in range(st.solves)],
                "ms_level": [st.ms_level[l] for l in range(L)], "ms_new": st.ms_new, "ms_total": st.ms_total}

    def solve(self, f1, f2):
        """Returns (u, v, m, info, stats): info = the number of solves that hit maxiter (0: all
        converged); stats = {levels, solves, sizes, iterations, info (per solve, coarsest level
        first), ms_level, ms_new, ms_total}."""
        n = self.w * self.h
        a, b = f64(f1, n, "f1"), f64(f2, n, "f2")
        u, v, m = _outputs(n)
        st, its, inf = self._stats()
        info = check(lib().foto_gn_pyr_solve(self._p, dptr(a), dptr(b), dptr(u), dptr(v), dptr(m), ctypes.byref(st)))
        return u, v, m, info, self._report(st, its, inf)

    def solve_device(self, f1, f2, out=None, dtype="float32", layout="planar", stream=None, stats=False):
        """solve() on two device frames with the arguments of Plan.solve_device, the flow left on
        the device (foto_gn_pyr_solve_dev): returns (out, info, stats).  stats is None unless
        asked for: reading the per-level times waits for the last level."""
        from . import device as D
        a, b = D._pair(f1, f2)
        if a.shape != (self.h, self.w):
            raise ValueError(f"frames of shape {a.shape}; this pyramid was made for {(self.h, self.w)}")
        sh = D.stream_handle(stream, f1, f2)
        out, ptr, dcode, lcode = D.export_target(out, dtype, layout, self.h, self.w)
        st, its, inf = self._stats() if stats else (None, None, None)
        info = check(lib().foto_gn_pyr_solve_dev(self._p, ctypes.byref(a), ctypes.byref(b), ctypes.c_void_p(ptr),
                                                 dcode, lcode, ctypes.c_void_p(sh),
                                                 ctypes.byref(st) if stats else None))
        return out, info, (self._report(st, its, inf) if stats else None)

    def close(self):
        if self._p:
            lib().foto_gn_pyr_destroy(self._p)
            self._p = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        if sys is None or sys.is_finalizing():   # (as Plan.__del__; at module teardown sys may be gone)
            return
        try:
            self.close()
        except Exception:
            pass


_pyramids = collections.OrderedDict()


def cached_pyramid(w, h, alpha, lam, levels=4, warps=3, min_size=16, rtol=GN_RTOL, maxiter=GN_MAXITER):
    """cached_plan for Pyramids: one per (w, h, alpha, lambda, levels, warps, min_size, rtol,
    maxiter) and FOTO_GN* environment, the least recently used of PLAN_CACHE_SIZE dropped."""
    key = (int(w), int(h), float(alpha), float(lam), int(levels), int(warps), int(min_size), float(rtol),
           int(maxiter))
    env = tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("FOTO_GN")))   # read at plan build
    p = _pyramids.pop(key + (env,), None)
    if p is None:
        p = Pyramid(*key)
        while len(_pyramids) >= PLAN_CACHE_SIZE:
            _pyramids.popitem(last=False)[1].close()
    _pyramids[key + (env,)] = p
    return p
