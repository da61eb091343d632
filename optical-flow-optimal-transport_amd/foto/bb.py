"""Benamou-Brenier (FOTO) solver on the GPU: Python face of libfoto's BB context.

``solve`` keeps the reference signature and stdout of ``benamou_brenier.solve``
(benamou_brenier.py:151-271): one line ``f"{crit} ({i+1}/{max_it})"`` per outer
iteration (Python ``str`` of a float64), the CG non-convergence warning of
benamou_brenier.py:86-87, and (u, v, m) from the trajectory flow extraction.
"""
import collections
import ctypes
import os
import sys

import numpy as np

from . import _lib
from ._lib import check, dptr, f64, lib

CG_STENCIL = 0
CG_SPECTRAL = 1
CG_SSTEP = 2
CG_GAUSS = 3


def fill_options(L, device, cg_rtol, cg_maxiter, cg_mode, rank, world, nccl_id, virtual_ranks, timing):
    """(foto_bb_opts, the buffer its nccl_id points into or None) -- keep the buffer alive for as
    long as the options are in use."""
    o = _lib.BBOpts()
    L.foto_bb_opts_default(ctypes.byref(o))
    o.device = int(device)
    o.cg_rtol = float(cg_rtol)
    o.cg_maxiter = int(cg_maxiter)
    o.cg_mode = int(cg_mode)
    o.rank = int(rank)
    o.world = int(world)
    idbuf = None
    if nccl_id is not None:
        idbuf = ctypes.create_string_buffer(bytes(nccl_id), 128)
        o.nccl_id = ctypes.cast(idbuf, ctypes.c_void_p)
    o.virtual_ranks = int(virtual_ranks)
    o.timing = 1 if timing else 0
    return o, idbuf


def kernel_stats(st):
    """The ``kernels`` dictionary of a foto_bb_stats: per timed kernel class its launches, ms, bytes."""
    return {name: {"n": int(st.n_k[i]), "ms": float(st.ms_k[i]), "bytes": float(st.bytes_k[i])}
            for i, name in enumerate(_lib.K_NAMES) if st.n_k[i] > 0}


class BBSolver:
    """Device-resident Benamou-Brenier state (mu, q, phi stay in HBM between calls).

    Parameters mirror ``benamou_brenier.solve``; ``cg_mode`` picks the Poisson CG
    (0 = the literal 7-point stencil CG, 1 = the same CG run in the DCT-II eigenbasis of A,
    2 = that spectral CG in s-step passes of up to 8 iterations, 3 = scipy's CG recurrence on
    the Gauss-compressed spectral measure of b -- this class's default --, < 0 = auto, the default
    of the C ABI's foto_bb_opts_default and of the drop-in benamou_brenier.solve: 0 on grids of
    at most 2^18 voxels, 3 above);
    ``rank/world/nccl_id`` shard the time axis over processes (RCCL),
    ``virtual_ranks`` shards it in-process on one device (test path); ``library`` is a
    ``_lib.load``-ed build other than the product libfoto.so (tests).
    """

    def __init__(self, rho0, rhoT, Nt, Nx, Ny, r=1.0, reg_epsilon=1e-3, *, device=-1, cg_rtol=1e-6,
                 cg_maxiter=1000, cg_mode=CG_GAUSS, rank=0, world=1, nccl_id=None, virtual_ranks=1,
                 timing=False, library=None, _device_pair=None):
        self._L = library if library is not None else lib()
        Nt, Nx, Ny = int(Nt), int(Nx), int(Ny)
        if Nt < 2:
            raise ZeroDivisionError("Nt must be >= 2 (benamou_brenier.py:194 divides by Nt - 1)")
        self.Nt, self.Nx, self.Ny = Nt, Nx, Ny
        self.r = float(r)
        self.eps = float(reg_epsilon)
        nxy = Nx * Ny
        o, self._id = fill_options(self._L, device, cg_rtol, cg_maxiter, cg_mode, rank, world, nccl_id, virtual_ranks,
                                   timing)
        self._ctx = ctypes.c_void_p()
        if _device_pair is None:
            self._rho0 = f64(rho0, nxy, "rho0")
            self._rhoT = f64(rhoT, nxy, "rhoT")
            self._check(self._L.foto_bb_create(dptr(self._rho0), dptr(self._rhoT), Nt, Nx, Ny, self.r, self.eps,
                                       ctypes.byref(o), ctypes.byref(self._ctx)))
        else:   # from_device: the two frames are foto_image descriptors of device memory
            a, b, normalize, stream = _device_pair
            sums = np.zeros(2)
            self._check(self._L.foto_bb_create_dev(ctypes.byref(a), ctypes.byref(b), 1 if normalize else 0,
                                                   ctypes.c_void_p(stream), Nt, Nx, Ny, self.r, self.eps,
                                                   ctypes.byref(o), dptr(sums), ctypes.byref(self._ctx)))
            self.sums = (float(sums[0]), float(sums[1]))
        self.world = int(world)
        self.rank = int(rank)
        self._clear_log()

    def _clear_log(self):
        """the per-iteration record of a run: empty on a new or reset context"""
        self.crit = []
        self.cg_its = []
        self.cg_info = []

    # -------------------------------------------------------------- device buffers
    @classmethod
    def from_device(cls, f0, f1, Nt, r=1.0, reg_epsilon=1e-3, *, normalize=False, stream=None, **opts):
        """A solver on two device frames (anything foto.device.as_image accepts: torch ROCm
        tensors, DeviceArrays, strided views; uint8 / float32 / float64, value = pixel / divisor):
        foto_bb_create_dev.  The context is in the state the host constructor leaves for the same
        values, so the solve is bit-identical.  ``normalize`` divides each frame by its own sum
        (main.py:71-74); ``self.sums`` holds the two sums ((1, 1) without).  ``stream``: the
        caller's stream (foto.device.stream_handle); the frames may be overwritten by work queued
        on it as soon as this returns."""
        from . import device as D
        a, b = D._pair(f0, f1)
        h, w = a.shape
        st = D.stream_handle(stream, f0, f1)
        return cls(None, None, Nt, w, h, r=r, reg_epsilon=reg_epsilon, _device_pair=(a, b, normalize, st), **opts)

    def reset_device(self, f0, f1, *, normalize=False, stream=None):
        """reset() on two device frames (foto_bb_reset_dev)."""
        from . import device as D
        a, b = D._pair(f0, f1)
        if a.shape != (self.Ny, self.Nx):
            raise ValueError(f"frames of shape {a.shape}; this solver was made for {(self.Ny, self.Nx)}")
        sums = np.zeros(2)
        self._check(self._L.foto_bb_reset_dev(self._ctx, ctypes.byref(a), ctypes.byref(b), 1 if normalize else 0,
                                              ctypes.c_void_p(D.stream_handle(stream, f0, f1)), dptr(sums)))
        self.sums = (float(sums[0]), float(sums[1]))
        self._clear_log()

    def flow_device(self, out=None, dtype="float32", layout="planar", stream=None):
        """flow() left on the device (foto_bb_flow_dev): a DeviceArray (or ``out``, any
        contiguous device array of that shape and dtype) of ``dtype`` float32 | float64, ``layout``
        "planar" [3][Ny][Nx] = u, v, m or "interleaved" [Ny][Nx][2] = (u, v), the .flo payload."""
        from . import device as D
        out, ptr, dcode, lcode = D.export_target(out, dtype, layout, self.Ny, self.Nx)
        self._check(self._L.foto_bb_flow_dev(self._ctx, ctypes.c_void_p(ptr), dcode, lcode,
                                             ctypes.c_void_p(D.stream_handle(stream, out))))
        return out

    # -------------------------------------------------------------- transport path
    def frames(self, s, scale=1.0):
        """Density frames [K, Ny, Nx] (float64, host) at plane positions ``s`` in [0, Nt-1] (an
        int K: np.linspace(0, Nt-1, K)): scale * ((1 - w) rho_n + w rho_{n+1}) of the last
        completed outer iteration's mu (before any: the linear initial path) -- foto_bb_frames.
        An integer position with scale 1 is plane n bit for bit."""
        from . import device as D
        pos = D.frame_positions(s, self.Nt)
        out = np.empty((pos.size, self.Ny, self.Nx))
        self._check(self._L.foto_bb_frames(self._ctx, dptr(pos), int(pos.size), float(scale), dptr(out)))
        return out

    def frames_device(self, s, scale=1.0, out=None, dtype="float32", stream=None):
        """frames() left on the device (foto_bb_frames_dev): a DeviceArray (or ``out``, any
        contiguous device array) [K][Ny][Nx] of ``dtype`` uint8 | float32 | float64; uint8 is
        255 * clip(x, 0, 1) rounded to nearest."""
        from . import device as D
        pos = D.frame_positions(s, self.Nt)
        out, ptr, dcode = D.frames_target(out, dtype, pos.size, self.Ny, self.Nx)
        self._check(self._L.foto_bb_frames_dev(self._ctx, dptr(pos), int(pos.size), float(scale),
                                               ctypes.c_void_p(ptr), dcode,
                                               ctypes.c_void_p(D.stream_handle(stream, out))))
        return out

    def flow_path(self):
        """(u, v, m), each [Nt-1, Ny*Nx]: record n-1 is the flow after the first n trajectory
        steps (flow() of the first n+1 planes of phi); the last record is flow()'s result."""
        nxy = self.Nx * self.Ny
        u, v, m = (np.empty((self.Nt - 1, nxy)) for _ in range(3))
        self._check(self._L.foto_bb_flow_path(self._ctx, dptr(u), dptr(v), dptr(m)))
        return u, v, m

    def flow_path_device(self, out=None, dtype="float32", layout="planar", stream=None):
        """flow_path() left on the device (foto_bb_flow_path_dev): Nt - 1 records laid out as
        flow_device lays out its one, [Nt-1][3][Ny][Nx] or [Nt-1][Ny][Nx][2]."""
        from . import device as D
        out, ptr, dcode, lcode = D.path_target(out, dtype, layout, self.Nt, self.Ny, self.Nx)
        self._check(self._L.foto_bb_flow_path_dev(self._ctx, ctypes.c_void_p(ptr), dcode, lcode,
                                                  ctypes.c_void_p(D.stream_handle(stream, out))))
        return out

    def track(self, points, all_steps=True):
        """Trajectories of arbitrary start points (foto_bb_track): ``points`` is anything
        np.asarray turns into (M, 2) = (x, y) in pixel-index coordinates (pixel (i, j) has centre
        (i, j), x along Nx; sub-pixel and out-of-frame values allowed), a single (2,) point is
        M = 1.  Returns float64 (R, M, 2): record n-1 is the displacement after the first n steps
        of utils.reconstructTrajectory, R = Nt-1 (``all_steps``) or 1 (the last record).  At
        pixel centres the records have the bits of flow_path()'s (u, v)."""
        from . import device as D
        pts = D.track_points(points)
        M = pts.shape[0]
        out = np.empty((self.Nt - 1 if all_steps else 1, M, 2))
        self._check(self._L.foto_bb_track(self._ctx, dptr(pts), M, 1 if all_steps else 0, dptr(out)))
        return out

    def track_device(self, points, out=None, dtype="float32", all_steps=True, stream=None):
        """track() on the device (foto_bb_track_dev): ``points`` is a C-contiguous (M, 2) float32
        | float64 device array, the result a DeviceArray (or ``out``, any contiguous device array)
        [R][M][2] of ``dtype`` float32 | float64.  Positions are float64 inside whatever the
        dtypes."""
        from . import device as D
        pptr, pcode, M = D.track_source(points)
        out, ptr, dcode = D.track_target(out, dtype, self.Nt - 1 if all_steps else 1, M)
        self._check(self._L.foto_bb_track_dev(self._ctx, ctypes.c_void_p(pptr), pcode, M, 1 if all_steps else 0,
                                              ctypes.c_void_p(ptr), dcode,
                                              ctypes.c_void_p(D.stream_handle(stream, out, points))))
        return out

    # -------------------------------------------------------------- maps and in-betweens
    def maps(self, times, inv_iters=_lib.FOTO_INV_ITERS_DEFAULT):
        """The transport read from plane positions ``times`` in [0, Nt-1] (an int K:
        np.linspace(0, Nt-1, K)) in both directions (foto_bb_maps): float64 (K, 4, Ny, Nx), per
        time the planes (a_x - x, a_y - y, b_x - x, b_y - y) -- the pixel of the time-s image at
        (x, y) came from a in frame 0 and goes to b in frame 1.  At time 0 the b-planes are
        flow()'s (u, v) bit for bit; at Nt-1 the negated a-planes are the backward flow, frame 1
        to frame 0.  ``inv_iters`` (1..64): rounds of the fixed-count inverse step."""
        from . import device as D
        pos = D.frame_positions(times, self.Nt)
        out = np.empty((pos.size, 4, self.Ny, self.Nx))
        self._check(self._L.foto_bb_maps(self._ctx, dptr(pos), int(pos.size), int(inv_iters), dptr(out)))
        return out

    def maps_device(self, times, inv_iters=_lib.FOTO_INV_ITERS_DEFAULT, out=None, dtype="float32", stream=None):
        """maps() left on the device (foto_bb_maps_dev): a DeviceArray (or ``out``, any contiguous
        device array) [K][4][Ny][Nx] of ``dtype`` float32 | float64."""
        from . import device as D
        pos = D.frame_positions(times, self.Nt)
        out, ptr, dcode = D.maps_target(out, dtype, pos.size, self.Ny, self.Nx)
        self._check(self._L.foto_bb_maps_dev(self._ctx, dptr(pos), int(pos.size), int(inv_iters), ctypes.c_void_p(ptr),
                                             dcode, ctypes.c_void_p(D.stream_handle(stream, out))))
        return out

    def interpolate(self, frame0, frame1, times, inv_iters=_lib.FOTO_INV_ITERS_DEFAULT, dtype=None, out=None,
                    stream=None, channels_last=True, divisor=None):
        """Motion-compensated in-betweens of the caller's own frames (foto_bb_interp_dev): per
        channel (1 - w) S(frame0; a) + w S(frame1; b), w = s / (Nt-1), along maps()'s a and b.
        ``frame0`` / ``frame1``: two numpy arrays (Ny, Nx) or (Ny, Nx, C) -- uploaded, the result
        downloaded -- or two device arrays ((C, Ny, Nx) with ``channels_last=False``), the result
        left on the device: (K, Ny, Nx[, C]) of ``dtype`` uint8 | float32 | float64 (None: the
        frames' own; numpy frames of another dtype go through float64).  Values are pixel /
        ``divisor`` (255 for uint8 frames, 1 otherwise); uint8 output is 255 clip(x, 0, 1) rounded
        to nearest.  Times 0 and Nt-1 give the two frames back bit for bit."""
        from . import device as D
        host = not (hasattr(frame0, "__cuda_array_interface__") or isinstance(frame0, dict))
        if host:
            def up(f):
                a = np.asarray(f)
                if a.dtype not in (np.uint8, np.float32, np.float64):
                    a = a.astype(np.float64)
                return D.DeviceArray.from_numpy(a)
            frame0, frame1 = up(frame0), up(frame1)
        a, b, C, sc0, sc1, has_c, own = D.interp_frames(frame0, frame1, channels_last, divisor)
        if a.shape != (self.Ny, self.Nx):
            raise ValueError(f"frames of shape {a.shape}; this solver was made for {(self.Ny, self.Nx)}")
        pos = D.frame_positions(times, self.Nt)
        out, ptr, dcode = D.interp_target(out, own if dtype is None else dtype, pos.size, self.Ny, self.Nx, C, has_c)
        self._check(self._L.foto_bb_interp_dev(self._ctx, ctypes.byref(a), ctypes.byref(b), C, sc0, sc1, dptr(pos),
                                               int(pos.size), int(inv_iters), ctypes.c_void_p(ptr), dcode,
                                               ctypes.c_void_p(D.stream_handle(stream, out, frame0, frame1))))
        return out.to_numpy() if host else out

    # -------------------------------------------------------------- transport report
    def report(self):
        """The TransportReport (foto.report) of the last completed outer iteration: per time
        plane the mass, action, vacuum momentum, continuity and Hamilton-Jacobi residual sums
        (foto_bb_report), one 64 Nt-byte download.  State rules of flow_path()."""
        from .report import REPORT_COLS, TransportReport
        out = np.empty((self.Nt, REPORT_COLS))
        self._check(self._L.foto_bb_report(self._ctx, dptr(out)))
        return TransportReport(out, self.Nt, self.Nx, self.Ny)

    def report_device(self, out=None, stream=None):
        """report()'s table left on the device (foto_bb_report_dev): a DeviceArray (or ``out``,
        any C-contiguous device array) (Nt, 8) float64, without a host synchronisation."""
        from . import device as D
        out, ptr = D.report_target(out, self.Nt)
        self._check(self._L.foto_bb_report_dev(self._ctx, ctypes.c_void_p(ptr),
                                               ctypes.c_void_p(D.stream_handle(stream, out))))
        return out

    def _check(self, rc):
        return check(rc, self._L)

    def reset(self, rho0, rhoT):
        """Start over on a new pair of the same size: the context's fields, CG state and
        predictions go back to what construction leaves (foto_bb_reset), so the solve is
        bit-identical to one on a fresh BBSolver, without its allocations and plans."""
        nxy = self.Nx * self.Ny
        self._rho0 = f64(rho0, nxy, "rho0")
        self._rhoT = f64(rhoT, nxy, "rhoT")
        self._check(self._L.foto_bb_reset(self._ctx, dptr(self._rho0), dptr(self._rhoT)))
        self._clear_log()

    # -------------------------------------------------------------- lifecycle
    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._L.foto_bb_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        if sys.is_finalizing():   # libfoto / HIP may already be torn down
            return
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -------------------------------------------------------------- iterations
    def iterate(self, n, convergence_tol=0.0, stop_rules=True, callback=None):
        """Run up to n outer iterations; returns True if a reference stop rule fired.
        ``callback(i, crit, cg_its, cg_info)`` is called after each iteration, while iteration
        i + 1 is already on the stream: in the default single-GPU loop ``phi()``, ``state()``
        and ``flow()`` called from it return iteration i's results; the one-in-flight loop
        (sharded contexts, FOTO_PIPE=0) raises FotoError for them there (foto.h)."""
        errors = []

        def _cb(user, it, crit, its, info):
            try:
                self.crit.append(crit)
                self.cg_its.append(its)
                self.cg_info.append(info)
                if callback is not None:
                    callback(it, crit, its, info)
            except BaseException as e:   # never let an exception unwind through C
                errors.append(e)

        cb = _lib.ITER_CB(_cb)
        done = ctypes.c_int(0)
        rc = self._L.foto_bb_iterate(self._ctx, int(n), float(convergence_tol), 1 if stop_rules else 0, cb, None,
                                   ctypes.byref(done))
        if errors:
            raise errors[0]
        self._check(rc)
        return rc == 1

    def flow(self):
        """(u, v, m) from the last phi (rank 0 gets the arrays; other ranks get None)."""
        nxy = self.Nx * self.Ny
        if self.world > 1 and self.rank != 0:
            self._check(self._L.foto_bb_flow(self._ctx, None, None, None))
            return None
        u = np.empty(nxy)
        v = np.empty(nxy)
        m = np.empty(nxy)
        self._check(self._L.foto_bb_flow(self._ctx, dptr(u), dptr(v), dptr(m)))
        return u, v, m

    def shard(self):
        t0 = ctypes.c_int()
        nl = ctypes.c_int()
        self._check(self._L.foto_bb_shard(self._ctx, ctypes.byref(t0), ctypes.byref(nl)))
        return t0.value, nl.value

    def comm_size(self):
        """Ranks of this context's RCCL communicator (ncclCommCount); 0 without one."""
        n = ctypes.c_int()
        self._check(self._L.foto_bb_comm_size(self._ctx, ctypes.byref(n)))
        return n.value

    def phi(self):
        _, nl = self.shard()
        out = np.empty(nl * self.Nx * self.Ny)
        self._check(self._L.foto_bb_get_phi(self._ctx, dptr(out)))
        return out

    def state(self):
        _, nl = self.shard()
        n = nl * self.Nx * self.Ny
        mu = np.empty(3 * n)
        q = np.empty(3 * n)
        self._check(self._L.foto_bb_get_state(self._ctx, dptr(mu), dptr(q)))
        return mu, q

    def stats(self):
        st = _lib.BBStats()
        self._check(self._L.foto_bb_stats_get(self._ctx, ctypes.byref(st)))
        d = {f: getattr(st, f) for f in ("outer_iters", "cg_iters_total", "last_crit", "ms_rhs", "ms_cg",
                                         "ms_prox", "ms_flow", "cg_redo")}
        d["kernels"] = kernel_stats(st)
        return d

    def reset_stats(self):
        self._check(self._L.foto_bb_stats_reset(self._ctx))

    def set_timing(self, on):
        self._check(self._L.foto_bb_set_timing(self._ctx, 1 if on else 0))

    def sync(self):
        self._check(self._L.foto_bb_sync(self._ctx))


# One context per (size, parameters) for a batch of same-size frames (run.sh:81-157 solves one
# pair per sequence): a context costs its HBM fields, DCT plans and a stream to build, and
# foto_bb_reset makes a reused one give the same bits as a fresh one.  FOTO_BB_CACHE=0 turns
# it off; sharded contexts (RCCL rank/world) and explicit libraries are never cached.
CONTEXT_CACHE_SIZE = 2
_ctx_cache = collections.OrderedDict()


def _cache_enabled(opts):
    if os.environ.get("FOTO_BB_CACHE", "1") == "0" or CONTEXT_CACHE_SIZE <= 0:
        return False
    return (opts.get("library") is None and opts.get("nccl_id") is None
            and int(opts.get("world", 1)) == 1)


def _cached(Nt, Nx, Ny, r, reg_epsilon, opts, reset, make):
    """The cache walk: the context of this size and these options taken out and ``reset(s)``, or
    ``make()``; put back as the most recently used, the least recently used beyond
    CONTEXT_CACHE_SIZE destroyed."""
    # FOTO_* tuning variables are read when a context is built: part of its identity
    env = tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("FOTO_")))
    key = (int(Nt), int(Nx), int(Ny), float(r), float(reg_epsilon), tuple(sorted(opts.items())), env)
    s = _ctx_cache.pop(key, None)
    if s is not None:
        reset(s)
    else:
        s = make()
    _ctx_cache[key] = s
    while len(_ctx_cache) > CONTEXT_CACHE_SIZE:
        _ctx_cache.popitem(last=False)[1].close()
    return s


def cached_solver(rho0, rhoT, Nt, Nx, Ny, r, reg_epsilon, **opts):
    """A BBSolver for this size and these options, reset to (rho0, rhoT): reused from the
    cache when one exists, else created (the least recently used context beyond
    CONTEXT_CACHE_SIZE is destroyed)."""
    return _cached(Nt, Nx, Ny, r, reg_epsilon, opts, lambda s: s.reset(rho0, rhoT),
                   lambda: BBSolver(rho0, rhoT, Nt, Nx, Ny, r=r, reg_epsilon=reg_epsilon, **opts))


def cached_solver_device(f0, f1, Nt, r, reg_epsilon, *, normalize=False, stream=None, **opts):
    """cached_solver for two device frames (the same cache: a context serves host and device
    pairs alike)."""
    from . import device as D
    a, b = D._pair(f0, f1)
    h, w = a.shape
    return _cached(Nt, w, h, r, reg_epsilon, opts, lambda s: s.reset_device(a, b, normalize=normalize, stream=stream),
                   lambda: BBSolver.from_device(a, b, Nt, r=r, reg_epsilon=reg_epsilon, normalize=normalize,
                                                stream=stream, **opts))


def drop_cached(s):
    """Forget and close a cached solver (after a failed solve: no half-used context stays)."""
    for k, v in list(_ctx_cache.items()):
        if v is s:
            del _ctx_cache[k]
    s.close()


def on_context(opts, cached, fresh, run):
    """``run(s)`` on the context ``cached()`` returns -- a failed run leaves no half-used context
    behind: it is forgotten and closed -- or, where these options are not cached, on ``fresh()``,
    closed afterwards."""
    if _cache_enabled(opts):
        s = cached()
        try:
            return run(s)
        except BaseException:
            drop_cached(s)
            raise
    with fresh() as s:
        return run(s)


def clear_context_cache():
    while _ctx_cache:
        _ctx_cache.popitem()[1].close()


def solve(rho0, rhoT, Nt, Nx, Ny, r=1, convergence_tol=0.3, reg_epsilon=1e-3, max_it=100, *, log=print,
          stats=None, then=None, **opts):
    """benamou_brenier.solve on the GPU.  Returns (u, v, m).  ``then(solver)``: called on the
    solved context after the flow extraction, while it still holds this pair's transport (the
    exports of the path: frames, maps, in-betweens); its result is dropped."""
    if max_it <= 0:
        # reference: the loop body never runs and `phi` is unbound at benamou_brenier.py:271
        raise UnboundLocalError("cannot access local variable 'phi' where it is not associated with a value")

    def cb(it, crit, its, info):
        if info > 0:
            log(f"WARNING: CG did not converge in {info} iterations.")
        log(str(np.float64(crit)) + " (" + str(it + 1) + "/" + str(max_it) + ")")

    return on_context(opts, lambda: cached_solver(rho0, rhoT, Nt, Nx, Ny, r, reg_epsilon, **opts),
                      lambda: BBSolver(rho0, rhoT, Nt, Nx, Ny, r=r, reg_epsilon=reg_epsilon, **opts),
                      lambda s: _run(s, max_it, convergence_tol, cb, stats, then))


def solve_ex(rho0, rhoT, Nt, Nx, Ny, r=1, convergence_tol=0.3, reg_epsilon=1e-3, max_it=100, *, cap=None,
             want_phi=True, device=-1, cg_mode=CG_GAUSS, cg_rtol=1e-6, cg_maxiter=1000, rank=0, world=1,
             nccl_id=None, virtual_ranks=1, timing=False, library=None):
    """benamou_brenier.solve through the one-shot C entry foto_bb_solve_ex (include/foto.h; the
    SURVEY.md §8(b) boundary): a context made, iterated with the reference's stop rules, the flow
    extracted and the context destroyed in one call.  Returns (u, v, m, report): report holds the
    per-outer-iteration crit / cg_its / cg_info (the first ``cap`` of them, default max_it), phi
    (this rank's slab) and the timings and byte counts of foto_bb_solve_stats.  With world > 1
    every rank calls it; (u, v, m) are None off rank 0."""
    L = library if library is not None else lib()
    Nt, Nx, Ny = int(Nt), int(Nx), int(Ny)
    nxy = Nx * Ny
    a0, aT = f64(rho0, nxy, "rho0"), f64(rhoT, nxy, "rhoT")
    # (idbuf: what o.nccl_id points into, alive until the call below has returned)
    o, idbuf = fill_options(L, device, cg_rtol, cg_maxiter, cg_mode, rank, world, nccl_id, virtual_ranks, timing)
    cap = int(max_it if cap is None else cap)
    crit = np.zeros(max(cap, 1))
    its = np.zeros(max(cap, 1), dtype=np.int32)
    info = np.zeros(max(cap, 1), dtype=np.int32)
    st = _lib.BBSolveStats()
    st.cap = cap
    st.crit = dptr(crit)
    st.cg_its = its.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    st.cg_info = info.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    on0 = int(world) == 1 or int(rank) == 0
    u, v, m = (np.empty(nxy) for _ in range(3)) if on0 else (None, None, None)
    # the largest slab a rank can hold (split_planes: balanced), or every plane on one GPU
    phi = np.empty(-(-Nt // max(int(world), 1)) * nxy) if want_phi else None
    null = _lib._D()
    check(L.foto_bb_solve_ex(dptr(a0), dptr(aT), Nt, Nx, Ny, float(r), float(convergence_tol), float(reg_epsilon),
                             int(max_it), ctypes.byref(o), dptr(u) if on0 else null, dptr(v) if on0 else null,
                             dptr(m) if on0 else null, dptr(phi) if want_phi else null, ctypes.byref(st)), L)
    n = min(st.outer_iters, cap)
    rep = {"outer_iters": st.outer_iters, "stopped": bool(st.stopped), "crit": crit[:n].copy(),
           "cg_its": its[:n].astype(np.int64), "cg_info": info[:n].astype(np.int64),
           "phi_t0": st.phi_t0, "phi_nloc": st.phi_nloc, "ms_create": st.ms_create, "ms_loop": st.ms_loop,
           "ms_flow": st.ms_flow, "alg_bytes_per_iter": st.alg_bytes_per_iter,
           "cg_iters_total": int(st.bb.cg_iters_total), "cg_redo": int(st.bb.cg_redo),
           "kernels": kernel_stats(st.bb)}
    if want_phi:
        rep["phi"] = phi[:st.phi_nloc * nxy].copy()
    return u, v, m, rep


def _run(s, max_it, convergence_tol, cb, stats, then=None):
    s.iterate(max_it, convergence_tol=convergence_tol, stop_rules=True, callback=cb)
    out = s.flow()
    if then is not None:
        then(s)
    if stats is not None:
        stats.update(crit=np.array(s.crit), cg_its=np.array(s.cg_its), cg_info=np.array(s.cg_info),
                     phi=s.phi(), **s.stats())
    return out
