"""Matrix-free GPU applications of the reference operators (libfoto per-op entry points).

Each function equals ``operators.<builder>(...) @ x`` of the reference (h = 1), computed
by one HIP kernel (operators.py line numbers in include/foto.h).
"""
import ctypes

import numpy as np

from ._lib import FOTO_INV_ITERS_DEFAULT, check, dptr, f64, lib


def grad_st(phi, Nt, Nx, Ny):
    N = Nt * Nx * Ny
    x = f64(phi, N, "phi")
    out = np.empty(3 * N)
    check(lib().foto_grad_st(dptr(x), Nt, Nx, Ny, dptr(out)))
    return out


def div_st(w, Nt, Nx, Ny):
    N = Nt * Nx * Ny
    x = f64(w, 3 * N, "w")
    out = np.empty(N)
    check(lib().foto_div_st(dptr(x), Nt, Nx, Ny, dptr(out)))
    return out


def laplacian_st(p, Nt, Nx, Ny):
    N = Nt * Nx * Ny
    x = f64(p, N, "p")
    out = np.empty(N)
    check(lib().foto_laplacian_st(dptr(x), Nt, Nx, Ny, dptr(out)))
    return out


def apply_A(p, Nt, Nx, Ny, r, eps):
    """(-r L_st + r eps I) @ p  (benamou_brenier.py:202-203)."""
    N = Nt * Nx * Ny
    x = f64(p, N, "p")
    out = np.empty(N)
    check(lib().foto_apply_A(dptr(x), Nt, Nx, Ny, float(r), float(eps), dptr(out)))
    return out


def grad2(f, Nx, Ny, bc="N"):
    x = f64(f, Nx * Ny, "f")
    out = np.empty(2 * Nx * Ny)
    check(lib().foto_grad2(dptr(x), Nx, Ny, _bc(bc), dptr(out)))
    return out


def div2(uv, Nx, Ny, bc="D"):
    x = f64(uv, 2 * Nx * Ny, "uv")
    out = np.empty(Nx * Ny)
    check(lib().foto_div2(dptr(x), Nx, Ny, _bc(bc), dptr(out)))
    return out


def grad2_forward(f, Nx, Ny):
    x = f64(f, Nx * Ny, "f")
    out = np.empty(2 * Nx * Ny)
    check(lib().foto_grad2_forward(dptr(x), Nx, Ny, dptr(out)))
    return out


def stepB(p, M):
    """benamou_brenier.stepB: projection onto {a + |b|^2/2 <= 0} of 3 SoA fields of length M."""
    x = f64(p, 3 * M, "p")
    out = np.empty(3 * M)
    check(lib().foto_stepB(dptr(x), ctypes.c_int64(M), dptr(out)))
    return out


def bb_rhs(mu, q, rho0, rhoT, r, Nt, Nx, Ny):
    """F = div_st(mu - r q) + temporal BC correction (benamou_brenier.py:64-82)."""
    N = Nt * Nx * Ny
    a, b = f64(mu, 3 * N, "mu"), f64(q, 3 * N, "q")
    r0, rT = f64(rho0, Nx * Ny, "rho0"), f64(rhoT, Nx * Ny, "rhoT")
    out = np.empty(N)
    check(lib().foto_bb_rhs(dptr(a), dptr(b), dptr(r0), dptr(rT), Nt, Nx, Ny, float(r), dptr(out)))
    return out


def cg(b, Nt, Nx, Ny, r, eps, rtol=1e-6, maxiter=1000, mode=0):
    """scipy cg on A = -r L_st + r eps I from x0 = 0.  Returns (x, info, iterations)."""
    N = Nt * Nx * Ny
    x_in = f64(b, N, "b")
    x = np.empty(N)
    its = ctypes.c_int(0)
    info = check(lib().foto_cg(dptr(x_in), Nt, Nx, Ny, float(r), float(eps), float(rtol), int(maxiter), int(mode),
                               dptr(x), ctypes.byref(its)))
    return x, info, its.value


def flow_from_phi(phi, Nt, Nx, Ny):
    """utils.opticalflow_from_benamoubrenier (grad bc 'N', div bc 'D')."""
    x = f64(phi, Nt * Nx * Ny, "phi")
    u, v, m = np.empty(Nx * Ny), np.empty(Nx * Ny), np.empty(Nx * Ny)
    check(lib().foto_flow_from_phi(dptr(x), Nt, Nx, Ny, dptr(u), dptr(v), dptr(m)))
    return u, v, m


def flow_path_from_phi(phi, Nt, Nx, Ny):
    """(u, v, m), each [Nt-1, Ny*Nx]: record n-1 is utils.opticalflow_from_benamoubrenier of the
    first n+1 planes of phi (the displacement after n trajectory steps); the last record has the
    bits of ``flow_from_phi``."""
    x = f64(phi, Nt * Nx * Ny, "phi")
    u, v, m = (np.empty((max(Nt - 1, 0), Nx * Ny)) for _ in range(3))
    check(lib().foto_flow_path_from_phi(dptr(x), Nt, Nx, Ny, dptr(u), dptr(v), dptr(m)))
    return u, v, m


def track_from_phi(phi, Nt, Nx, Ny, points, all_steps=True):
    """float64 (R, M, 2): the displacement of each start point (x, y) of ``points`` ((M, 2), or one
    (2,) point) after the first n steps of utils.reconstructTrajectory through grad('N') of phi's
    planes, n = 1..Nt-1 (``all_steps``) or n = Nt-1 only (R = 1).  At pixel centres the records
    have the bits of ``flow_path_from_phi``'s (u, v)."""
    from .device import track_points
    x = f64(phi, Nt * Nx * Ny, "phi")
    pts = track_points(points)
    M = pts.shape[0]
    out = np.empty((max(Nt - 1, 0) if all_steps else 1, M, 2))
    check(lib().foto_track_from_phi(dptr(x), Nt, Nx, Ny, dptr(pts), M, 1 if all_steps else 0, dptr(out)))
    return out


def maps_from_phi(phi, Nt, Nx, Ny, times, inv_iters=FOTO_INV_ITERS_DEFAULT):
    """float64 (K, 4, Ny, Nx): the maps of BBSolver.maps from a caller's phi, without a context --
    per time the planes (a_x - x, a_y - y, b_x - x, b_y - y) of include/foto.h, "maps and
    in-betweens".  ``times``: an int K (np.linspace(0, Nt-1, K)) or a sequence of plane positions."""
    from .device import frame_positions
    x = f64(phi, Nt * Nx * Ny, "phi")
    pos = frame_positions(times, Nt)
    out = np.empty((pos.size, 4, Ny, Nx))
    check(lib().foto_maps_from_phi(dptr(x), Nt, Nx, Ny, dptr(pos), int(pos.size), int(inv_iters), dptr(out)))
    return out


def interp_from_phi(phi, Nt, Nx, Ny, frame0, frame1, times, inv_iters=FOTO_INV_ITERS_DEFAULT):
    """float64 (K, Ny, Nx[, C]): the in-betweens of BBSolver.interpolate from a caller's phi and
    two host frames (Ny, Nx) or (Ny, Nx, C), taken as float64 values (divisor 1)."""
    from .device import frame_positions
    x = f64(phi, Nt * Nx * Ny, "phi")
    a, b = np.asarray(frame0, dtype=np.float64), np.asarray(frame1, dtype=np.float64)
    if a.shape != b.shape or a.ndim not in (2, 3) or a.shape[:2] != (Ny, Nx):
        raise ValueError(f"frames of shape {a.shape} and {b.shape}: both ({Ny}, {Nx}) or ({Ny}, {Nx}, C)")
    C = a.shape[2] if a.ndim == 3 else 1
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    pos = frame_positions(times, Nt)
    out = np.empty((pos.size,) + a.shape)
    check(lib().foto_interp_from_phi(dptr(x), Nt, Nx, Ny, dptr(a), dptr(b), C, dptr(pos), int(pos.size),
                                     int(inv_iters), dptr(out)))
    return out


def report_from_state(mu, phi, rho0, rhoT, Nt, Nx, Ny):
    """The (Nt, 8) table of foto_bb_report from a caller's state, without a context: ``mu`` =
    [rho; m1; m2] and ``phi`` of Nt*Nx*Ny voxels, ``rho0`` / ``rhoT`` of Nx*Ny.  The same kernel,
    so the table has the bits of BBSolver.report() on that state (foto.report has the columns)."""
    from .report import REPORT_COLS
    N = Nt * Nx * Ny
    a, p = f64(mu, 3 * N, "mu"), f64(phi, N, "phi")
    r0, rT = f64(rho0, Nx * Ny, "rho0"), f64(rhoT, Nx * Ny, "rhoT")
    out = np.empty((max(Nt, 0), REPORT_COLS))
    check(lib().foto_report_from_state(dptr(a), dptr(p), dptr(r0), dptr(rT), Nt, Nx, Ny, dptr(out)))
    return out


def _bc(bc):
    if bc not in ("N", "D"):
        raise NotImplementedError("These boundary conditions are not implemented")
    return bc.encode()


def dct(x, axis_len, inner=1, inverse=False, path=0):
    """Orthonormal DCT-II (DCT-III if inverse) along the middle axis of a C-order
    [outer][axis_len][inner] array on the GPU (foto_dct; path 0 auto, 1 FFT, 2 GEMM)."""
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float64)).reshape(-1)
    outer = a.size // (axis_len * inner)
    assert outer * axis_len * inner == a.size
    out = np.empty_like(a)
    check(lib().foto_dct(dptr(a), outer, axis_len, inner, int(bool(inverse)), int(path), dptr(out)))
    return out
