"""Numpy restatement of the duality-based TV-L1 flow with an illumination channel (include/foto.h,
DESIGN.md: Zach, Pock & Bischof 2007; Chambolle & Pock 2011), the yardstick of
tests/test_tvl1_host.py and tests/test_gpu_tvl1.py.  Built on gn_pyr_ref's sizes / down / up /
sample, and nothing else.  Every expression is written in the order the kernels evaluate it."""
import numpy as np

import gn_pyr_ref as G

DEFAULTS = dict(lam=38.0, theta=0.3, tau=0.25, gamma=0.1, levels=4, warps=5, iters=30, min_size=16)


def grad_c(f, w, h):
    """(Gx f, Gy f): central differences, zero in the first and last column / row (bc N)."""
    F = np.asarray(f, dtype=np.float64).reshape(h, w)
    gx, gy = np.zeros((h, w)), np.zeros((h, w))
    gx[:, 1:-1] = 0.5 * (F[:, 2:] - F[:, :-2])
    gy[1:-1, :] = 0.5 * (F[2:, :] - F[:-2, :])
    return gx.ravel(), gy.ravel()


def fwd(a):
    """Forward differences of an (h, w) field, zero in the last column / row."""
    dx, dy = np.zeros_like(a), np.zeros_like(a)
    dx[:, :-1] = a[:, 1:] - a[:, :-1]
    dy[:-1, :] = a[1:, :] - a[:-1, :]
    return dx, dy


def div(px, py):
    """Minus the adjoint of fwd: px[0]; px[i] - px[i-1]; -px[w-2], the same in y, x part + y part."""
    dx, dy = np.empty_like(px), np.empty_like(py)
    dx[:, 0] = px[:, 0]
    dx[:, 1:-1] = px[:, 1:-1] - px[:, :-2]
    dx[:, -1] = -px[:, -2]
    dy[0, :] = py[0, :]
    dy[1:-1, :] = py[1:-1, :] - py[:-2, :]
    dy[-1, :] = -py[-2, :]
    return dx + dy


def coeffs(f1, f2, u, v, w, h, gamma):
    """One warp's (a1, a2, a3, n2, rc) at U0 = (u, v, .)."""
    f1 = np.asarray(f1, dtype=np.float64).ravel()
    u, v = np.asarray(u, dtype=np.float64).ravel(), np.asarray(v, dtype=np.float64).ravel()
    jj, ii = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    x, y = ii.ravel() + u, jj.ravel() + v
    gx, gy = grad_c(f2, w, h)
    g = G.sample(f2, w, h, x, y)
    a1, a2 = G.sample(gx, w, h, x, y), G.sample(gy, w, h, x, y)
    a3 = -gamma * g
    n2 = (a1 * a1 + a2 * a2) + a3 * a3
    rc = ((g - f1) - a1 * u) - a2 * v
    return a1, a2, a3, n2, rc


def dual_step(Ud, Pd, tt):
    """P_d <- (P_d + (tau / theta) fwd(U_d)) / (1 + (tau / theta) |fwd(U_d)|); (h, w) arrays."""
    dx, dy = fwd(Ud)
    den = 1.0 + tt * np.sqrt(dx * dx + dy * dy)
    return (Pd[0] + tt * dx) / den, (Pd[1] + tt * dy) / den


def iterate(co, U, P, w, h, lam, theta, tau, n, perturb=None):
    """n inner iterations: co = (a1, a2, a3, n2, rc), U = 3 fields, P = 6 fields (px, py of u, v,
    w); returns (U, P) as lists of flat arrays.  perturb(size) -> an array added to each channel
    after each iteration (the error-propagation measurement only)."""
    a1, a2, a3, n2, rc = (np.asarray(c, dtype=np.float64).reshape(h, w) for c in co)
    a = (a1, a2, a3)
    U = [np.array(x, dtype=np.float64).reshape(h, w) for x in U]
    P = [np.array(x, dtype=np.float64).reshape(h, w) for x in P]
    lt, tt = lam * theta, tau / theta
    with np.errstate(divide="ignore", invalid="ignore"):
        for _ in range(n):
            rho = ((rc + a1 * U[0]) + a2 * U[1]) + a3 * U[2]
            k = np.where(n2 > 1e-12, -rho / n2, 0.0)
            k = np.where(rho > lt * n2, -lt, k)
            k = np.where(rho < -lt * n2, lt, k)
            for d in range(3):
                U[d] = (U[d] + k * a[d]) + theta * div(P[2 * d], P[2 * d + 1])
                if perturb is not None:
                    U[d] = U[d] + perturb(U[d].size).reshape(h, w)
                P[2 * d], P[2 * d + 1] = dual_step(U[d], (P[2 * d], P[2 * d + 1]), tt)
    return [x.ravel() for x in U], [x.ravel() for x in P]


def level(f1, f2, U, w, h, lam, theta, tau, gamma, warps, iters, perturb=None):
    """One pyramid level from U: P starts at zero and is kept across the warps."""
    P = [np.zeros(w * h) for _ in range(6)]
    for _ in range(warps):
        co = coeffs(f1, f2, U[0], U[1], w, h, gamma)
        U, P = iterate(co, U, P, w, h, lam, theta, tau, iters, perturb)
    return U


def tvl1(f1, f2, w, h, lam=38.0, theta=0.3, tau=0.25, gamma=0.1, levels=4, warps=5, iters=30, min_size=16,
         perturb=None):
    """(u, v, m = gamma w) of the whole scheme."""
    sz = G.sizes(w, h, levels, min_size)
    a, b = [np.asarray(f1, dtype=np.float64).ravel()], [np.asarray(f2, dtype=np.float64).ravel()]
    for (wl, hl) in sz[:-1]:
        a.append(G.down(a[-1], wl, hl))
        b.append(G.down(b[-1], wl, hl))
    U = None
    for l in range(len(sz) - 1, -1, -1):
        wl, hl = sz[l]
        U = [np.zeros(wl * hl) for _ in range(3)] if U is None else list(G.up(*U, *sz[l + 1], wl, hl))
        U = level(a[l], b[l], U, wl, hl, lam, theta, tau, gamma, warps, iters, perturb)
    return U[0], U[1], gamma * U[2]


def interior_epe(u, v, w, h, tu, tv, border=8):
    """Mean endpoint error against the truth (tu, tv) (scalars or fields), `border` pixels off."""
    tu, tv = np.broadcast_to(tu, (h, w)), np.broadcast_to(tv, (h, w))
    e = np.sqrt((np.asarray(u).reshape(h, w) - tu) ** 2 + (np.asarray(v).reshape(h, w) - tv) ** 2)
    return float(e[border:h - border, border:w - border].mean())


# ------------------------------------------------------------------ the quality pairs

def layered_pair():
    """(f1, f2, truth u, truth v): two layers moving (2, 0) and (-2, 1), 96 x 80."""
    from foto.synthetic import textured_pair
    w, h = 96, 80
    b0, b1 = (x.reshape(h, w).copy() for x in textured_pair(w, h, seed=7, dx=2, dy=0, smooth=4))
    g0, g1 = (x.reshape(h, w) for x in textured_pair(w, h, seed=11, dx=-2, dy=1, smooth=4))
    b0[25:55, 30:66] = g0[25:55, 30:66]
    b1[26:56, 28:64] = g1[26:56, 28:64]
    tu, tv = np.full((h, w), 2.0), np.zeros((h, w))
    tu[25:55, 30:66], tv[25:55, 30:66] = -2.0, 1.0
    return b0.ravel(), b1.ravel(), tu, tv


def shift_pair(bright=False):
    """textured_pair(96, 80, seed=5, dx=5, dy=3, smooth=6); bright: frame 1 times a smooth 30 % bump."""
    from foto.synthetic import textured_pair
    w, h = 96, 80
    f1, f2 = textured_pair(w, h, seed=5, dx=5, dy=3, smooth=6)
    if bright:
        jj, ii = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        f2 = (f2.reshape(h, w) * (1 + 0.3 * np.exp(-((ii - 50) ** 2 + (jj - 40) ** 2) / (2 * 15.0 ** 2)))).ravel()
    return f1, f2


# ------------------------------------------------------------------ the whole-solve cases

GAMMAS = (0.0, 0.1)
_cache = {}


def reference(case, gamma):
    """The restatement's (u, v, m) of a gn_pyr_ref case at the defaults and this gamma, computed
    once per process and shared (read-only)."""
    key = (case, float(gamma))
    if key not in _cache:
        w, h = G.CASES[case][:2]
        x = tvl1(*G.frames(case), w, h, gamma=gamma)
        for a in x:
            a.setflags(write=False)
        _cache[key] = x
    return _cache[key]
