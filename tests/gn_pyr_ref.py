"""Numpy restatement of the coarse-to-fine GN scheme (include/foto.h), the yardstick of
tests/test_gn_pyr_host.py and tests/test_gpu_gn_pyr.py.  Built on the oracle's gn_assemble and
gn_neg_lap and scipy's spsolve, and nothing else."""
import numpy as np
from scipy.sparse.linalg import spsolve

from oracle import foto_oracle as O


def sizes(w, h, levels, min_size=16):
    out = [(w, h)]
    while len(out) < levels and min(out[-1]) >= 2 * min_size:
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def down(f, w, h):
    F = np.asarray(f, dtype=np.float64).reshape(h, w)
    wc, hc = (w + 1) // 2, (h + 1) // 2
    I0, J0 = 2 * np.arange(wc), 2 * np.arange(hc)
    I1, J1 = np.minimum(I0 + 1, w - 1), np.minimum(J0 + 1, h - 1)
    c = 0.25 * (((F[np.ix_(J0, I0)] + F[np.ix_(J0, I1)]) + F[np.ix_(J1, I0)]) + F[np.ix_(J1, I1)])
    return c.ravel()


def sample(f, w, h, x, y):
    """S(f; x, y); a NaN coordinate gives NaN."""
    F = np.asarray(f, dtype=np.float64).reshape(h, w)
    bad = np.isnan(x) | np.isnan(y)
    xc = np.clip(np.where(bad, 0.0, x), 0, w - 1)
    yc = np.clip(np.where(bad, 0.0, y), 0, h - 1)
    i0 = np.minimum(np.floor(xc).astype(np.int64), w - 2)
    j0 = np.minimum(np.floor(yc).astype(np.int64), h - 2)
    ax, ay = xc - i0, yc - j0
    val = ((1 - ay) * ((1 - ax) * F[j0, i0] + ax * F[j0, i0 + 1])
           + ay * ((1 - ax) * F[j0 + 1, i0] + ax * F[j0 + 1, i0 + 1]))
    return np.where(bad, np.nan, val)


def up(u, v, m, wc, hc, w, h):
    jj, ii = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    x = ((ii + 0.5) * wc / w - 0.5).ravel()
    y = ((jj + 0.5) * hc / h - 0.5).ravel()
    return (w / wc) * sample(u, wc, hc, x, y), (h / hc) * sample(v, wc, hc, x, y), sample(m, wc, hc, x, y)


def warp(f2, u, v, m, w, h):
    jj, ii = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    return (1 - np.asarray(m)) * sample(f2, w, h, ii.ravel() + u, jj.ravel() + v)


def system(f1, g, w, h, alpha, lam, prior=None):
    """(A, b) of one increment solve: A(f1, g), b(f1, g) - [alpha N u; alpha N v; lambda N m]."""
    A, b = O.gn_assemble(f1, g, w, h, alpha, lam)
    if prior is not None:
        u, v, m = prior
        b = b - np.concatenate([alpha * O.gn_neg_lap(u, w, h), alpha * O.gn_neg_lap(v, w, h),
                                lam * O.gn_neg_lap(m, w, h)])
    return A, b


def solve_inc(f1, g, w, h, alpha, lam, prior=None, perturb=None):
    """The total flow after one increment solve."""
    n = w * h
    A, b = system(f1, g, w, h, alpha, lam, prior)
    d = spsolve(A, b)   # (A as gn_assemble returns it, like the oracle's gn_solve)
    if perturb is not None:
        d = d + perturb(d.size)
    d = (d[:n], d[n:2 * n], d[2 * n:])
    return d if prior is None else tuple(p + q for p, q in zip(prior, d))


def pyramid(f1, f2, w, h, alpha, lam, levels, warps, min_size=16, perturb=None):
    sz = sizes(w, h, levels, min_size)
    a, b = [np.asarray(f1, dtype=np.float64).ravel()], [np.asarray(f2, dtype=np.float64).ravel()]
    for (wl, hl) in sz[:-1]:
        a.append(down(a[-1], wl, hl))
        b.append(down(b[-1], wl, hl))
    x = None
    for l in range(len(sz) - 1, -1, -1):
        wl, hl = sz[l]
        if x is not None:
            x = up(*x, *sz[l + 1], wl, hl)
        for _ in range(warps):
            g = b[l] if x is None else warp(b[l], *x, wl, hl)
            x = solve_inc(a[l], g, wl, hl, alpha, lam, x, perturb)
    return x


def interior_epe(u, v, w, h, dx, dy, border=10):
    e = np.sqrt((np.asarray(u) - dx) ** 2 + (np.asarray(v) - dy) ** 2).reshape(h, w)
    return float(e[border:h - border, border:w - border].mean())


# the issue's cases: (w, h, (dx, dy), smooth, levels, warps), frames from textured_pair(seed=5)
CASES = {
    "96x80": (96, 80, (5.0, 3.0), 6, 3, 3),
    "71x77": (71, 77, (4.0, -3.0), 6, 3, 2),
    "45x37": (45, 37, (3.0, 2.0), 4, 2, 2),
}
ALPHA, LAM = 0.1, 0.2


def frames(case):
    from foto.synthetic import textured_pair
    w, h, (dx, dy), smooth, levels, warps = CASES[case]
    return textured_pair(w, h, seed=5, dx=dx, dy=dy, smooth=smooth)


_cache = {}


def reference(case):
    """The restatement's flow of a case, computed once per process and shared (read-only)."""
    if case not in _cache:
        w, h, _, _, levels, warps = CASES[case]
        f1, f2 = frames(case)
        x = pyramid(f1, f2, w, h, ALPHA, LAM, levels, warps)
        for a in x:
            a.setflags(write=False)
        _cache[case] = x
    return _cache[case]
