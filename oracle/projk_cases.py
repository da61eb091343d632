"""The input regimes of the stepB / project_K envelope tests (tests/test_projk_exact_host.py on
the CPU, tests/test_gpu_projk.py on the device): fixed seeds, 3 SoA float64 fields per regime
in ``foto_oracle.stepB``'s layout.  Point counts are deliberately no multiple of the 256-thread
block; M = 1, 255 and 257 appear once each.

Inputs from 1e100 upward are out of scope: the reference's own a^3 overflows there.
"""
import numpy as np

SCALES = (1e-12, 1e-8, 1e-4, 1e-2, 1e2, 1e4, 1e8, 1e50)
DELTAS = (1e-3, 1e-8, 1e-13)
SEAM_ULPS = (0, 1, -1, 2, -2, 4, -4)
SEAM_RELS = (1e-9, -1e-9, 1e-3, -1e-3)
SEAM_M = 301


def _soa(a, b1, b2):
    return np.concatenate([np.asarray(a, dtype=np.float64), np.asarray(b1, dtype=np.float64),
                           np.asarray(b2, dtype=np.float64)])


def _ulps(x, k):
    to = np.inf if k > 0 else -np.inf
    for _ in range(abs(k)):
        x = np.nextafter(x, to)
    return x


def seam_points(rng, M):
    """a = -1 - U(3, 40) and rho on the branch seam 32 (a + 1)^3 + 108 rho^2 = 0, to the
    nearest double of the float64 evaluation."""
    a = -1.0 - rng.uniform(3.0, 40.0, M)
    ap1 = a + 1.0
    return a, np.sqrt(-8.0 / 27.0 * (ap1 * ap1 * ap1))


def seam_regimes():
    """name -> (p, M): rho moved off the seam by k ulps and by relative amounts, once rotated by
    a random angle and once axis-aligned (b2 = 0: the kernel's rho is then the given double)."""
    out = {}
    rng = np.random.default_rng(950)
    a, rho = seam_points(rng, SEAM_M)
    th = rng.uniform(-np.pi, np.pi, SEAM_M)
    moved = [(f"{k:+d}ulp", _ulps(rho, k)) for k in SEAM_ULPS] + [(f"rel{r:+.0e}", rho * (1.0 + r)) for r in SEAM_RELS]
    for tag, rh in moved:
        out[f"seam_axis_{tag}"] = (_soa(a, rh, np.zeros(SEAM_M)), SEAM_M)
        out[f"seam_rot_{tag}"] = (_soa(a, rh * np.cos(th), rh * np.sin(th)), SEAM_M)
    return out


def axis_points():
    """rho = 0 and a > 0 (every point projects onto the apex 0), under all four signs of the
    zeros (b1, b2): (a, b1, b2) arrays."""
    rng = np.random.default_rng(31)
    a = np.concatenate([10.0 ** rng.uniform(-300.0, -1.0, 40), np.abs(3.0 * rng.standard_normal(40)) + 1e-3,
                        10.0 ** rng.uniform(0.0, 8.0, 20), [0.5, 1.0, 2.0, 3.0, 1e-320]])
    n = a.size
    z1 = np.concatenate([np.full(n, s) for s in (0.0, 0.0, -0.0, -0.0)])
    z2 = np.concatenate([np.full(n, s) for s in (0.0, -0.0, 0.0, -0.0)])
    return np.tile(a, 4), z1, z2


def boundary_points():
    """Points exactly on the boundary of K, from small integers (all arithmetic exact)."""
    b1, b2 = (v.ravel().astype(np.float64) for v in np.meshgrid(np.arange(-6, 7), np.arange(-6, 7)))
    b1 = np.concatenate([[1.0, 0.0, 3.0], b1])
    b2 = np.concatenate([[0.0, 2.0, 4.0], b2])
    a = -(b1 * b1 + b2 * b2) / 2.0
    # the apex under every sign of its zeros, and signed zeros beside a nonzero component
    z = [(sa, s1, s2) for sa in (0.0, -0.0) for s1 in (0.0, -0.0) for s2 in (0.0, -0.0)]
    z += [(-1.0, -0.0, 0.0), (-1.0, 0.0, -0.0), (-0.5, -0.0, 1.0), (-0.5, -1.0, -0.0)]
    za, z1, z2 = (np.array(v) for v in zip(*z))
    return np.concatenate([a, za]), np.concatenate([b1, z1]), np.concatenate([b2, z2])


def plain_regimes():
    """name -> (p, M): every regime away from the branch seam."""
    out = {}
    rng = np.random.default_rng(7)
    for name, M in (("normal3", 1999), ("normal3_M1", 1), ("normal3_M255", 255), ("normal3_M257", 257)):
        out[name] = (3.0 * rng.standard_normal(3 * M), M)
    for k, s in enumerate(SCALES):
        M = 601 + 2 * k
        out[f"scale_{s:.0e}"] = (s * rng.standard_normal(3 * M), M)
    M = 1501
    out["mixed"] = (np.where(rng.random(3 * M) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-6.0, 6.0, 3 * M), M)
    for d in DELTAS:
        M = 701
        b1, b2 = 3.0 * rng.standard_normal(M), 3.0 * rng.standard_normal(M)
        r2 = b1 * b1 + b2 * b2
        out[f"near_{d:.0e}"] = (_soa(-r2 / 2.0 + d * (1.0 + r2), b1, b2), M)
    a, b1, b2 = boundary_points()
    out["boundary"] = (_soa(a, b1, b2), a.size)
    a, b1, b2 = axis_points()
    out["axis"] = (_soa(a, b1, b2), a.size)
    return out


def regimes():
    out = plain_regimes()
    out.update(seam_regimes())
    return out


def scale_of(p, M):
    """s_i = max(1, |p_i|_inf)."""
    return np.maximum(1.0, np.abs(np.asarray(p).reshape(3, M)).max(axis=0))


_cache = {}


def exact(name):
    """(p, M, hi, lo, inside, residual, oracle q) of a regime, computed once per process and
    shared; callers must not write into the arrays."""
    if name not in _cache:
        from . import foto_oracle, projk_exact
        p, M = regimes()[name]
        hi, lo, ins, res = projk_exact.project(p, M)
        with np.errstate(all="ignore"):
            qo = foto_oracle.stepB(p, M)
        for v in (p, hi, lo, ins, res, qo):
            v.setflags(write=False)
        _cache[name] = (p, M, hi, lo, ins, res, qo)
    return _cache[name]
