"""The exact projection onto K = {(a, b1, b2): a + (b1^2 + b2^2)/2 <= 0}, to 80 digits.

``foto_oracle.stepB`` restates the reference's closed forms (Cardano / trigonometric) in
float64, and the HIP ``project_K`` restates them again; neither is a yardstick for the other's
rounding.  This module computes the projection from its optimality conditions alone, in
``decimal`` (stdlib only), and shares no formula with either:

  p = (a, b) outside K  =>  q_b = b / x,  q_a = -|q_b|^2 / 2,
  x = 1 + lambda > 1 the unique root of  f(x) = x^3 - (a + 1) x^2 - rho^2 / 2,  rho = |b|.

(The Lagrangian gives q_b = b / (1 + lambda), q_a = a - lambda, and q on the boundary gives
a - lambda + rho^2 / (2 (1 + lambda)^2) = 0; multiplied by x^2 this is f.)  f(1) = -(a +
rho^2/2) < 0 outside K, and right of the root f is increasing and convex, so Newton started
right of it decreases monotonically onto it.  q_a is formed from q_b, never as a - lambda: at
large |a| that difference cancels.  Every point checks itself: |f(x)| <= 1e-45 of the largest
of f's three terms.  Membership in K is decided exactly, in rational arithmetic.

Inputs are float64 (converted exactly); inputs must be finite.  The result comes back as an
unevaluated float64 pair (hi, lo), q = hi + lo to ~2^-106 relative, so errors of float64
candidates can be formed vectorised: err = |(cand - hi) - lo|.
"""
import decimal
import math
from fractions import Fraction

import numpy as np

PREC = 80
RESIDUAL_BAR = decimal.Decimal("1e-45")
_CTX = decimal.Context(prec=PREC, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN)
_D = decimal.Decimal


def inside(a, b1, b2):
    """2 a + b1^2 + b2^2 <= 0, exactly (float64 arguments)."""
    return 2 * Fraction(a) + Fraction(b1) ** 2 + Fraction(b2) ** 2 <= 0


def _cbrt_above(c):
    """A Decimal >= c^(1/3) and within 1e-9 relative of it (c > 0)."""
    e = c.adjusted()
    k = e // 3
    m = float(c.scaleb(-3 * k, _CTX))            # in [1, 1000)
    return _D(math.exp(math.log(m) / 3.0) * (1.0 + 1e-9)).scaleb(k, _CTX)


def _start(ap1, c):
    """A point right of the root of f (or on it), within a small factor of it."""
    t = _cbrt_above(c)
    if ap1 <= 0:
        # f(x) = x^2 (x + m) - c, m = -(a + 1) >= 0: f >= x^3 - c and f >= m x^2 - c
        if ap1 < 0:
            t = min(t, _CTX.sqrt(_CTX.divide(c, -ap1)) * _D("1.000000001"))
        return t
    # f(a + 1 + t) = x^2 t - c with x >= t and x >= a + 1
    t = min(t, _CTX.divide(c, ap1 * ap1) * _D("1.000000001"))
    return _CTX.add(ap1, t)


def root(a, rho2):
    """(x, residual): the root x > 1 of x^3 - (a + 1) x^2 - rho2 / 2 for a point outside K
    (Decimal a, rho2 = |b|^2 exact), and |f(x)| over the largest of f's terms."""
    C = _CTX
    ap1 = C.add(a, 1)
    c = C.divide(rho2, 2)
    if c == 0:                       # on the axis: x^2 (x - (a + 1)) = 0
        return ap1, _D(0)
    x = _start(ap1, c)

    def f(x):
        x2 = C.multiply(x, x)
        return C.subtract(C.multiply(x2, C.subtract(x, ap1)), c), x2

    for _ in range(400):
        fx, x2 = f(x)
        if fx <= 0:
            break
        # f'(x) = 3 x^2 - 2 (a + 1) x > 0 right of the root
        xn = C.subtract(x, C.divide(fx, C.subtract(3 * x2, 2 * C.multiply(ap1, x))))
        if xn >= x:
            break
        x = xn
    fx, x2 = f(x)
    big = max(C.multiply(x2, x), abs(C.multiply(ap1, x2)), c)
    return x, abs(C.divide(fx, big))


def project_point(a, b1, b2):
    """((q_a, q_1, q_2) as Decimals, residual) for one float64 point; inside K the identity
    (residual 0)."""
    if not (math.isfinite(a) and math.isfinite(b1) and math.isfinite(b2)):
        raise ValueError("projk_exact: finite inputs only")
    A, B1, B2 = _D(a), _D(b1), _D(b2)
    if inside(a, b1, b2):
        return (A, B1, B2), _D(0)
    C = _CTX
    # (rounded to PREC digits; only the membership test above needs |b|^2 exactly)
    rho2 = C.add(C.multiply(B1, B1), C.multiply(B2, B2))
    x, res = root(A, rho2)
    q1 = C.divide(B1, x)
    q2 = C.divide(B2, x)
    qa = C.divide(C.add(C.multiply(q1, q1), C.multiply(q2, q2)), -2)
    return (qa, q1, q2), res


def project_point_bisect(a, b1, b2, iters=420):
    """The same projection by another route, for cross-checking: lambda > 0 with
    g(lambda) = a - lambda + rho^2 / (2 (1 + lambda)^2) = 0 (g decreasing) by bisection."""
    A, B1, B2 = _D(a), _D(b1), _D(b2)
    if inside(a, b1, b2):
        return A, B1, B2
    C = _CTX
    h = C.divide(C.add(C.multiply(B1, B1), C.multiply(B2, B2)), 2)
    if h == 0:
        return _D(0), C.divide(B1, C.add(A, 1)), C.divide(B2, C.add(A, 1))

    def g(lam):
        x = C.add(1, lam)
        return C.add(C.subtract(A, lam), C.divide(h, C.multiply(x, x)))

    lo = _D(0)
    hi = C.add(abs(A), C.add(h, 1))           # g(hi) <= a - |a| - h - 1 + h < 0
    for _ in range(iters):
        mid = C.divide(C.add(lo, hi), 2)
        if mid == lo or mid == hi:
            break
        if g(mid) > 0:
            lo = mid
        else:
            hi = mid
    x = C.add(1, C.divide(C.add(lo, hi), 2))
    q1 = C.divide(B1, x)
    q2 = C.divide(B2, x)
    return C.divide(C.add(C.multiply(q1, q1), C.multiply(q2, q2)), -2), q1, q2


def _split(d):
    hi = float(d)
    return hi, float(_CTX.subtract(d, _D(hi)))


def project(p, M):
    """The projection of 3 SoA float64 fields of length M (``foto_oracle.stepB``'s layout).
    Returns (hi, lo, inside, residual): hi + lo the exact result ([3M] each), the boolean
    membership mask and the per-point cubic residual ([M])."""
    p = np.asarray(p, dtype=np.float64)
    hi = np.empty(3 * M)
    lo = np.empty(3 * M)
    ins = np.zeros(M, dtype=bool)
    res = np.zeros(M)
    for i in range(M):
        a, b1, b2 = float(p[i]), float(p[M + i]), float(p[2 * M + i])
        ins[i] = inside(a, b1, b2)
        q, r = project_point(a, b1, b2)
        res[i] = float(r)
        for k in range(3):
            hi[k * M + i], lo[k * M + i] = _split(q[k])
    return hi, lo, ins, res


def point_error(q, hi, lo, M):
    """err_i = max_k |q - q_exact| per point, for a float64 candidate q ([3M]); non-finite
    where q is."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs((np.asarray(q, dtype=np.float64) - hi) - lo).reshape(3, M)
        return np.where(np.isnan(d).any(axis=0), np.nan, d.max(axis=0))
