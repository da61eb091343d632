"""The numpy restatement of the entropic-transport section of include/foto.h (convolutional
Sinkhorn on the pixel grid, cost |x - y|^2 / 2, the Gibbs kernel truncated to a (2 R + 1)^2 box):
the yardstick of tests/test_gpu_sinkhorn.py, which holds the device to it bit for bit, and of
tests/test_sinkhorn_host.py, which holds it to a dense solve.

Every tap sum runs sequentially in ascending d from 0.0 with the product rounded before the add
(numpy never fuses a * b + c); a tap outside the frame is 0.0."""
import math

import numpy as np

F64 = np.float64
MAX_RADIUS = 32


def tables(eps, R):
    """float64 (3, R + 1): k[d] = exp(-d d / (2 eps)), k1[d] = d k[d], k2[d] = (0.5 (d d)) k[d]."""
    if not (isinstance(R, (int, np.integer)) and 0 <= R <= MAX_RADIUS):
        raise ValueError(f"radius = {R!r} must be an int in 0 .. {MAX_RADIUS}")
    if not (np.isfinite(eps) and eps > 0):
        raise ValueError(f"eps = {eps!r} must be finite and > 0")
    d = np.arange(R + 1, dtype=F64)
    k = np.exp(-(d * d) / (2.0 * F64(eps)))
    return np.stack([k, d * k, (0.5 * (d * d)) * k])


def signed(tab):
    """(3, 2 R + 1): the tables at d = -R .. R (k[|d|], -k1[|d|], k2[|d|] for negative d)."""
    k, k1, k2 = tab
    return np.stack([np.concatenate([k[:0:-1], k]), np.concatenate([-k1[:0:-1], k1]),
                     np.concatenate([k2[:0:-1], k2])])


def _pass(p, z, axis):
    """sum_d p[d] z(.. + d ..) along `axis`, d ascending, zero outside the frame."""
    R = (len(p) - 1) // 2
    pad = [(0, 0), (0, 0)]
    pad[axis] = (R, R)
    zp = np.pad(z, pad)
    n = z.shape[axis]
    acc = np.zeros_like(z)
    for d in range(2 * R + 1):
        sl = zp[:, d:d + n] if axis == 1 else zp[d:d + n, :]
        acc = acc + p[d] * sl
    return acc


def conv(p, q, z):
    """Row table p (along x), then column table q (along y); p, q of length 2 R + 1."""
    return _pass(q, _pass(p, z, 1), 0)


def div(m, s):
    ok = (m > 0) & (s > 0)
    with np.errstate(all="ignore"):
        return np.where(ok, m / np.where(ok, s, 1.0), 0.0)


def clean(f):
    """(frame with negative / non-finite pixels at 0, their count)."""
    f = np.asarray(f, dtype=F64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(f) & (f >= 0)
    return np.where(ok, f, 0.0), int(np.count_nonzero(~ok))


class Ref:
    """The solver of include/foto.h on h x w float64 frames."""

    def __init__(self, w, h, eps=2.0, radius=16, table=None):
        self.w, self.h, self.R = int(w), int(h), int(radius)
        self.tab = signed(tables(eps, radius) if table is None else np.asarray(table, dtype=F64))
        self.k, self.k1, self.k2 = self.tab

    def set_frames(self, f0, f1):
        self.mu, b0 = clean(np.reshape(f0, (self.h, self.w)))
        self.nu, b1 = clean(np.reshape(f1, (self.h, self.w)))
        self.bad = b0 + b1
        self.a = np.zeros((self.h, self.w))
        self.b = np.ones((self.h, self.w))
        self.iterations = 0
        return self

    def iterate(self, n):
        for _ in range(int(n)):
            self.a = div(self.mu, conv(self.k, self.k, self.b))
            self.b = div(self.nu, conv(self.k, self.k, self.a))
        self.iterations += int(n)
        return self

    def flow(self, direction="forward"):
        """(u, v, valid): float64 (h, w) twice and uint8 (h, w)."""
        z, marg = (self.b, self.mu) if direction == "forward" else (self.a, self.nu)
        s = conv(self.k, self.k, z)
        ok = (marg > 0) & (s > 0)
        den = np.where(ok, s, 1.0)
        with np.errstate(all="ignore"):
            u = np.where(ok, conv(self.k1, self.k, z) / den, 0.0)
            v = np.where(ok, conv(self.k, self.k1, z) / den, 0.0)
        return u, v, ok.astype(np.uint8)

    def terms(self):
        """The per-pixel terms of the record's two device sums: |a s - mu| and the cost."""
        s = conv(self.k, self.k, self.b)
        with np.errstate(all="ignore"):
            err = np.abs(self.a * s - self.mu)
            cost = self.a * (conv(self.k2, self.k, self.b) + conv(self.k, self.k2, self.b))
        return err, cost, (self.mu > 0) & (s == 0)

    def info(self):
        """The record as a dict; the four float sums exactly rounded (math.fsum), so that a sum in
        any order is within sum_bounds() of them."""
        err, cost, unr = self.terms()
        c = math.fsum(cost.ravel())
        return dict(mass0=math.fsum(self.mu.ravel()), mass1=math.fsum(self.nu.ravel()),
                    marginal_error=math.fsum(err.ravel()), cost=c,
                    w2=float(np.sqrt(2.0 * c)), bad=self.bad, unreachable=int(np.count_nonzero(unr)),
                    iterations=self.iterations)

    def sum_bounds(self):
        """n 2^-53 sum |terms| for mass0, mass1, marginal_error, cost: the bound of any order."""
        err, cost, _ = self.terms()
        n = self.w * self.h
        return tuple(n * 2.0 ** -53 * float(np.abs(t).sum()) for t in (self.mu, self.nu, err, cost))


def costs(f0, f1, w, h, eps, radius, iters):
    """(cost01, cost00, cost11) and the Ref objects of the three solves of the divergence."""
    out, refs = [], []
    for x, y in ((f0, f1), (f0, f0), (f1, f1)):
        r = Ref(w, h, eps, radius).set_frames(x, y).iterate(iters)
        refs.append(r)
        out.append(r.info()["cost"])
    return tuple(out), refs


def divergence(f0, f1, w, h, eps, radius, iters):
    """(cost01 - cost00 / 2 - cost11 / 2, w2_debiased = sqrt(2 max(that, 0)))."""
    (c01, c00, c11), _ = costs(f0, f1, w, h, eps, radius, iters)
    d = c01 - 0.5 * c00 - 0.5 * c11
    return d, float(np.sqrt(2.0 * max(d, 0.0)))


def same(a, b):
    """Bit for bit, NaNs of any payload alike."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all((a == b) | ((a != a) & (b != b))))


def dense_kernel(w, h, tab):
    """The N x N truncated Gibbs kernel and the displacement matrices (N = w h, row-major pixels)."""
    k = np.asarray(tab)[0]
    R = len(k) - 1
    jj, ii = np.divmod(np.arange(w * h), w)
    dx = ii[None, :] - ii[:, None]
    dy = jj[None, :] - jj[:, None]
    inside = (np.abs(dx) <= R) & (np.abs(dy) <= R)
    K = np.where(inside, k[np.minimum(np.abs(dx), R)] * k[np.minimum(np.abs(dy), R)], 0.0)
    return K, dx.astype(F64), dy.astype(F64)


def dense_solve(f0, f1, w, h, tab, iters):
    """Dense Sinkhorn with the same truncated kernel: (a, b, u, v, valid, cost), by matrix products."""
    K, dx, dy = dense_kernel(w, h, tab)
    mu, _ = clean(np.ravel(f0))
    nu, _ = clean(np.ravel(f1))
    a, b = np.zeros(w * h), np.ones(w * h)
    for _ in range(iters):
        a = div(mu, K @ b)
        b = div(nu, K @ a)
    s = K @ b
    ok = (mu > 0) & (s > 0)
    den = np.where(ok, s, 1.0)
    u = np.where(ok, ((K * dx) @ b) / den, 0.0)
    v = np.where(ok, ((K * dy) @ b) / den, 0.0)
    cost = float(a @ ((K * (0.5 * (dx * dx + dy * dy))) @ b))
    sh = (h, w)
    return a.reshape(sh), b.reshape(sh), u.reshape(sh), v.reshape(sh), ok.reshape(sh), cost
