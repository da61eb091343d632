"""Numpy restatement of the maps and in-betweens of include/foto.h ("maps and in-betweens"),
written from the definitions alone, vectorised over the pixels, one IEEE operation per library
operation and in the same order -- so a float64 result can be compared at the last-bit level.

    V_n(z)         vel(P, x, y): one step of utils.reconstructTrajectory without its add
    F_n(z)         step(P, x, y) = z + V_n(z)
    inv(n, th, p)  inv(P, th, iters, x, y): z <- p, then z <- p - th V_n(z), iters times
    maps at s      maps(phi, s, iters) -> (4, Ny, Nx) = (a_x - x, a_y - y, b_x - x, b_y - y)
    in-between     interp(phi, f0, f1, s, iters) -> (Ny, Nx[, C]) float64, to_u8() the 8-bit rule

Also the seeded inputs the CPU and the GPU tests share: smooth_phi (low-pass, scaled to a given
largest |dV| per pixel) and smooth_frames.
"""
import numpy as np


def _trunc_clamp(v, hi):
    t = np.trunc(v)
    t = np.where(t >= 0.0, t, 0.0)          # also NaN and -inf
    t = np.minimum(t, float(hi))
    return t.astype(np.int64)


def vel(P, x, y):
    """(vx, vy) = V(x, y) on the Ny x Nx plane P: bilinear sample of un = G_x P, vn = G_y P
    (central differences, zero on the edge columns / rows), cell (trunc_clamp x, trunc_clamp y)."""
    Ny, Nx = P.shape
    tx, ty = _trunc_clamp(x, Nx - 2), _trunc_clamp(y, Ny - 2)
    xm, xp = np.maximum(tx - 1, 0), np.minimum(tx + 2, Nx - 1)
    ym, yp = np.maximum(ty - 1, 0), np.minimum(ty + 2, Ny - 1)
    a0, b0, c0, d0 = P[ty, xm], P[ty, tx], P[ty, tx + 1], P[ty, xp]
    a1, b1, c1, d1 = P[ty + 1, xm], P[ty + 1, tx], P[ty + 1, tx + 1], P[ty + 1, xp]
    bm, cm = P[ym, tx], P[ym, tx + 1]
    bp, cp = P[yp, tx], P[yp, tx + 1]
    dX, dY = x - tx, y - ty
    w1, w2, w3, w4 = (1 - dY) * (1 - dX), dX * (1 - dY), dY * dX, (1 - dX) * dY
    xl, xr = tx == 0, tx + 1 == Nx - 1
    yl, yr = ty == 0, ty + 1 == Ny - 1
    u00, u01 = np.where(xl, 0.0, 0.5 * (c0 - a0)), np.where(xr, 0.0, 0.5 * (d0 - b0))
    u11, u10 = np.where(xr, 0.0, 0.5 * (d1 - b1)), np.where(xl, 0.0, 0.5 * (c1 - a1))
    v00, v01 = np.where(yl, 0.0, 0.5 * (b1 - bm)), np.where(yl, 0.0, 0.5 * (c1 - cm))
    v11, v10 = np.where(yr, 0.0, 0.5 * (cp - c0)), np.where(yr, 0.0, 0.5 * (bp - b0))
    vx = w1 * u00 + w2 * u01 + w3 * u11 + w4 * u10
    vy = w1 * v00 + w2 * v01 + w3 * v11 + w4 * v10
    return vx, vy


def step(P, x, y):
    vx, vy = vel(P, x, y)
    return x + vx, y + vy


def inv(P, theta, iters, px, py):
    x, y = px, py
    for _ in range(iters):
        vx, vy = vel(P, x, y)
        x, y = px - theta * vx, py - theta * vy
    return x, y


def ends(phi, s, iters):
    """(ax, ay, bx, by, x, y), each (Ny, Nx): the two ends of the trajectory through every pixel
    centre of the time-s image.  phi: (Nt, Ny, Nx)."""
    Nt, Ny, Nx = phi.shape
    assert 0.0 <= s <= Nt - 1 and 1 <= iters <= 64
    y, x = np.meshgrid(np.arange(Ny, dtype=np.float64), np.arange(Nx, dtype=np.float64), indexing="ij")
    n = int(s)
    theta = s - n
    px, py = x, y
    if theta > 0:
        px, py = inv(phi[n], theta, iters, x, y)
    bx, by = px, py
    for m in range(n, Nt - 1):
        bx, by = step(phi[m], bx, by)
    ax, ay = px, py
    for m in range(n - 1, -1, -1):
        ax, ay = inv(phi[m], 1.0, iters, ax, ay)
    return ax, ay, bx, by, x, y


def maps(phi, s, iters=6):
    ax, ay, bx, by, x, y = ends(phi, s, iters)
    return np.stack([ax - x, ay - y, bx - x, by - y])


def sample(f, x, y):
    """S(f; x, y), f (h, w) or (h, w, C): clamped bilinear; a NaN coordinate gives NaN."""
    h, w = f.shape[:2]
    bad = np.isnan(x) | np.isnan(y)
    xc = np.where(bad, 0.0, np.minimum(np.maximum(x, 0.0), float(w - 1)))
    yc = np.where(bad, 0.0, np.minimum(np.maximum(y, 0.0), float(h - 1)))
    i0 = np.minimum(np.floor(xc).astype(np.int64), w - 2)
    j0 = np.minimum(np.floor(yc).astype(np.int64), h - 2)
    ax, ay = xc - i0, yc - j0
    if f.ndim == 3:
        ax, ay, bad = ax[..., None], ay[..., None], bad[..., None]
    t = (1.0 - ax) * f[j0, i0] + ax * f[j0, i0 + 1]
    b = (1.0 - ax) * f[j0 + 1, i0] + ax * f[j0 + 1, i0 + 1]
    v = (1.0 - ay) * t + ay * b
    return np.where(bad, np.nan, v)


def interp(phi, f0, f1, s, iters=6, divisor=1.0):
    """float64 (Ny, Nx[, C]): (1 - w) S(f0 / divisor; a) + w S(f1 / divisor; b), w = s / (Nt - 1)."""
    Nt = phi.shape[0]
    ax, ay, bx, by, _, _ = ends(phi, s, iters)
    g0 = np.asarray(f0).astype(np.float64)
    g1 = np.asarray(f1).astype(np.float64)
    if divisor != 1.0:
        g0, g1 = g0 / divisor, g1 / divisor
    w = s / float(Nt - 1)
    return (1.0 - w) * sample(g0, ax, ay) + w * sample(g1, bx, by)


def u8_arg(x):
    """255 clip(x, 0, 1) + 0.5 with NaN -> clip 0: the value the 8-bit rule truncates."""
    x = np.where(x >= 0.0, x, 0.0)
    x = np.minimum(x, 1.0)
    return 255.0 * x + 0.5


def to_u8(x):
    return np.floor(u8_arg(x)).astype(np.uint8)


def u8_ambiguous(x, eps=1e-9):
    """pixels whose 255 x + 0.5 lies within eps of an integer: their 8-bit value may differ"""
    a = u8_arg(x)
    return np.abs(a - np.round(a)) <= eps


# ------------------------------------------------------------------------- seeded inputs

def node_velocity(phi):
    """(un, vn), each (Nt, Ny, Nx): grad('N') of every plane -- central differences, zero borders."""
    un, vn = np.zeros_like(phi), np.zeros_like(phi)
    un[:, :, 1:-1] = 0.5 * (phi[:, :, 2:] - phi[:, :, :-2])
    vn[:, 1:-1, :] = 0.5 * (phi[:, 2:, :] - phi[:, :-2, :])
    return un, vn


def max_dv(phi):
    """the largest |dV| between neighbouring pixels, over both components and both axes"""
    m = 0.0
    for f in node_velocity(phi):
        for ax in (1, 2):
            d = np.abs(np.diff(f, axis=ax))
            if d.size:
                m = max(m, float(d.max()))
    return m


def smooth_phi(Nt, Ny, Nx, seed=0, dv=0.3, modes=3):
    """A low-pass random phi (Nt, Ny, Nx): a few cosine modes per plane, scaled so that max_dv is
    `dv` (left alone where the grid is too small to carry a velocity at all)."""
    rng = np.random.default_rng(seed)
    y = (np.arange(Ny) + 0.5) / Ny
    x = (np.arange(Nx) + 0.5) / Nx
    phi = np.zeros((Nt, Ny, Nx))
    for t in range(Nt):
        for p in range(min(modes, Nx)):
            for q in range(min(modes, Ny)):
                phi[t] += rng.standard_normal() * np.outer(np.cos(np.pi * q * y), np.cos(np.pi * p * x))
    m = max_dv(phi)
    if m > 0:
        phi *= dv / m
    return phi


def smooth_frames(Ny, Nx, C=None, seed=1):
    """Two float64 frames in [0, 1], (Ny, Nx) or (Ny, Nx, C): a few cosine modes plus a little noise."""
    rng = np.random.default_rng(seed)
    y = (np.arange(Ny) + 0.5) / Ny
    x = (np.arange(Nx) + 0.5) / Nx
    shape = (Ny, Nx) + (() if C is None else (C,))
    out = []
    for _ in range(2):
        f = np.zeros(shape)
        for c in range(1 if C is None else C):
            g = 0.5 + 0.05 * rng.standard_normal((Ny, Nx))
            for p in range(1, 4):
                g += 0.12 * rng.standard_normal() * np.outer(np.cos(np.pi * p * y), np.cos(np.pi * (4 - p) * x))
            if C is None:
                f = g
            else:
                f[..., c] = g
        out.append(np.clip(f, 0.0, 1.0))
    return out[0], out[1]


def u8_frames(Ny, Nx, C=None, seed=1):
    """smooth_frames as 8-bit images.  The four corner pixels never move (both velocity components
    are edge zeros there), so half-way their in-between is the exact mean of two 8-bit values: a
    rounding tie of the 8-bit rule whenever the two differ by an odd number.  The seeded frames
    agree in the corners, so that the reference itself is not on a tie there."""
    f0, f1 = smooth_frames(Ny, Nx, C, seed)
    u0, u1 = np.round(255 * f0).astype(np.uint8), np.round(255 * f1).astype(np.uint8)
    for j in (0, -1):
        for i in (0, -1):
            u1[j, i] = u0[j, i]
    return u0, u1


def blob_pair(Ny, Nx, shift=(3.0, 1.5), sigma=4.0, base=0.2):
    """A Gaussian blob on a background and the same blob shifted by `shift` = (dx, dy); and
    between(w): the analytically shifted frame at fraction w of the way."""
    y, x = np.meshgrid(np.arange(Ny, dtype=np.float64), np.arange(Nx, dtype=np.float64), indexing="ij")
    cx, cy = 0.5 * (Nx - 1) - 0.5 * shift[0], 0.5 * (Ny - 1) - 0.5 * shift[1]

    def between(w):
        return base + 0.7 * np.exp(-((x - cx - w * shift[0]) ** 2 + (y - cy - w * shift[1]) ** 2) / (2 * sigma ** 2))

    return between(0.0), between(1.0), between
