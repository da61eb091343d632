"""Numpy restatement of the sparse tracking entries (include/foto.h, "sparse tracking"): the
Shi-Tomasi corner detector, pyramidal Lucas-Kanade with fixed counts, and a dense flow sampled at
points -- the yardstick of tests/test_sparse_host.py and tests/test_gpu_sparse.py.  Built on
gn_pyr_ref's sizes / down / sample and tvl1_ref's grad_c, and on nothing else.  Every sum is
written in the order the kernels evaluate it, so the device is held to it bit for bit."""
import numpy as np

import gn_pyr_ref as G
import tvl1_ref as T

CORNER_DEFAULTS = dict(quality=0.01, window=3, nms=5, margin=8)
LK_DEFAULTS = dict(radius=7, levels=4, min_size=16, iters=10, min_eig=1e-7)
FLAT, OUT, NONFINITE, INCONSISTENT = 1, 2, 4, 8


# ------------------------------------------------------------------ corners

def box_sum(P, c):
    """The (2 c + 1)^2 box sum of an (h, w) plane that counts as +0.0 outside the frame: horizontal
    sums in increasing dx from the first term, then vertical sums of those in increasing dy."""
    h, w = P.shape
    Z = np.zeros((h, w + 2 * c))
    Z[:, c:c + w] = P
    H = Z[:, 0:w].copy()
    for dx in range(1, 2 * c + 1):
        H = H + Z[:, dx:dx + w]
    Z = np.zeros((h + 2 * c, w))
    Z[c:c + h] = H
    B = Z[0:h].copy()
    for dy in range(1, 2 * c + 1):
        B = B + Z[dy:dy + h]
    return B


def response(f, w, h, window=3):
    """R = the smaller eigenvalue of the box-summed structure tensor, (h, w)."""
    gx, gy = (g.reshape(h, w) for g in T.grad_c(f, w, h))
    a, b, cc = box_sum(gx * gx, window), box_sum(gx * gy, window), box_sum(gy * gy, window)
    with np.errstate(invalid="ignore", over="ignore"):
        return 0.5 * ((a + cc) - np.sqrt((a - cc) * (a - cc) + 4.0 * (b * b)))


def candidates(R, quality=0.01, nms=5, margin=8):
    """The raster indices of the candidate pixels of an (h, w) response, ascending."""
    h, w = R.shape
    with np.errstate(invalid="ignore"):
        pos = np.isfinite(R) & (R > 0)
        rmax = R[pos].max() if pos.any() else 0.0
        ok = pos & (R >= quality * rmax)
    inner = np.zeros((h, w), dtype=bool)
    if h > 2 * margin and w > 2 * margin:
        inner[margin:h - margin, margin:w - margin] = True
    out = []
    for y, x in np.argwhere(ok & inner):
        y0, y1, x0, x1 = max(y - nms, 0), min(y + nms, h - 1), max(x - nms, 0), min(x + nms, w - 1)
        win = R[y0:y1 + 1, x0:x1 + 1]
        yy, xx = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
        earlier = (yy < y) | ((yy == y) & (xx < x))
        later = ~earlier & ~((yy == y) & (xx == x))
        with np.errstate(invalid="ignore"):
            if np.all(R[y, x] > win[earlier]) and np.all(R[y, x] >= win[later]):
                out.append(y * w + x)
    return np.array(out, dtype=np.int64)


def corners(f, w, h, max_count, quality=0.01, window=3, nms=5, margin=8):
    """(points (max_count, 2) float64 = (x, y) with NaN rows from the count on, count, R (h, w)):
    the max_count strongest candidates (R descending, then index ascending) in raster order."""
    R = response(f, w, h, window)
    idx = candidates(R, quality, nms, margin)
    key = R.ravel()[idx]
    order = sorted(range(len(idx)), key=lambda k: (-key[k], idx[k]))[:max_count]
    kept = np.sort(idx[order]) if len(order) else idx[:0]
    pts = np.full((max_count, 2), np.nan)
    pts[:len(kept), 0] = kept % w
    pts[:len(kept), 1] = kept // w
    return pts, len(kept), R


# ------------------------------------------------------------------ Lucas-Kanade

def wsum(V):
    """The window sum of (M, n) values, n <= 256, in the lane order: zero-padded to (4, 64), three
    adds, then six halvings a[p] += a[p + o], p < o, o = 32 .. 1."""
    M, n = V.shape
    P = np.zeros((M, 256))
    P[:, :n] = V
    P = P.reshape(M, 4, 64)
    a = ((P[:, 0] + P[:, 1]) + P[:, 2]) + P[:, 3]
    for o in (32, 16, 8, 4, 2, 1):
        a = a[:, :o] + a[:, o:2 * o]
    return a[:, 0]


def pyramids(f0, f1, w, h, levels=4, min_size=16):
    """(sizes, levels of f0, levels of f1), finest first."""
    sz = G.sizes(w, h, levels, min_size)
    a, b = [np.asarray(f0, dtype=np.float64).ravel()], [np.asarray(f1, dtype=np.float64).ravel()]
    for (wl, hl) in sz[:-1]:
        a.append(G.down(a[-1], wl, hl))
        b.append(G.down(b[-1], wl, hl))
    return sz, a, b


def lk_track(f0, f1, w, h, pts, direction=0, prior=None, fb_tol=0.5, status=None, dtype=np.float64, radius=7,
             levels=4, min_size=16, iters=10, min_eig=1e-7, pyr=None):
    """(d (M, 2) of ``dtype``, status uint8 (M,), err (M,), fb (M,) or None) of the points ``pts``
    ((M, 2), float32 or float64).  ``prior`` ((M, 2) of ``dtype``): the start point is pts + prior,
    fb = |prior + d|, and ``status`` (the buffer passed in) gains INCONSISTENT unless fb <= fb_tol."""
    sz, A, B = pyr if pyr is not None else pyramids(f0, f1, w, h, levels, min_size)
    if direction == 1:
        A, B = B, A
    L = len(sz)
    pts = np.asarray(pts).astype(np.float64).reshape(-1, 2)
    M = len(pts)
    x0, y0 = pts[:, 0].copy(), pts[:, 1].copy()
    if prior is not None:
        pr = np.asarray(prior).astype(np.float64).reshape(-1, 2)
        x0, y0 = x0 + pr[:, 0], y0 + pr[:, 1]
    fin = np.isfinite(x0) & np.isfinite(y0)
    X0, Y0 = x0[fin], y0[fin]
    m = len(X0)
    side = 2 * radius + 1
    n = side * side
    e = np.arange(n)
    ay, ax = (e // side - radius).astype(np.float64), (e % side - radius).astype(np.float64)
    dx, dy = np.zeros(m), np.zeros(m)
    st = np.zeros(m, dtype=np.uint8)
    err = np.full(m, np.nan)
    with np.errstate(all="ignore"):
        for l in range(L - 1, -1, -1):
            x, y = X0.copy(), Y0.copy()
            for k in range(l):
                x = (x + 0.5) * (float(sz[k + 1][0]) / float(sz[k][0])) - 0.5
                y = (y + 0.5) * (float(sz[k + 1][1]) / float(sz[k][1])) - 0.5
            wl, hl = sz[l]
            if l < L - 1:
                dx = dx * (float(wl) / float(sz[l + 1][0]))
                dy = dy * (float(hl) / float(sz[l + 1][1]))
            gxa, gya = T.grad_c(A[l], wl, hl)
            cx, cy = x[:, None] + ax[None, :], y[:, None] + ay[None, :]
            Tm = G.sample(A[l], wl, hl, cx, cy)
            Gx, Gy = G.sample(gxa, wl, hl, cx, cy), G.sample(gya, wl, hl, cx, cy)
            gxx, gxy, gyy = wsum(Gx * Gx), wsum(Gx * Gy), wsum(Gy * Gy)
            det = gxx * gyy - gxy * gxy
            mineig = 0.5 * ((gxx + gyy) - np.sqrt((gxx - gyy) * (gxx - gyy) + 4.0 * (gxy * gxy))) / float(n)
            tex = mineig > min_eig
            if l == 0:
                st[~tex] |= FLAT

            def residual():
                return Tm - G.sample(B[l], wl, hl, (x + dx)[:, None] + ax[None, :], (y + dy)[:, None] + ay[None, :])

            for _ in range(iters):
                r = residual()
                bx, by = wsum(r * Gx), wsum(r * Gy)
                dx = np.where(tex, dx + (gyy * bx - gxy * by) / det, dx)
                dy = np.where(tex, dy + (gxx * by - gxy * bx) / det, dy)
            if l == 0:
                err = wsum(np.abs(residual())) / float(n)
    d = np.full((M, 2), np.nan)
    d[fin, 0], d[fin, 1] = dx, dy
    status_out = np.zeros(M, dtype=np.uint8)
    status_out[fin] = st
    err_out = np.full(M, np.nan)
    err_out[fin] = err
    bad = ~(np.isfinite(d[:, 0]) & np.isfinite(d[:, 1]))
    d[bad] = np.nan
    err_out[bad] = np.nan
    status_out[bad] |= NONFINITE
    with np.errstate(invalid="ignore"):
        xe, ye = x0 + d[:, 0], y0 + d[:, 1]
        inside = ((x0 >= 0) & (x0 <= w - 1) & (y0 >= 0) & (y0 <= h - 1) & (xe >= 0) & (xe <= w - 1) & (ye >= 0)
                  & (ye <= h - 1))
    status_out[~inside] |= OUT
    fb = None
    if prior is not None:
        with np.errstate(invalid="ignore"):
            sx, sy = pr[:, 0] + d[:, 0], pr[:, 1] + d[:, 1]
            fb = np.sqrt(sx * sx + sy * sy)
            ok = fb <= fb_tol
        status_out = np.array(status, dtype=np.uint8).copy()
        status_out[~ok] |= INCONSISTENT
    return d.astype(dtype), status_out, err_out, fb


def track_checked(f0, f1, w, h, pts, fb_tol=0.5, **opts):
    """The forward track and the forward-backward check: (d, status, err, fb)."""
    pyr = pyramids(f0, f1, w, h, opts.get("levels", 4), opts.get("min_size", 16))
    d, st, err, _ = lk_track(f0, f1, w, h, pts, pyr=pyr, **opts)
    _, st, _, fb = lk_track(f0, f1, w, h, pts, direction=1, prior=d, fb_tol=fb_tol, status=st, pyr=pyr, **opts)
    return d, st, err, fb


# ------------------------------------------------------------------ sampling

def sample_flow(u, v, w, h, pts, dtype=np.float64):
    """(S(u; x, y), S(v; x, y)) at the points, (M, 2) of ``dtype``; u, v widen to float64."""
    pts = np.asarray(pts).astype(np.float64).reshape(-1, 2)
    u, v = np.asarray(u).astype(np.float64), np.asarray(v).astype(np.float64)
    return np.stack([G.sample(u, w, h, pts[:, 0], pts[:, 1]), G.sample(v, w, h, pts[:, 0], pts[:, 1])],
                    axis=-1).astype(dtype)


def same(a, b):
    """Bit equality for the tests: equal values, NaN where NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
