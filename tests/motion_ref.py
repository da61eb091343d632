"""The numpy restatement of the global-motion stage (include/foto.h, "global motion";
csrc/foto_motion.hip): the sample lookup, the elimination, the scoring rule, the fixed-order normal
equations, the refinement, the matrix in pixel coordinates, the field and the residual.  Every
operation is written in the order the header states, one rounding per operation (numpy never
fuses a product and a sum), so the device can be held to it bit for bit.  numpy.linalg is not used.
"""
import numpy as np

TRANSLATION, SIMILARITY, AFFINE, HOMOGRAPHY = range(4)
MODELS = {"translation": TRANSLATION, "similarity": SIMILARITY, "affine": AFFINE, "homography": HOMOGRAPHY}
NONE, KEPT = 1, 2
TILE = 1024
PIVOT = 1e-12
DEFAULTS = dict(threshold=1.0, rounds=3, min_inliers=0)
IDENTITY = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0])


def samples(H=256, seed=0):
    """The host table of sample numbers, uint32 (H, 4): foto.motion.samples' rule."""
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=(int(H), 4), dtype=np.uint64).astype(np.uint32)


def k_of(model):
    return model + 1


def P_of(model):
    return 2 * (model + 1)


def same(a, b):
    """Bit equality for the tests: equal values, NaN where NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


# ------------------------------------------------------------------ the models

def rows(model, x, y, X, Y):
    """(r1, b1, r2, b2) of correspondences x, y, X, Y (any common shape S): r (S, P), b (S)."""
    x, y, X, Y = (np.asarray(a, dtype=np.float64) for a in (x, y, X, Y))
    one, zero = np.ones_like(x), np.zeros_like(x)
    if model == TRANSLATION:
        return np.stack([one, zero], -1), X - x, np.stack([zero, one], -1), Y - y
    if model == SIMILARITY:
        return np.stack([x, -y, one, zero], -1), X, np.stack([y, x, zero, one], -1), Y
    r1, r2 = [x, y, one, zero, zero, zero], [zero, zero, zero, x, y, one]
    if model == HOMOGRAPHY:
        r1 += [-(X * x), -(X * y)]
        r2 += [-(Y * x), -(Y * y)]
    return np.stack(r1, -1), X, np.stack(r2, -1), Y


def matrix(model, p):
    """The 3 x 3 matrices (B, 9) of parameter vectors p (B, P)."""
    B = p.shape[0]
    m = np.zeros((B, 9))
    m[:, 8] = 1.0
    if model == TRANSLATION:
        m[:, 0] = m[:, 4] = 1.0
        m[:, 2], m[:, 5] = p[:, 0], p[:, 1]
    elif model == SIMILARITY:
        m[:, 0], m[:, 1], m[:, 2] = p[:, 0], -p[:, 1], p[:, 2]
        m[:, 3], m[:, 4], m[:, 5] = p[:, 1], p[:, 0], p[:, 3]
    else:
        m[:, :6] = p[:, :6]
        if model == HOMOGRAPHY:
            m[:, 6], m[:, 7] = p[:, 6], p[:, 7]
    return m


def solve(A, b):
    """The elimination of include/foto.h for a batch: A (B, n, n), b (B, n) -> p (B, n), ok (B).
    A degenerate system has ok False and p NaN."""
    A, b = np.array(A, dtype=np.float64), np.array(b, dtype=np.float64)
    B, n, _ = A.shape
    every = np.arange(B)
    ok = np.ones(B, dtype=bool)
    with np.errstate(all="ignore"):
        for c in range(n):
            piv = np.full(B, c)
            best = np.abs(A[:, c, c])
            for r in range(c + 1, n):
                a = np.abs(A[:, r, c])
                better = a > best
                best = np.where(better, a, best)
                piv = np.where(better, r, piv)
            ok &= best > PIVOT
            t = A[every, c].copy()
            A[every, c] = A[every, piv]
            A[every, piv] = t
            t = b[every, c].copy()
            b[every, c] = b[every, piv]
            b[every, piv] = t
            for r in range(c + 1, n):
                f = A[:, r, c] / A[:, c, c]
                for j in range(c + 1, n):
                    A[:, r, j] = A[:, r, j] - f * A[:, c, j]
                b[:, r] = b[:, r] - f * b[:, c]
        p = np.zeros((B, n))
        for r in range(n - 1, -1, -1):
            s = b[:, r].copy()
            for j in range(r + 1, n):
                s = s - A[:, r, j] * p[:, j]
            p[:, r] = s / A[:, r, r]
    p[~ok] = np.nan
    return p, ok


def inlier(m, x, y, X, Y, t2):
    """The inlier rule: m (..., 9) against list entries (n): a bool array (..., n)."""
    m = np.asarray(m, dtype=np.float64)[..., None, :]
    with np.errstate(all="ignore"):
        wv = (m[..., 6] * x + m[..., 7] * y) + 1.0
        ex = ((m[..., 0] * x + m[..., 1] * y) + m[..., 2]) - X * wv
        ey = ((m[..., 3] * x + m[..., 4] * y) + m[..., 5]) - Y * wv
        return (wv > 0.0) & (ex * ex + ey * ey <= t2 * (wv * wv))


def fsum(terms, M):
    """The one order of every floating-point sum: terms (K, n), n <= M, padded with +0.0 to
    ceil(M / TILE) tiles; thread slots, the wave tree, the four waves, the tiles in order."""
    terms = np.atleast_2d(np.asarray(terms, dtype=np.float64))
    K, n = terms.shape
    nb = (M + TILE - 1) // TILE
    a = np.zeros((K, nb * TILE))
    a[:, :n] = terms
    a = a.reshape(K, nb, 4, 4, 64)            # (slot, wave, lane): entry = slot * 256 + wave * 64 + lane
    a = ((a[:, :, 0] + a[:, :, 1]) + a[:, :, 2]) + a[:, :, 3]
    o = 32
    while o >= 1:
        a = a[..., :o] + a[..., o:2 * o]
        o //= 2
    a = a[..., 0]
    a = ((a[:, :, 0] + a[:, :, 1]) + a[:, :, 2]) + a[:, :, 3]
    s = np.zeros(K)
    for b in range(nb):
        s = s + a[:, b]
    return s


def normalise(px, py, dx, dy, w, h):
    s, cx, cy = 0.5 * max(w, h), 0.5 * (w - 1), 0.5 * (h - 1)
    with np.errstate(all="ignore"):
        return (px - cx) / s, (py - cy) / s, ((px + dx) - cx) / s, ((py + dy) - cy) / s


def denormalise(m, w, h):
    """The pixel matrix (9,) of a normalised one."""
    s, cx, cy = 0.5 * max(w, h), 0.5 * (w - 1), 0.5 * (h - 1)
    m = np.asarray(m, dtype=np.float64).reshape(3, 3)
    A, B = np.zeros((3, 3)), np.zeros((3, 3))
    with np.errstate(all="ignore"):
        A[:, 0] = m[:, 0] / s
        A[:, 1] = m[:, 1] / s
        A[:, 2] = (m[:, 2] - (m[:, 0] * cx) / s) - (m[:, 1] * cy) / s
        B[0] = s * A[0] + cx * A[2]
        B[1] = s * A[1] + cy * A[2]
        B[2] = A[2]
        out = (B / B[2, 2]).ravel()
    out[8] = 1.0
    return out


# ------------------------------------------------------------------ the fit

def refine_round(model, m, x, y, X, Y, t2, M):
    """One refinement round from the normalised model m: (m', kept)."""
    k = k_of(model)
    P = P_of(model)
    inl = inlier(m, x, y, X, Y, t2)
    if inl.sum() < k:
        return m, True
    r1, b1, r2, b2 = rows(model, x, y, X, Y)
    terms = []
    with np.errstate(all="ignore"):
        for a in range(P):
            for b in range(a, P):
                terms.append(np.where(inl, r1[:, a] * r1[:, b] + r2[:, a] * r2[:, b], 0.0))
        for a in range(P):
            terms.append(np.where(inl, r1[:, a] * b1 + r2[:, a] * b2, 0.0))
    tot = fsum(np.array(terms), M)
    N = np.zeros((P, P))
    i = 0
    for a in range(P):
        for b in range(a, P):
            N[a, b] = N[b, a] = tot[i]
            i += 1
    p, ok = solve(N[None], tot[None, i:])
    if not ok[0]:
        return m, True
    return matrix(model, p)[0], False


def fit_list(model, x, y, X, Y, M, w, h, table, threshold=1.0, rounds=3, min_inliers=0):
    """Steps 3 to 6 on the list of valid correspondences (normalised): (pixel model (9,), list
    mask uint8 (n,), info int64 (4,), rms, scores int (H,), normalised model (9,))."""
    model = MODELS.get(model, model)
    k = k_of(model)
    n = len(x)
    table = np.asarray(table, dtype=np.uint32).reshape(-1, 4)
    H = len(table)
    s = 0.5 * max(w, h)
    t = threshold / s
    t2 = t * t
    scores = np.full(H, -1, dtype=np.int64)
    hyp = np.full((H, 9), np.nan)
    if n >= k:
        q = ((table[:, :k].astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)   # (H, k)
        r1, b1, r2, b2 = rows(model, x[q], y[q], X[q], Y[q])                                       # (H, k, P)
        A = np.stack([r1, r2], 2).reshape(H, 2 * k, 2 * k)     # entry i: rows 2 i, 2 i + 1
        b = np.stack([b1, b2], 2).reshape(H, 2 * k)
        p, ok = solve(A, b)
        hyp[ok] = matrix(model, p[ok])
        for j0 in range(0, H, 64):   # (in slices: H x n booleans at once would be large)
            scores[j0:j0 + 64] = np.where(ok[j0:j0 + 64], inlier(hyp[j0:j0 + 64], x, y, X, Y, t2).sum(axis=1), -1)
    winner = int(np.argmax(scores))   # the first of the highest: the lowest index on a tie
    if scores[winner] < max(k, min_inliers):
        info = np.array([0, n, -1, NONE], dtype=np.int64)
        return IDENTITY.copy(), np.zeros(n, dtype=np.uint8), info, np.nan, scores, IDENTITY.copy()
    m = hyp[winner].copy()
    status = 0
    for _ in range(rounds):
        m, kept = refine_round(model, m, x, y, X, Y, t2, M)
        status |= KEPT if kept else 0
    inl = inlier(m, x, y, X, Y, t2)
    with np.errstate(all="ignore"):
        wv = (m[6] * x + m[7] * y) + 1.0
        rx = ((m[0] * x + m[1] * y) + m[2]) / wv - X
        ry = ((m[3] * x + m[4] * y) + m[5]) / wv - Y
        S = fsum(np.where(inl, rx * rx + ry * ry, 0.0), M)[0]
        count = int(inl.sum())
        rms = s * np.sqrt(S / np.float64(count))
    info = np.array([count, n, winner, status], dtype=np.int64)
    return denormalise(m, w, h), inl.astype(np.uint8), info, rms, scores, m


def fit(points, disp, w, h, model="affine", status=None, table=None, **opts):
    """foto_motion_fit_dev: (model (9,), mask uint8 (M,), info int64 (4,), rms).  points, disp:
    (M, 2) float32 | float64, widened exactly."""
    p, d = np.asarray(points).astype(np.float64), np.asarray(disp).astype(np.float64)
    M = len(p)
    valid = np.isfinite(p).all(axis=1) & np.isfinite(d).all(axis=1)
    if status is not None:
        valid &= np.asarray(status) == 0
    idx = np.flatnonzero(valid)
    x, y, X, Y = normalise(p[idx, 0], p[idx, 1], d[idx, 0], d[idx, 1], w, h)
    table = samples() if table is None else table
    m, lmask, info, rms, _, _ = fit_list(model, x, y, X, Y, M, w, h, table, **opts)
    mask = np.zeros(M, dtype=np.uint8)
    mask[idx] = lmask
    return m, mask, info, rms


def flow_uv(flow, layout="planar"):
    """(u, v) float64 (h, w) of one flow record, planar (3, h, w) or interleaved (h, w, 2)."""
    f = np.asarray(flow)
    u, v = (f[0], f[1]) if layout == "planar" else (f[..., 0], f[..., 1])
    return u.astype(np.float64), v.astype(np.float64)


def fit_flow(flow, w, h, model="affine", layout="planar", stride=4, mask=None, table=None, **opts):
    """foto_motion_fit_flow_dev on one record: (model, mask uint8 (lh, lw), info, rms)."""
    u, v = flow_uv(flow, layout)
    ys, xs = np.arange(0, h, stride), np.arange(0, w, stride)
    py, px = (a.ravel().astype(np.float64) for a in np.meshgrid(ys, xs, indexing="ij"))
    dx, dy = u[::stride, ::stride].ravel(), v[::stride, ::stride].ravel()
    M = len(px)
    valid = np.isfinite(dx) & np.isfinite(dy)
    if mask is not None:
        valid &= np.asarray(mask)[::stride, ::stride].ravel() != 0
    idx = np.flatnonzero(valid)
    x, y, X, Y = normalise(px[idx], py[idx], dx[idx], dy[idx], w, h)
    table = samples() if table is None else table
    m, lmask, info, rms, _, _ = fit_list(model, x, y, X, Y, M, w, h, table, **opts)
    out = np.zeros(M, dtype=np.uint8)
    out[idx] = lmask
    return m, out.reshape(len(ys), len(xs)), info, rms


# ------------------------------------------------------------------ field and residual

def field_uv(m, w, h):
    """(u, v) float64 (h, w) of the pixel model m (9,)."""
    m = np.asarray(m, dtype=np.float64).ravel()
    y, x = (a.astype(np.float64) for a in np.meshgrid(np.arange(h), np.arange(w), indexing="ij"))
    with np.errstate(all="ignore"):
        wv = (m[6] * x + m[7] * y) + m[8]
        u = ((m[0] * x + m[1] * y) + m[2]) / wv - x
        v = ((m[3] * x + m[4] * y) + m[5]) / wv - y
    bad = ~(wv > 0.0)
    u[bad] = np.nan
    v[bad] = np.nan
    return u, v


def field(models, w, h, dtype=np.float32, layout="planar"):
    """foto_motion_field_dev: models (9,) -> one record, (R, 9) -> R records."""
    ms = np.asarray(models, dtype=np.float64)
    recs = []
    for m in ms.reshape(-1, 9):
        u, v = field_uv(m, w, h)
        recs.append(np.stack([u, v, np.zeros_like(u)]) if layout == "planar" else np.stack([u, v], -1))
    out = np.stack(recs).astype(dtype)
    return out[0] if ms.ndim == 1 else out


def residual(flow, models, layout="planar"):
    """foto_motion_residual_dev: flow of one record or (R, ...) records; models (9,) or (R, 9)."""
    f = np.asarray(flow)
    batched = f.ndim == 4
    fr = f if batched else f[None]
    h, w = fr.shape[2:] if layout == "planar" else fr.shape[1:3]
    ms = np.asarray(models, dtype=np.float64).reshape(-1, 9)
    out = fr.copy()
    for r in range(len(fr)):
        u, v = field_uv(ms[r if len(ms) > 1 else 0], w, h)
        fu, fv = flow_uv(fr[r], layout)
        if layout == "planar":
            out[r, 0], out[r, 1] = (fu - u).astype(f.dtype), (fv - v).astype(f.dtype)
        else:
            out[r, ..., 0], out[r, ..., 1] = (fu - u).astype(f.dtype), (fv - v).astype(f.dtype)
    return out if batched else out[0]


# ------------------------------------------------------------------ fixtures

def true_matrix(model, w, h, rng):
    """A plausible pixel model of the kind: a few pixels of shift, a few per cent of scale, roll and
    shear, a perspective term that changes wv by a few per cent over the frame."""
    model = MODELS.get(model, model)
    tx, ty = rng.uniform(-4, 4, 2)
    m = np.array([1.0, 0, tx, 0, 1.0, ty, 0, 0, 1.0])
    if model >= SIMILARITY:
        a, sc = rng.uniform(-0.05, 0.05), 1.0 + rng.uniform(-0.04, 0.04)
        m[0], m[1], m[3], m[4] = sc * np.cos(a), -sc * np.sin(a), sc * np.sin(a), sc * np.cos(a)
        # about the frame centre
        cx, cy = 0.5 * (w - 1), 0.5 * (h - 1)
        m[2] += cx - (m[0] * cx + m[1] * cy)
        m[5] += cy - (m[3] * cx + m[4] * cy)
    if model >= AFFINE:
        m[1] += rng.uniform(-0.03, 0.03)
        m[3] += rng.uniform(-0.03, 0.03)
    if model == HOMOGRAPHY:
        m[6], m[7] = rng.uniform(-3e-4, 3e-4, 2)
    return m


def apply(m, px, py):
    wv = m[6] * px + m[7] * py + m[8]
    return (m[0] * px + m[1] * py + m[2]) / wv, (m[3] * px + m[4] * py + m[5]) / wv


def synthetic(model, w, h, M, outliers, seed, noise=0.05, span=15.0):
    """Correspondences of a true model with Gaussian noise and a share of them displaced by up to
    +-span px per axis: (points (M, 2), disp (M, 2), displaced bool (M,), shift (M,), true m)."""
    rng = np.random.default_rng(seed)
    m = true_matrix(model, w, h, rng)
    p = np.column_stack([rng.uniform(0, w - 1, M), rng.uniform(0, h - 1, M)])
    ex, ey = apply(m, p[:, 0], p[:, 1])
    d = np.column_stack([ex - p[:, 0], ey - p[:, 1]]) + rng.normal(0.0, noise, (M, 2))
    bad = np.zeros(M, dtype=bool)
    bad[rng.permutation(M)[:int(round(outliers * M))]] = True
    shift = rng.uniform(-span, span, (M, 2)) * bad[:, None]
    return p, d + shift, bad, np.hypot(shift[:, 0], shift[:, 1]), m
