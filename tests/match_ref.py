"""Numpy restatement of the feature-matching entries (include/foto.h, "feature matching"): the
host tables, the binary descriptors at points, the Hamming matcher and the mutual check -- the
yardstick of tests/test_match_host.py and tests/test_gpu_match.py.  Built on sparse_ref's box sum
and on nothing else.  The two moment sums are written in the order the kernel evaluates them;
everything else is integer, so the device is held to all of it bit for bit."""
import numpy as np

import sparse_ref as S

DESCRIBE_DEFAULTS = dict(blur=2, patch=15, orientations=1)
MATCH_DEFAULTS = dict(max_disp=0.0, max_dist=64, ratio=205)
NONE, OUT, NONFINITE, NOT_MUTUAL, AMBIGUOUS = 1, 2, 4, 8, 16
MAX_PATCH, MAX_ORIENT, MAX_BLUR = 31, 32, 7
TESTS, FAR = 256, 257
_QUARTERS = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))

if hasattr(np, "bitwise_count"):
    def popcount(a):
        return np.bitwise_count(a).astype(np.int64)
else:
    _LUT = np.array([bin(v).count("1") for v in range(1 << 16)], dtype=np.int64)

    def popcount(a):
        a = np.asarray(a, dtype=np.uint64)
        m = np.uint64(0xFFFF)
        return (_LUT[a & m] + _LUT[(a >> np.uint64(16)) & m] + _LUT[(a >> np.uint64(32)) & m]
                + _LUT[(a >> np.uint64(48)) & m])


# ------------------------------------------------------------------ host tables

def directions(K):
    """(cos, sin)(2 pi k / K), exact 0 / +-1 at the multiples of pi / 2: float64 (K, 2)."""
    a = 2.0 * np.pi * np.arange(K, dtype=np.float64) / float(K)
    d = np.stack([np.cos(a), np.sin(a)], axis=1)
    for k in range(K):
        if (4 * k) % K == 0:
            d[k] = _QUARTERS[(4 * k // K) % 4]
    return d


def into_disc(x, y, patch):
    while x * x + y * y > patch * patch:
        if abs(x) >= abs(y):
            x -= int(np.sign(x))
        else:
            y -= int(np.sign(y))
    return x, y


def pattern(orientations=1, patch=15, seed=0):
    """int8 (K, 256, 4) = (ax, ay, bx, by): bin 0 from N(0, (patch / 2.5)^2), rounded, a pair redrawn
    until both ends are in the disc; bin k: bin 0 rotated by directions(K)[k], rinted, clipped."""
    K = int(orientations)
    dirs = directions(K)
    rng = np.random.default_rng(seed)
    base = np.empty((TESTS, 4), dtype=np.int64)
    for t in range(TESTS):
        while True:
            v = np.rint(rng.normal(0.0, patch / 2.5, 4)).astype(np.int64)
            if v[0] * v[0] + v[1] * v[1] <= patch * patch and v[2] * v[2] + v[3] * v[3] <= patch * patch:
                break
        base[t] = v
    out = np.empty((K, TESTS, 4), dtype=np.int8)
    x, y = base[:, 0::2].astype(np.float64), base[:, 1::2].astype(np.float64)
    for k in range(K):
        c, s = dirs[k]
        rx, ry = np.rint(c * x - s * y).astype(np.int64), np.rint(s * x + c * y).astype(np.int64)
        for t in range(TESTS):
            for e in range(2):
                out[k, t, 2 * e], out[k, t, 2 * e + 1] = into_disc(int(rx[t, e]), int(ry[t, e]), patch)
    return out


# ------------------------------------------------------------------ descriptors

def smoothed(F, blur):
    """B: the undivided (2 blur + 1)^2 box sum of the (h, w) frame, +0.0 outside; blur 0: the frame."""
    return S.box_sum(F, blur) if blur > 0 else F


def lane_sum(V):
    """(M, n) terms in the lane order: padded with +0.0 to (slots, 64), the slots of a lane added in
    increasing e from the first term, then the tree a[p] += a[p + o], o = 32 .. 1."""
    M, n = V.shape
    slots = (n + 63) // 64
    P = np.zeros((M, slots * 64))
    P[:, :n] = V
    P = P.reshape(M, slots, 64)
    a = P[:, 0].copy()
    for q in range(1, slots):
        a = a + P[:, q]
    for o in (32, 16, 8, 4, 2, 1):
        a = a[:, :o] + a[:, o:2 * o]
    return a[:, 0]


def describe(F, pts, blur=2, patch=15, orientations=1, table=None, seed=0):
    """(desc uint64 (M, 4), state uint8 (M,), bin int32 (M,)) of the points ``pts`` ((M, 2), float32
    or float64) in the widened (h, w) frame ``F``."""
    F = np.asarray(F, dtype=np.float64)
    h, w = F.shape
    K, R = int(orientations), int(patch)
    tab = pattern(K, R, seed) if table is None else np.asarray(table)
    dirs = directions(K)
    B = smoothed(F, blur)
    p = np.asarray(pts).astype(np.float64).reshape(-1, 2)
    M = len(p)
    desc = np.zeros((M, 4), dtype=np.uint64)
    state = np.zeros(M, dtype=np.uint8)
    bins = np.full(M, -1, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        fi, fj = np.floor(p[:, 0] + 0.5), np.floor(p[:, 1] + 0.5)
        fin = np.isfinite(p[:, 0]) & np.isfinite(p[:, 1])
        inside = (fi >= R) & (fi <= w - 1 - R) & (fj >= R) & (fj <= h - 1 - R)
    state[~fin] = NONFINITE | OUT
    state[fin & ~inside] = OUT
    ok = np.flatnonzero(state == 0)
    if not len(ok):
        return desc, state, bins
    i, j = fi[ok].astype(np.int64), fj[ok].astype(np.int64)
    b = np.zeros(len(ok), dtype=np.int64)
    if K > 1:
        side = 2 * R + 1
        e = np.arange(side * side)
        ay, ax = e // side - R, e % side - R
        on = ax * ax + ay * ay <= R * R
        with np.errstate(invalid="ignore", over="ignore"):
            v = F[j[:, None] + ay[None, :], i[:, None] + ax[None, :]]
            m10 = lane_sum(np.where(on[None, :], ax.astype(np.float64)[None, :] * v, 0.0))
            m01 = lane_sum(np.where(on[None, :], ay.astype(np.float64)[None, :] * v, 0.0))
            held = m10 * dirs[0, 0] + m01 * dirs[0, 1]
            for k in range(1, K):
                val = m10 * dirs[k, 0] + m01 * dirs[k, 1]
                better = val > held
                held = np.where(better, val, held)
                b = np.where(better, k, b)
    t = tab[b].astype(np.int64)   # (m, 256, 4)
    with np.errstate(invalid="ignore"):
        bit = B[j[:, None] + t[:, :, 1], i[:, None] + t[:, :, 0]] < B[j[:, None] + t[:, :, 3], i[:, None] + t[:, :, 2]]
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    words = (bit.reshape(len(ok), 4, 64).astype(np.uint64) * weights[None, None, :]).sum(axis=2, dtype=np.uint64)
    desc[ok] = words
    bins[ok] = b
    return desc, state, bins


# ------------------------------------------------------------------ the matcher

def distances(desc0, desc1):
    """d(i, j): the set bits of desc0[i] XOR desc1[j] over the four words, int64 (N0, N1)."""
    d = np.zeros((len(desc0), len(desc1)), dtype=np.int64)
    for k in range(4):
        d += popcount(desc0[:, None, k] ^ desc1[None, :, k])
    return d


def match(desc0, state0, pts0, desc1, state1, pts1, max_disp=0.0, max_dist=64, ratio=205, dtype=np.float32):
    """(idx int32 (N0,), dist int32 (N0, 2), status uint8 (N0,), disp (N0, 2) of ``dtype``)."""
    p0, p1 = np.asarray(pts0).astype(np.float64).reshape(-1, 2), np.asarray(pts1).astype(np.float64).reshape(-1, 2)
    N0, N1 = len(p0), len(p1)
    cand = np.broadcast_to((np.asarray(state1) == 0)[None, :], (N0, N1)).copy()
    if max_disp != 0:
        with np.errstate(invalid="ignore"):
            cand &= (np.abs(p1[None, :, 0] - p0[:, None, 0]) <= max_disp) & (np.abs(p1[None, :, 1] - p0[:, None, 1]) <= max_disp)
    key = np.where(cand, distances(desc0, desc1), FAR)
    j1 = np.argmin(key, axis=1)            # (the first minimum: ties go to the lower j)
    rows = np.arange(N0)
    d1 = key[rows, j1]
    rest = key.copy()
    rest[rows, j1] = FAR
    d2 = rest.min(axis=1)
    idx = np.where(d1 < FAR, j1, -1).astype(np.int32)
    status = np.zeros(N0, dtype=np.uint8)
    status[(idx < 0) | (d1 > max_dist)] |= NONE
    if ratio != 0:
        status[~(d1 * 256 < ratio * d2)] |= AMBIGUOUS
    idx[(status & NONE) != 0] = -1
    s0 = np.asarray(state0, dtype=np.uint8)
    bad = s0 != 0
    status[bad] = s0[bad]
    idx[bad] = -1
    dist = np.stack([d1, d2], axis=1).astype(np.int32)
    dist[bad] = FAR
    disp = np.full((N0, 2), np.nan)
    has = idx >= 0
    disp[has] = p1[idx[has]] - p0[has]
    return idx, dist, status, disp.astype(dtype)


def cross(idx01, idx10, status):
    """status with NOT_MUTUAL where idx01[i] >= 0 and idx10[idx01[i]] != i (a copy)."""
    idx01, idx10 = np.asarray(idx01), np.asarray(idx10)
    out = np.array(status, dtype=np.uint8).copy()
    has = idx01 >= 0
    j = np.clip(idx01, 0, len(idx10) - 1)
    out[has & ((idx01 >= len(idx10)) | (idx10[j] != np.arange(len(idx01))))] |= NOT_MUTUAL
    return out


def match_checked(desc0, state0, pts0, desc1, state1, pts1, **kw):
    """Both directions and the mutual check: (idx, dist, status, disp)."""
    idx, dist, status, disp = match(desc0, state0, pts0, desc1, state1, pts1, **kw)
    idx10 = match(desc1, state1, pts1, desc0, state0, pts0, **kw)[0]
    return idx, dist, cross(idx, idx10, status), disp


def match_frames(f0, f1, w, h, max_corners, check=True, corner_opts=None, dtype=np.float32, blur=2, patch=15,
                 orientations=1, seed=0, **m_opts):
    """foto.device.match_frames restated: (points, disp, status, idx, dist)."""
    co = dict(S.CORNER_DEFAULTS, **(corner_opts or {}))
    co["margin"] = max(co["margin"], patch)
    F0, F1 = np.asarray(f0, dtype=np.float64).reshape(h, w), np.asarray(f1, dtype=np.float64).reshape(h, w)
    p0 = S.corners(F0.ravel(), w, h, max_corners, **co)[0].astype(dtype)
    p1 = S.corners(F1.ravel(), w, h, max_corners, **co)[0].astype(dtype)
    tab = pattern(orientations, patch, seed)
    d0, s0, _ = describe(F0, p0, blur, patch, orientations, tab)
    d1, s1, _ = describe(F1, p1, blur, patch, orientations, tab)
    fn = match_checked if check else match
    idx, dist, status, disp = fn(d0, s0, p0, d1, s1, p1, dtype=dtype, **m_opts)
    return p0, disp, status, idx, dist


def same(a, b):
    """Bit equality for the tests: equal values, NaN where NaN."""
    return S.same(a, b)
