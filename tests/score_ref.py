"""The scoring definitions of include/foto.h ("scoring") restated in numpy: the yardstick of
tests/test_score_host.py and tests/test_gpu_score.py, beside oracle.foto_oracle.EE / AE / IE for the
quantities the reference has.

Per pixel, on values widened to float64, in the reference's operations (utils.py:294-338):
    EE = sqrt((u - uGT)^2 + (v - vGT)^2)
    AE = arccos((1 + u uGT + v vGT) / (sqrt(1 + u^2 + v^2) sqrt(1 + uGT^2 + vGT^2)))
valid: mask non-zero (when given) and |uGT| <= 1e9, |vGT| <= 1e9, neither NaN; EE kept where valid
and EE <= ee_cap, AE kept where valid and not NaN.  R(t): the fraction of the kept errors strictly
above t.  A(p): the k-th smallest kept error by np.sort, k = max(1, ceil(p n / 100)) in float64.
Table columns: 0 n_valid | 1 n_EE, 2 mean, 3 std, 4 max, 5-8 R, 9-12 A | 13 n_AE, 14 mean, 15 std,
16 max, 17-20 R, 21-24 A | 25-31 zero; unused R / A slots and every statistic of an empty set NaN.
"""
import numpy as np

COLS = 32
EE_THR = (0.5, 1.0, 2.0)
AE_THR = tuple(float(np.deg2rad(d)) for d in (2.5, 5.0, 10.0))
PCT = (50.0, 75.0, 95.0)


def split_uv(flow, layout):
    """(u, v) as float64 [R][h][w] of a planar ([R,] 3, h, w) or interleaved ([R,] h, w, 2) flow."""
    a = np.asarray(flow)
    if layout == "planar":
        a = a if a.ndim == 4 else a[None]
        return a[:, 0].astype(np.float64), a[:, 1].astype(np.float64)
    a = a if a.ndim == 4 else a[None]
    return a[..., 0].astype(np.float64), a[..., 1].astype(np.float64)


def rank(p, n):
    """k of A(p) among n kept errors, 1-based: max(1, ceil(p n / 100)) in float64."""
    return max(1, int(np.ceil(float(p) * float(n) / 100.0)))


def _quantity(row, x, kept, thr, pct):
    """n, mean, std, max, R[4], A[4] of the kept values of x into row[0..12)."""
    row[:] = np.nan
    k = x[kept]
    n = k.size
    row[0] = n
    if n == 0:
        return
    mean = np.sum(k) / n
    row[1] = mean
    row[2] = np.sqrt(np.sum((k - mean) ** 2) / n)
    row[3] = np.max(k)
    for i, t in enumerate(thr):
        row[4 + i] = np.count_nonzero(k > t) / n
    s = np.sort(k)
    for j, p in enumerate(pct):
        row[8 + j] = s[rank(p, n) - 1]


def errors(u, v, uG, vG):
    """(EE, AE) per pixel in the reference's operations."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        du, dv = u - uG, v - vG
        ee = np.sqrt(du * du + dv * dv)
        ae = np.arccos((1.0 + u * uG + v * vG) / (np.sqrt(1.0 + u * u + v * v) * np.sqrt(1.0 + uG * uG + vG * vG)))
    return ee, ae


def score_flow(flow, gt, layout="planar", gt_layout="interleaved", mask=None, ee_cap=50.0, ee_thr=EE_THR,
               ae_thr=AE_THR, pct=PCT):
    """(table [R][32], maps [R][2][h][w] float64: EE and AE, NaN where the pixel is not valid)."""
    u, v = split_uv(flow, layout)
    uG, vG = split_uv(gt, gt_layout)
    R, h, w = u.shape
    table = np.zeros((R, COLS))
    maps = np.full((R, 2, h, w), np.nan)
    for r in range(R):
        g = 0 if uG.shape[0] == 1 else r
        ee, ae = errors(u[r], v[r], uG[g], vG[g])
        with np.errstate(invalid="ignore"):
            valid = (np.abs(uG[g]) <= 1e9) & (np.abs(vG[g]) <= 1e9)   # (a NaN compares false)
            if mask is not None:
                valid &= np.asarray(mask) != 0
            keep_e = valid & (ee <= ee_cap)
        keep_a = valid & ~np.isnan(ae)
        table[r, 0] = np.count_nonzero(valid)
        _quantity(table[r, 1:13], ee, keep_e, ee_thr, pct)
        _quantity(table[r, 13:25], ae, keep_a, ae_thr, pct)
        maps[r, 0][valid] = ee[valid]
        maps[r, 1][valid] = ae[valid]
    return table, maps


def score_frames(frames, truth, mask=None, ne_eps=1.0, divisor=None):
    """table [K][4] = n, IE, NE, max |255 I - 255 T|; frames (K, h, w) or (h, w), uint8 values
    divided by 255 (``divisor`` None), np.gradient for the gradient of 255 T."""
    def val(a):
        a = np.asarray(a)
        d = divisor if divisor is not None else (255.0 if a.dtype == np.uint8 else 1.0)
        a = a.astype(np.float64)
        return a if d == 1.0 else a / d

    I = val(frames)
    I = I if I.ndim == 3 else I[None]
    T = 255 * val(truth)
    h, w = T.shape
    gy = np.gradient(T, axis=0) if h > 1 else np.zeros_like(T)
    gx = np.gradient(T, axis=1) if w > 1 else np.zeros_like(T)
    den = gx * gx + gy * gy + ne_eps
    keep = np.ones((h, w), bool) if mask is None else np.asarray(mask) != 0
    out = np.full((I.shape[0], 4), np.nan)
    for k in range(I.shape[0]):
        d = (255 * I[k] - T)[keep]
        n = d.size
        out[k, 0] = n
        if n:
            out[k, 1] = np.sqrt(np.sum(d * d) / n)
            out[k, 2] = np.sqrt(np.sum(d * d / den[keep]) / n)
            out[k, 3] = np.max(np.abs(d))
    return out
