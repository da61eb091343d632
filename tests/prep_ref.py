"""Numpy restatement of the frame preparation section of include/foto.h: the yardstick of
tests/test_gpu_prep.py (PIL need not be installed where the GPU tests run), itself pinned to Pillow's
Image.resize / convert('L') and to the bin/ tools by tests/test_prep_host.py.

Every function follows the operation order the header states, so a comparison is on bit patterns.
The transcendental of the Lanczos kernel is math.sin, the C library's, like the library's host code.
"""
import math

import numpy as np

FILTERS = {"box": 0, "bilinear": 1, "bicubic": 2, "lanczos": 3}
SUPPORT = {"box": 0.5, "bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}
PRECISION_BITS = 22


# ------------------------------------------------------------------ grey

def gray(a):
    """(h, w, 3 | 4) -> (h, w): uint8 is PIL's convert('L'); floats use the same weights over 65536
    in float64, summed left to right, written in the input dtype.  Alpha is ignored."""
    a = np.asarray(a)
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    if a.dtype == np.uint8:
        r, g, b = (x.astype(np.int64) for x in (r, g, b))
        return ((19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16).astype(np.uint8)
    r, g, b = (x.astype(np.float64) for x in (r, g, b))
    return (((19595 / 65536) * r + (38470 / 65536) * g) + (7471 / 65536) * b).astype(a.dtype)


# ------------------------------------------------------------------ resize

def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _filter(name, x):
    if name == "box":
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if name == "bilinear":
        x = abs(x)
        return 1.0 - x if x < 1.0 else 0.0
    if name == "bicubic":
        x = abs(x)
        if x < 1.0:
            return (1.5 * x - 2.5) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * -0.5
        return 0.0
    if name == "lanczos":
        return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    raise ValueError(name)


def coeffs(n_in, n_out, filt):
    """Pillow's precompute_coeffs for the whole axis: (ksize, bounds int32 (n_out, 2) = (first tap,
    tap count), kk float64 (n_out, ksize), zero beyond the count)."""
    scale = float(np.float32(n_in)) / n_out
    filterscale = max(scale, 1.0)
    support = SUPPORT[filt] * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), np.int32)
    kk = np.zeros((n_out, ksize), np.float64)
    ss = 1.0 / filterscale
    for xx in range(n_out):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        ww = 0.0
        for x in range(xmax):
            w = _filter(filt, (x + xmin - center + 0.5) * ss)
            kk[xx, x] = w
            ww += w
        if ww != 0.0:
            for x in range(xmax):
                kk[xx, x] /= ww
        bounds[xx] = (xmin, xmax)
    return ksize, bounds, kk


def coeffs_int(kk):
    """Pillow's normalize_coeffs_8bpc: (int)(+-0.5 + k 2^22), truncating toward zero."""
    x = kk * float(1 << PRECISION_BITS)
    return np.where(kk < 0, np.trunc(-0.5 + x), np.trunc(0.5 + x)).astype(np.int32)


def _pass(a, n_out, filt, axis, scale=1.0, last=True):
    """One pass of a 2-D array along `axis` (1: horizontal, 0: vertical).  `scale` multiplies the
    float accumulator before the final rounding (the flow resize; 1 for frames)."""
    a = a if axis == 1 else a.T
    _, bounds, kk = coeffs(a.shape[1], n_out, filt)
    out = np.empty((a.shape[0], n_out), a.dtype)
    if a.dtype == np.uint8:
        ki = coeffs_int(kk)
        src = a.astype(np.int32)
        for xx in range(n_out):
            acc = np.full(a.shape[0], 1 << (PRECISION_BITS - 1), np.int32)
            for t in range(bounds[xx, 1]):
                acc = acc + src[:, bounds[xx, 0] + t] * ki[xx, t]
            out[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    else:
        src = a.astype(np.float64)
        for xx in range(n_out):
            acc = np.zeros(a.shape[0], np.float64)
            for t in range(bounds[xx, 1]):
                acc = acc + src[:, bounds[xx, 0] + t] * kk[xx, t]
            out[:, xx] = acc * scale if last else acc
    return out if axis == 1 else out.T


def resize2d(a, size, filt, scale=1.0):
    """PIL's Image.resize of one 2-D uint8 ('L') / float32 ('F') / float64 plane to size = (ow, oh):
    horizontal pass, then vertical, a pass skipped when its size does not change.  `scale` is
    applied in the last pass that runs."""
    ow, oh = size
    h, w = a.shape
    need_h, need_v = ow != w, oh != h
    if need_h:
        a = _pass(a, ow, filt, 1, scale, last=not need_v)
    if need_v:
        a = _pass(a, oh, filt, 0, scale, last=True)
    return np.array(a)


def resize(a, size, filt="lanczos"):
    """resize2d of a (h, w) frame or of every channel of a (h, w, C) one."""
    a = np.asarray(a)
    if a.ndim == 2:
        return resize2d(a, size, filt)
    return np.stack([resize2d(a[..., c], size, filt) for c in range(a.shape[2])], axis=2)


def resize_flow(f, layout, size, filt="bilinear"):
    """Every record and plane of a flow through the float path; u scaled by ow / w, v by oh / h in
    the last pass, before the final rounding; m unscaled.  planar (R, 3, h, w), interleaved
    (R, h, w, 2)."""
    ow, oh = size
    f = np.asarray(f)
    if layout == "planar":
        R, _, h, w = f.shape
        sc = (ow / w, oh / h, 1.0)
        out = np.empty((R, 3, oh, ow), f.dtype)
        for r in range(R):
            for p in range(3):
                out[r, p] = resize2d(f[r, p], size, filt, sc[p])
        return out
    R, h, w, _ = f.shape
    sc = (ow / w, oh / h)
    out = np.empty((R, oh, ow, 2), f.dtype)
    for r in range(R):
        for c in range(2):
            out[r, :, :, c] = resize2d(f[r, :, :, c], size, filt, sc[c])
    return out


# ------------------------------------------------------------------ pointwise stages

def values(a, divisor=None):
    """(double)pixel / divisor, divisor 255 for uint8 and 1 otherwise."""
    a = np.asarray(a)
    d = divisor if divisor is not None else (255.0 if a.dtype == np.uint8 else 1.0)
    return a.astype(np.float64) / d


def out_cast(x, dtype):
    """uint8: the truncating np.uint8(255 clip(x, 0, 1)), NaN -> 0; floats: the value itself."""
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        with np.errstate(invalid="ignore"):
            y = 255 * np.clip(x, 0, 1)
        return np.where(np.isnan(y), 0, y).astype(np.int32).astype(np.uint8)
    return x.astype(dtype)


def normalize_pair(f0, f1, S0, S1, dtype="uint8", divisor=None):
    """bin/normalize_image.py with the sums given: out = (v / S) / scale, scale = max(max0 / S0,
    max1 / S1).  Returns (out0, out1, (max0, max1))."""
    v0, v1 = values(f0, divisor), values(f1, divisor)
    m0, m1 = np.max(v0), np.max(v1)
    scale = max(m0 / S0, m1 / S1)
    return out_cast((v0 / S0) / scale, dtype), out_cast((v1 / S1) / scale, dtype), (m0, m1)


def illuminate(f, shapes, dtype="uint8", divisor=None):
    """bin/create_lum_dataset.py's additions on a (h, w) frame, in list order: ("rect", L_x, L_y,
    r_x, r_y, v) adds v on int(r - L / 2) <= index < int(r + L / 2) (clipped to the frame), ("circle",
    R, c_x, c_y, v) where (i - c_x)^2 + (j - c_y)^2 < R^2."""
    x = values(f, divisor).copy()
    h, w = x.shape
    jj, ii = np.mgrid[0:h, 0:w]
    for s in shapes:
        if s[0] == "rect":
            _, L_x, L_y, r_x, r_y, v = s
            x0, x1 = max(int(r_x - L_x / 2), 0), min(int(r_x + L_x / 2), w)
            y0, y1 = max(int(r_y - L_y / 2), 0), min(int(r_y + L_y / 2), h)
            if x1 > x0 and y1 > y0:
                x[y0:y1, x0:x1] += v
        else:
            _, R, c_x, c_y, v = s
            dx, dy = ii.astype(np.float64) - c_x, jj.astype(np.float64) - c_y
            x[dx * dx + dy * dy < R * R] += v
    return out_cast(x, dtype)


def difference(f0, f1, dtype="uint8", divisor=None):
    """bin/data_diff.py: d = v1 - v0, (d - min) / (max - min); a constant d gives 0 / 0."""
    d = values(f1, divisor) - values(f0, divisor)
    mn, mx = np.min(d), np.max(d)
    with np.errstate(invalid="ignore", divide="ignore"):
        return out_cast((d - mn) / (mx - mn), dtype)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, a.dtype, b.shape, b.dtype)
    view = {1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    ai, bi = np.ascontiguousarray(a).view(view), np.ascontiguousarray(b).view(view)
    bad = np.flatnonzero(ai.ravel() != bi.ravel())
    assert bad.size == 0, (f"{bad.size} of {a.size} values differ; first at flat index {bad[0]}: "
                           f"{a.ravel()[bad[0]]!r} != {b.ravel()[bad[0]]!r}")
