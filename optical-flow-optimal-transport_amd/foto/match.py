"""Feature matching on the device (csrc/foto_match.hip; include/foto.h, "feature matching"): the
stage between ``foto.sparse.corners`` and ``foto.motion.fit`` for motion a differential tracker
cannot follow -- a pan of a third of the frame, a roll of the camera.

``pattern``      the host table of test pairs, per orientation bin (numpy; the device draws nothing)
``directions``   the host table of the bins' directions
``describe``     256-bit binary descriptors of the neighbourhoods of device points
``match``        nearest and second-nearest descriptor under the Hamming distance, with a distance
                 bound, Lowe's ratio and a spatial gate: what ``foto.motion.fit`` takes as
                 (points, disp, status)
``cross``        the mutual check of two ``match`` calls

Everything stays in device memory and nothing here waits for the device.
"""
import ctypes
import functools

import numpy as np

from . import _lib
from . import device as D
from ._lib import check, lib

DESCRIBE_DEFAULTS = dict(blur=2, patch=15, orientations=1)
MATCH_DEFAULTS = dict(max_disp=0.0, max_dist=64, ratio=0.8)
NONE, OUT, NONFINITE, NOT_MUTUAL, AMBIGUOUS = (_lib.FOTO_MATCH_NONE, _lib.FOTO_MATCH_OUT, _lib.FOTO_MATCH_NONFINITE,
                                               _lib.FOTO_MATCH_NOT_MUTUAL, _lib.FOTO_MATCH_AMBIGUOUS)
TESTS = 256
_U8 = {"uint8": _lib.FOTO_U8}
_I32 = {"int32": 0}
_U64 = {"uint64": 0}
_QUARTERS = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))


def directions(K):
    """(cos, sin)(2 pi k / K), k < K, as a float64 (K, 2) host array, with exact 0 / +-1 at the
    multiples of pi / 2."""
    K = int(K)
    if not 1 <= K <= _lib.FOTO_MATCH_MAX_ORIENT:
        raise ValueError(f"orientations = {K}: 1 .. {_lib.FOTO_MATCH_MAX_ORIENT} bins")
    a = 2.0 * np.pi * np.arange(K, dtype=np.float64) / float(K)
    d = np.stack([np.cos(a), np.sin(a)], axis=1)
    for k in range(K):
        if (4 * k) % K == 0:
            d[k] = _QUARTERS[(4 * k // K) % 4]
    return d


def _into_disc(x, y, patch):
    """An integer offset clipped to the disc x x + y y <= patch patch: the coordinate of the larger
    magnitude (x on a tie) moves one step towards 0 until it is inside."""
    while x * x + y * y > patch * patch:
        if abs(x) >= abs(y):
            x -= int(np.sign(x))
        else:
            y -= int(np.sign(y))
    return x, y


def pattern(orientations=1, patch=15, seed=0):
    """The test pairs as an int8 (K, 256, 4) host array of (ax, ay, bx, by), reproducible per seed.
    Bin 0: 256 pairs whose four offsets are drawn from an isotropic Gaussian of standard deviation
    patch / 2.5 (BRIEF's G II), rounded, the pair redrawn until both ends lie in the disc of radius
    ``patch``.  Bin k: bin 0's offsets rotated by 2 pi k / K with ``directions``' (c, s) in float64,
    (c x - s y, s x + c y), np.rint-ed and clipped to the disc -- for K = 4 the exact integer
    rotation (x, y) -> (-y, x), repeated."""
    K, patch = int(orientations), int(patch)
    if not 2 <= patch <= _lib.FOTO_MATCH_MAX_PATCH:
        raise ValueError(f"patch = {patch}: the disc's radius is 2 .. {_lib.FOTO_MATCH_MAX_PATCH}")
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
                out[k, t, 2 * e], out[k, t, 2 * e + 1] = _into_disc(int(rx[t, e]), int(ry[t, e]), patch)
    return out


@functools.lru_cache(maxsize=8)
def _cached_pattern(orientations, patch, seed):
    t = pattern(orientations, patch, seed)
    t.setflags(write=False)
    return t


def _table(table, K, patch, seed):
    t = _cached_pattern(K, patch, seed) if table is None else np.ascontiguousarray(table)
    if t.dtype != np.int8 or t.shape != (K, TESTS, 4):
        raise ValueError(f"table: an int8 ({K}, {TESTS}, 4) host array (foto.match.pattern); got {t.dtype} {t.shape}")
    return t


def describe(frame, points, *, blur=DESCRIBE_DEFAULTS["blur"], patch=DESCRIBE_DEFAULTS["patch"],
             orientations=DESCRIBE_DEFAULTS["orientations"], seed=0, table=None, return_bin=False, divisor=None,
             stream=None):
    """The binary descriptors of the device points ``points`` ((M, 2) float32 | float64, e.g.
    ``foto.sparse.corners``' buffer with its NaN rows) in the device frame ``frame``: (desc, state),
    or (desc, state, bin) with ``return_bin``.  desc: uint64 (M, 4); state: uint8 (M,), 0 = described,
    OUT where the patch leaves the frame, NONFINITE | OUT for a NaN or Inf point (zero words);
    bin: int32 (M,), the orientation bin or -1.  ``table``: foto.match.pattern's array for
    (orientations, patch); None: that of ``seed``."""
    im = D.as_image(frame, divisor)
    h, w = im.shape
    pptr, pcode, M = D.track_source(points)
    o = _lib.DescribeOpts(int(blur), int(patch), int(orientations), 0)
    dirs = directions(o.orientations)
    if not 2 <= o.patch <= _lib.FOTO_MATCH_MAX_PATCH:
        raise ValueError(f"patch = {o.patch}: the disc's radius is 2 .. {_lib.FOTO_MATCH_MAX_PATCH}")
    t = _table(table, o.orientations, o.patch, seed)
    desc = D.DeviceArray((M, 4), np.uint64)
    state = D.DeviceArray((M,), np.uint8)
    b = D.DeviceArray((M,), np.int32) if return_bin else None
    check(lib().foto_describe_dev(ctypes.byref(im), w, h, ctypes.c_void_p(pptr), pcode, M, ctypes.byref(o),
                                  t.ctypes.data_as(ctypes.c_void_p), dirs.ctypes.data_as(ctypes.c_void_p),
                                  ctypes.c_void_p(desc.ptr), ctypes.c_void_p(state.ptr),
                                  ctypes.c_void_p(b.ptr) if return_bin else None,
                                  ctypes.c_void_p(D.stream_handle(stream, frame, points))))
    return (desc, state, b) if return_bin else (desc, state)


def ratio_code(ratio):
    """Lowe's ratio in 1 / 256: a float becomes int(round(ratio 256)), None becomes 0 (no test)."""
    r = 0 if ratio is None else int(round(float(ratio) * 256))
    if not 0 <= r <= 256:
        raise ValueError(f"ratio = {ratio!r} must be in [0, 1], or None")
    return r


def match(desc0, state0, pts0, desc1, state1, pts1, *, max_disp=MATCH_DEFAULTS["max_disp"],
          max_dist=MATCH_DEFAULTS["max_dist"], ratio=MATCH_DEFAULTS["ratio"], dtype="float32", stream=None):
    """For every query (``describe``'s results for frame 0 and its points) the nearest train
    descriptor (frame 1): (idx int32 (N0,), dist int32 (N0, 2), status uint8 (N0,), disp (N0, 2) of
    ``dtype``).  idx: the match or -1; dist: the best and second-best Hamming distance, 257 = none;
    status: 0 = a match, else the query's state, NONE (no candidate, or farther than ``max_dist``),
    AMBIGUOUS (Lowe's ``ratio`` fails); disp = pts1[idx] - pts0, NaN without a match.  ``max_disp``
    > 0: only train points within that many pixels in x and in y are candidates."""
    p0, c0, N0 = D.track_source(pts0)
    p1, c1, N1 = D.track_source(pts1)
    _, d0, _ = D._shaped_target(desc0, "uint64", _U64, (N0, 4), "descriptors")
    _, d1, _ = D._shaped_target(desc1, "uint64", _U64, (N1, 4), "descriptors")
    _, s0, _ = D._shaped_target(state0, "uint8", _U8, (N0,), "state bytes")
    _, s1, _ = D._shaped_target(state1, "uint8", _U8, (N1,), "state bytes")
    o = _lib.MatchOpts(float(max_disp), int(max_dist), ratio_code(ratio), (ctypes.c_int * 2)(0, 0))
    idx, dist = D.DeviceArray((N0,), np.int32), D.DeviceArray((N0, 2), np.int32)
    status = D.DeviceArray((N0,), np.uint8)
    disp, dp, dcode = D._shaped_target(None, dtype, D._OUT_DTYPES, (N0, 2), "displacements")
    check(lib().foto_match_dev(ctypes.c_void_p(d0), ctypes.c_void_p(s0), ctypes.c_void_p(p0), c0, N0,
                               ctypes.c_void_p(d1), ctypes.c_void_p(s1), ctypes.c_void_p(p1), c1, N1, ctypes.byref(o),
                               ctypes.c_void_p(idx.ptr), ctypes.c_void_p(dist.ptr), ctypes.c_void_p(status.ptr),
                               ctypes.c_void_p(dp), dcode,
                               ctypes.c_void_p(D.stream_handle(stream, desc0, desc1, pts0, pts1))))
    return idx, dist, status, disp


def cross(idx01, idx10, status, *, stream=None):
    """The mutual check: NOT_MUTUAL is ORed into ``status`` (of the 0 -> 1 ``match``) where the match
    of query i does not match back to i; ``idx01``, ``idx10``: the two calls' idx.  Returns status."""
    (N0,), (N1,) = D.device_interface(idx01)[2], D.device_interface(idx10)[2]
    _, a, _ = D._shaped_target(idx01, "int32", _I32, (N0,), "indices")
    _, b, _ = D._shaped_target(idx10, "int32", _I32, (N1,), "indices")
    _, s, _ = D._shaped_target(status, "uint8", _U8, (N0,), "status bytes")
    check(lib().foto_match_cross_dev(ctypes.c_void_p(a), N0, ctypes.c_void_p(b), N1, ctypes.c_void_p(s),
                                     ctypes.c_void_p(D.stream_handle(stream, idx01, idx10))))
    return status
