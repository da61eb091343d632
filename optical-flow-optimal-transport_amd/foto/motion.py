"""Global motion on the device (csrc/foto_motion.hip; include/foto.h, "global motion"): the one
parametric motion that dominates a set of tracks or a dense flow -- a pan, a zoom, a roll, a plane
seen from a moving camera -- fitted by RANSAC, refined over its inliers, and removed.

``samples``    the host table of sample numbers a fit draws its hypotheses from
``fit``        a model fitted to device correspondences: ``foto.sparse.corners`` /
               ``LK.track``'s points, displacements and status bytes as they are
``fit_flow``   the same on a lattice of one record of a device flow buffer
``field``      a model's flow field: a flow buffer ``foto.render.reconstruct`` (stabilisation),
               ``foto.chain.compose`` and ``foto.evaluate.score_flow`` take as it is
``residual``   a flow with the model's field removed: what moves once the camera does not

Everything stays in device memory and nothing here waits for the device; a ``Fit`` downloads on
request (``matrix``, ``counts``, ``rms``).
"""
import ctypes

import numpy as np

from . import _lib
from . import device as D
from ._lib import check, lib

MODELS = {"translation": _lib.FOTO_MOTION_TRANSLATION, "similarity": _lib.FOTO_MOTION_SIMILARITY,
          "affine": _lib.FOTO_MOTION_AFFINE, "homography": _lib.FOTO_MOTION_HOMOGRAPHY}
DEFAULTS = dict(threshold=1.0, rounds=3, min_inliers=0)
NONE, KEPT = _lib.FOTO_MOTION_NONE, _lib.FOTO_MOTION_KEPT
_U8 = {"uint8": _lib.FOTO_U8}
_F64 = {"float64": _lib.FOTO_F64}


def samples(H=256, seed=0):
    """The sample numbers of ``H`` hypotheses: a uint32 (H, 4) host array, reproducible per seed.
    Point i of hypothesis j is the valid correspondence number (samples[j][i] * n_valid) >> 32, so
    one table serves every number of correspondences."""
    H = int(H)
    if H < 1:
        raise ValueError(f"H = {H} hypotheses must be >= 1")
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=(H, 4), dtype=np.uint64).astype(np.uint32)


class Fit:
    """The result of a fit, in device memory: ``model`` (float64 (3, 3), pixel coordinates, maps a
    start point to its end point), ``inliers`` (uint8, 1 = inlier) and ``info`` (uint8 (40,): the
    int64 record (inliers, n_valid, winning hypothesis, status bits), then the float64 rms)."""

    def __init__(self, model, inliers, info):
        self.model, self.inliers, self.info = model, inliers, info

    def matrix(self):
        """The 3 x 3 matrix on the host (waits)."""
        return self.model.to_numpy()

    def counts(self):
        """(inliers, n_valid, winning hypothesis or -1, status bits) as ints (waits)."""
        return tuple(int(v) for v in self.info.to_numpy()[:32].view(np.int64))

    def rms(self):
        """The root mean square of the inliers' residual in pixels; NaN without inliers (waits)."""
        return float(self.info.to_numpy()[32:].view(np.float64)[0])


def _opts(model, threshold, rounds, min_inliers):
    if model not in MODELS:
        raise ValueError(f"model {model!r}: one of {sorted(MODELS)}")
    return _lib.MotionOpts(MODELS[model], int(rounds), int(min_inliers), 0, float(threshold))


def _table(table):
    t = samples() if table is None else np.ascontiguousarray(table)
    if t.dtype != np.uint32 or t.ndim != 2 or t.shape[1] != 4 or t.shape[0] < 1:
        raise ValueError(f"samples: a uint32 (H, 4) host array (foto.motion.samples); got {t.dtype} {t.shape}")
    return t


def _results(shape):
    return D.DeviceArray((3, 3), np.float64), D.DeviceArray(shape, np.uint8), D.DeviceArray((40,), np.uint8)


def fit(points, disp, w, h, model="affine", status=None, threshold=DEFAULTS["threshold"], rounds=DEFAULTS["rounds"],
        samples=None, *, min_inliers=DEFAULTS["min_inliers"], stream=None):
    """The ``model`` ("translation", "similarity", "affine", "homography") that most of the device
    correspondences ``points`` -> ``points + disp`` ((M, 2) float32 | float64 each) of a w x h frame
    follow: a ``Fit``.  ``status``: a uint8 (M,) device array, non-zero = unusable (LK's status byte
    as it is); a NaN or Inf coordinate is unusable too.  ``samples``: foto.motion.samples' table
    (None: the default 256 of seed 0)."""
    pptr, pcode, M = D.track_source(points)
    dptr, dcode, Md = D.track_source(disp)
    if Md != M:
        raise ValueError(f"{M} points and {Md} displacements")
    sptr = None
    if status is not None:
        _, sptr, _ = D._shaped_target(status, "uint8", _U8, (M,), "status bytes")
    o, t = _opts(model, threshold, rounds, min_inliers), _table(samples)
    m, inl, info = _results((M,))
    check(lib().foto_motion_fit_dev(ctypes.c_void_p(pptr), pcode, ctypes.c_void_p(dptr), dcode,
                                    ctypes.c_void_p(sptr) if status is not None else None, M, int(w), int(h),
                                    ctypes.byref(o), t.ctypes.data_as(ctypes.c_void_p), len(t), ctypes.c_void_p(m.ptr),
                                    ctypes.c_void_p(inl.ptr), ctypes.c_void_p(info.ptr), ctypes.c_void_p(info.ptr + 32),
                                    ctypes.c_void_p(D.stream_handle(stream, points, disp))))
    return Fit(m, inl, info)


def fit_flow(flow, w=None, h=None, record=0, stride=4, mask=None, model="affine", threshold=DEFAULTS["threshold"],
             rounds=DEFAULTS["rounds"], samples=None, *, layout="planar", min_inliers=DEFAULTS["min_inliers"],
             stream=None):
    """``fit`` on record ``record`` of a device flow buffer (foto.render.flow_arg's shapes), read
    at the lattice pixels (i stride, j stride).  ``mask``: a uint8 (h, w) device array, non-zero =
    usable (foto.chain.consistency's ``valid``); a NaN flow value is unusable too.  The inlier mask
    has the lattice's shape.  ``w``, ``h``: the flow's own when None."""
    from .render import flow_arg
    fl, R, fh, fw, _ = flow_arg(flow, layout)
    if (w is not None and int(w) != fw) or (h is not None and int(h) != fh):
        raise ValueError(f"the flow is {fh} x {fw} (h x w), not {h} x {w}")
    stride = int(stride)
    if stride < 1:
        raise ValueError(f"stride = {stride} must be >= 1")
    mptr = None
    if mask is not None:
        _, mptr, _ = D._shaped_target(mask, "uint8", _U8, (fh, fw), "mask bytes")
    o, t = _opts(model, threshold, rounds, min_inliers), _table(samples)
    m, inl, info = _results(((fh - 1) // stride + 1, (fw - 1) // stride + 1))
    check(lib().foto_motion_fit_flow_dev(ctypes.byref(fl), int(record), fw, fh, stride,
                                         ctypes.c_void_p(mptr) if mask is not None else None, ctypes.byref(o),
                                         t.ctypes.data_as(ctypes.c_void_p), len(t), ctypes.c_void_p(m.ptr),
                                         ctypes.c_void_p(inl.ptr), ctypes.c_void_p(info.ptr),
                                         ctypes.c_void_p(info.ptr + 32),
                                         ctypes.c_void_p(D.stream_handle(stream, flow))))
    return Fit(m, inl, info)


def _models(model):
    """(device array, pointer, count, has_record_axis) of a ``Fit``, a float64 device (3, 3) / (9,)
    model or (R, 3, 3) / (R, 9) models."""
    if isinstance(model, Fit):
        model = model.model
    ptr, typestr, shape, strides, _ = D.device_interface(model)
    if typestr != "<f8" or shape not in ((9,), (3, 3)) and not (len(shape) >= 2 and shape[1:] in ((9,), (3, 3))):
        raise ValueError(f"model: a float64 device (3, 3) matrix or (R, 3, 3) matrices; got {typestr} {shape}")
    if not D.c_contiguous(shape, strides, 8):
        raise ValueError("model must be C-contiguous")
    batched = shape not in ((9,), (3, 3))
    return model, ptr, (int(shape[0]) if batched else 1), batched


def field(model, w, h, *, dtype="float32", layout="planar", out=None, stream=None):
    """The flow field of a model (a ``Fit`` or a float64 device (3, 3) matrix; (R, 3, 3): R records):
    a flow buffer (``foto.device.export_target``'s shapes) with (u, v) = H(x, y) - (x, y), m = 0,
    NaN where the homography's denominator is not positive."""
    keep, mptr, count, batched = _models(model)
    w, h = int(w), int(h)
    if batched:
        out, ptr, code, lay = D.path_target(out, dtype, layout, count + 1, h, w)
    else:
        out, ptr, code, lay = D.export_target(out, dtype, layout, h, w)
    check(lib().foto_motion_field_dev(ctypes.c_void_p(mptr), count, w, h, ctypes.c_void_p(ptr), code, lay,
                                      ctypes.c_void_p(D.stream_handle(stream, keep))))
    return out


def residual(flow, model, *, layout="planar", out=None, stream=None):
    """``flow`` minus the field of ``model`` (one for every record, or one per record), m copied:
    a flow buffer of the flow's shape and dtype."""
    from .render import flow_arg
    fl, R, h, w, batched = flow_arg(flow, layout)
    keep, mptr, count, _ = _models(model)
    if count not in (1, R):
        raise ValueError(f"{count} models for {R} records: one, or one per record")
    name = "float32" if fl.dtype == _lib.FOTO_F32 else "float64"
    rec = (3, h, w) if layout == "planar" else (h, w, 2)
    out, ptr, _ = D._shaped_target(out, name, D._OUT_DTYPES, ((R,) if batched else ()) + rec, "flow records")
    check(lib().foto_motion_residual_dev(ctypes.byref(fl), ctypes.c_void_p(mptr), count, w, h, ctypes.c_void_p(ptr),
                                         ctypes.c_void_p(D.stream_handle(stream, flow, keep))))
    return out
