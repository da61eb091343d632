"""Flow algebra for sequences (include/foto.h, "flow algebra"): K pair flows of K + 1 frames --
``foto.device.bb_sequence`` writes such a buffer -- chained, inverted and cross-checked on the device.

``compose``      frame 0 -> frame k for every k (or the last alone): long-range motion
``invert``       the backward flow of a forward flow, by a fixed number of fixed-point rounds
``consistency``  the forward-backward check: the validity mask ``foto.evaluate.score_flow`` takes,
                 the four class counts and, on request, the per-pixel error

A flow is what ``foto.render`` takes: a C-contiguous float32 / float64 array, "planar" (3, h, w) or
(R, 3, h, w) = u, v, m, or "interleaved" (h, w, 2) or (R, h, w, 2) = (u, v).  Device arrays
(``DeviceArray``, torch tensors, anything with ``__cuda_array_interface__``) stay on the device and
nothing waits; numpy arrays are uploaded and the results downloaded.
"""
import ctypes

import numpy as np

from . import _lib
from . import device as D
from ._lib import check, lib
from .render import _host_flow, flow_arg

INV_ITERS_DEFAULT, INV_ITERS_MAX = _lib.FOTO_INV_ITERS_DEFAULT, _lib.FOTO_INV_ITERS_MAX
ALPHA1, ALPHA2 = _lib.FOTO_CONSISTENCY_ALPHA1, _lib.FOTO_CONSISTENCY_ALPHA2
CLASSES = ("consistent", "inconsistent", "leaves the frame", "not finite")   # the columns of the table
_NAMES = {_lib.FOTO_F32: "float32", _lib.FOTO_F64: "float64"}
_F64 = {"float64": _lib.FOTO_F64}


def _rec_shape(layout, h, w):
    return (3, h, w) if layout == "planar" else (h, w, 2)


def _flow_target(fl, in_layout, dtype, layout, lead, h, w, out):
    """(out, pointer, dtype code, layout code) of a flow result: ``dtype`` / ``layout`` None = the input's."""
    dtype = _NAMES[fl.dtype] if dtype is None else dtype
    layout = in_layout if layout is None else layout
    if layout not in D._LAYOUTS:
        raise ValueError(f"layout {layout!r}: 'planar' ([R][3][h][w] = u, v, m) or 'interleaved' ([R][h][w][2] = (u, v))")
    out, ptr, code = D._shaped_target(out, dtype, D._OUT_DTYPES, lead + _rec_shape(layout, h, w), "flow records")
    return out, ptr, code, D._LAYOUTS[layout]


def _min_size(h, w):
    if h < 2 or w < 2:
        raise ValueError(f"a {h} x {w} (h x w) flow: the bilinear cell needs h, w >= 2")


def compose(flow, *, in_layout="planar", last_only=False, dtype=None, layout=None, out=None, stream=None):
    """The pair flows ``flow`` (record k: frame k -> frame k + 1; ``in_layout`` is their layout)
    chained from frame 0 (foto_flow_compose_dev): C_0 = F_0, C_k(p) = C_{k-1}(p) + S(F_k; p +
    C_{k-1}(p)) with the clamped bilinear sample S.  Returns the records C_0 .. C_{K-1}, shaped like
    the input, or with ``last_only`` the one record C_{K-1} (no record axis): the flow frame 0 ->
    frame K.  ``dtype`` / ``layout`` of the result default to the input's.  A planar result of a
    planar input carries the composed gain, 1 + M_k = (1 + M_{k-1}) (1 + S(m_k; .)); of an
    interleaved input, m = 0."""
    host = isinstance(flow, np.ndarray)
    if host:
        if out is not None:
            raise ValueError("out: a device array for device input; numpy input returns a numpy array")
        flow = _host_flow(flow)
    fl, R, h, w, batched = flow_arg(flow, in_layout)
    _min_size(h, w)
    lead = () if last_only or not batched else (R,)
    out, ptr, code, lcode = _flow_target(fl, in_layout, dtype, layout, lead, h, w, out)
    check(lib().foto_flow_compose_dev(ctypes.byref(fl), w, h, 1 if last_only else 0, ctypes.c_void_p(ptr), code, lcode,
                                      ctypes.c_void_p(D.stream_handle(stream, flow))))
    return out.to_numpy() if host else out


def invert(flow, *, in_layout="planar", iters=INV_ITERS_DEFAULT, dtype=None, layout=None, out=None, stream=None):
    """The backward flow B of every record F of ``flow``, F(p + B) + B = 0 (foto_flow_invert_dev):
    B = 0, then B <- -S(F; p + B) exactly ``iters`` times (1 .. INV_ITERS_MAX), no convergence test
    -- BBSolver.maps' rule.  It converges where F is a contraction.  Shaped like the input; the m
    plane of a planar result is 0."""
    host = isinstance(flow, np.ndarray)
    if host:
        if out is not None:
            raise ValueError("out: a device array for device input; numpy input returns a numpy array")
        flow = _host_flow(flow)
    fl, R, h, w, batched = flow_arg(flow, in_layout)
    _min_size(h, w)
    iters = int(iters)
    if not 1 <= iters <= INV_ITERS_MAX:
        raise ValueError(f"iters = {iters} is outside [1, {INV_ITERS_MAX}]")
    out, ptr, code, lcode = _flow_target(fl, in_layout, dtype, layout, (R,) if batched else (), h, w, out)
    check(lib().foto_flow_invert_dev(ctypes.byref(fl), w, h, iters, ctypes.c_void_p(ptr), code, lcode,
                                     ctypes.c_void_p(D.stream_handle(stream, flow))))
    return out.to_numpy() if host else out


def consistency(fwd, bwd, *, layout="planar", bwd_layout=None, alpha1=ALPHA1, alpha2=ALPHA2, err=False, out=None,
                table_out=None, stream=None):
    """The forward-backward check of ``fwd`` against ``bwd`` (as many records, or one for all;
    ``bwd_layout`` None: ``layout``) by foto_flow_consistency_dev: q = p + F(p), Bq = S(B; q), and per
    pixel the first class that applies of 3 not finite, 2 q outside the frame, 1 |F + Bq|^2 >
    alpha1 (|F|^2 + |Bq|^2) + alpha2, 0 consistent.  Returns (valid, table) or, with ``err``
    ("float32" / "float64" / True = float64, or a device array), (valid, table, err): ``valid``
    uint8 ([R,] h, w), 1 = consistent -- score_flow's ``mask`` -- ``table`` float64 ([R,] 4), the
    class counts in CLASSES' order, ``err`` = |F + Bq|, NaN where not finite.  ``out`` / ``table_out``:
    device arrays for valid and table."""
    host = isinstance(fwd, np.ndarray)
    if host != isinstance(bwd, np.ndarray):
        raise TypeError("consistency: fwd and bwd are both numpy arrays or both device arrays")
    if host:
        if out is not None or table_out is not None or not isinstance(err, (bool, str, type, np.dtype)):
            raise ValueError("out / table_out / err arrays: device arrays for device input")
        fwd, bwd = _host_flow(fwd), _host_flow(bwd)
    for name, a in (("alpha1", alpha1), ("alpha2", alpha2)):
        if not (np.isfinite(a) and a >= 0):
            raise ValueError(f"{name} = {a!r} must be finite and >= 0")
    f, R, h, w, batched = flow_arg(fwd, layout)
    b, Rb, hb, wb, _ = flow_arg(bwd, layout if bwd_layout is None else bwd_layout)
    _min_size(h, w)
    if (hb, wb) != (h, w):
        raise ValueError(f"bwd is {hb} x {wb} (h x w), fwd {h} x {w}")
    if Rb not in (1, R):
        raise ValueError(f"bwd has {Rb} records: 1 (for every record) or fwd's {R}")
    lead = (R,) if batched else ()
    valid, vptr, _ = D._shaped_target(out, "uint8", {"uint8": _lib.FOTO_U8}, lead + (h, w), "masks")
    table, tptr, _ = D._shaped_target(table_out, "float64", _F64, lead + (4,), "class counts")
    eobj, eptr, ecode = None, None, _lib.FOTO_F64
    if err is not False and err is not None:
        if isinstance(err, (bool, str, type, np.dtype)):
            eobj, eptr, ecode = D._shaped_target(None, "float64" if err is True else err, D._OUT_DTYPES, lead + (h, w),
                                                 "errors")
        else:
            ts = D.device_interface(err)[1]
            eobj, eptr, ecode = D._shaped_target(err, np.dtype(ts).name, D._OUT_DTYPES, lead + (h, w), "errors")
    check(lib().foto_flow_consistency_dev(ctypes.byref(f), ctypes.byref(b), w, h, float(alpha1), float(alpha2),
                                          ctypes.c_void_p(vptr), ctypes.c_void_p(eptr), ecode, ctypes.c_void_p(tptr),
                                          ctypes.c_void_p(D.stream_handle(stream, fwd, bwd))))
    res = (valid, table) + ((eobj,) if eobj is not None else ())
    return tuple(x.to_numpy() for x in res) if host else res
