"""GPU evaluation helpers: the backward warp and the flow / intensity
error metrics of the reference's utils.py, through libfoto's C ABI.

warp            utils.apply_opticalflow (utils.py:186-248)  bit-identical
flow_errors     utils.EE + utils.AE     (utils.py:294-338)  up to summation order
intensity_error utils.IE                (utils.py:340-354)  up to summation order
"""
import ctypes

import numpy as np

from ._lib import check, dptr, f64, lib


def warp(f1, u, v, w, h, m=None):
    """(1 + m) f1 (or f1 if m is None) warped backwards by (u, v)."""
    n = w * h
    f = f64(f1, n, "f1")
    uu, vv = f64(u, n, "u"), f64(v, n, "v")
    mm = None if m is None else f64(np.broadcast_to(np.asarray(m, dtype=np.float64), (n,)), n, "m")
    out = np.empty(n)
    check(lib().foto_warp(dptr(f), dptr(uu), dptr(vv), dptr(mm) if mm is not None else None, w, h, dptr(out)))
    return out


def flow_errors(u, v, uGT, vGT, w, h):
    """(AEE, SDEE, AAE, SDAE): endpoint error <= 50 and non-NaN angular error (radians)."""
    n = w * h
    a = [f64(np.asarray(x, dtype=np.float64)[:n], n, name) for x, name in ((u, "u"), (v, "v"), (uGT, "uGT"), (vGT, "vGT"))]
    out = np.empty(4)
    check(lib().foto_flow_errors(*(dptr(x) for x in a), w, h, dptr(out)))
    return tuple(float(x) for x in out)


def intensity_error(I, IGT, w, h):
    """RMS of 255 I - 255 IGT."""
    n = w * h
    a, b = f64(I, n, "I"), f64(IGT, n, "IGT")
    out = np.empty(1)
    check(lib().foto_intensity_error(dptr(a), dptr(b), w, h, dptr(out)))
    return float(out[0])


# ------------------------------------------------------------------ device buffers
# The same three calls on contiguous float64 device arrays (foto.device.DeviceArray, torch ROCm
# tensors, ...): the same kernels and reduction order, without the uploads.

def _dev_f64(x, n, name):
    from . import device as D
    ptr, typestr, shape, strides, _ = D.device_interface(x)
    size = int(np.prod(shape, dtype=np.int64))
    if typestr != "<f8" or size != n:
        raise ValueError(f"{name}: expected {n} float64 values on the device, got {size} of {typestr}")
    if not D.c_contiguous(shape, strides, 8):
        raise ValueError(f"{name}: must be C-contiguous")
    return ctypes.c_void_p(ptr)


def warp_device(f1, u, v, w, h, m=None, out=None, stream=None):
    """warp() on device arrays; returns the DeviceArray (or ``out``) of h x w float64."""
    from . import device as D
    n = w * h
    if out is None:
        out = D.DeviceArray((h, w), np.float64)
    st = D.stream_handle(stream, f1, u, v)
    check(lib().foto_warp_dev(_dev_f64(f1, n, "f1"), _dev_f64(u, n, "u"), _dev_f64(v, n, "v"),
                              _dev_f64(m, n, "m") if m is not None else None, w, h, _dev_f64(out, n, "out"),
                              ctypes.c_void_p(st)))
    return out


def flow_errors_device(u, v, uGT, vGT, w, h, stream=None):
    """flow_errors() on device arrays (host scalars back)."""
    from . import device as D
    n = w * h
    out = np.empty(4)
    st = D.stream_handle(stream, u, v, uGT, vGT)
    check(lib().foto_flow_errors_dev(_dev_f64(u, n, "u"), _dev_f64(v, n, "v"), _dev_f64(uGT, n, "uGT"),
                                     _dev_f64(vGT, n, "vGT"), w, h, dptr(out), ctypes.c_void_p(st)))
    return tuple(float(x) for x in out)


def intensity_error_device(I, IGT, w, h, stream=None):
    """intensity_error() on device arrays (a host scalar back)."""
    from . import device as D
    n = w * h
    out = np.empty(1)
    st = D.stream_handle(stream, I, IGT)
    check(lib().foto_intensity_error_dev(_dev_f64(I, n, "I"), _dev_f64(IGT, n, "IGT"), w, h, dptr(out),
                                         ctypes.c_void_p(st)))
    return float(out[0])
