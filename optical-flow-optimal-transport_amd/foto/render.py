"""Rendering on the device (include/foto.h, "rendering"): what main.py:107-146 and run.sh:104,115
do with a flow, on the flow buffers ``flow_device``, ``flow_path_device`` and
``gn.Plan.solve_device`` leave in device memory -- one record or many, nothing leaves HBM.

``reconstruct``   the first frame warped by the flow, clipped to [0, 1] (main.py:109-110,142)
``luminosity``    the 8-bit luminosity map of m (main.py:146)
``flow_color``    the Middlebury colour code (run.sh:104,115; bin/color_flow.py) in float64
``reconstruct_host`` / ``flow_color_host``  the same on numpy arrays (upload, render, download)

A flow is a C-contiguous float32 / float64 device array: "planar" (3, h, w) or (R, 3, h, w) =
u, v, m, or "interleaved" (h, w, 2) or (R, h, w, 2) = (u, v).  The result mirrors the arguments:
a leading record axis when the flow has one, a trailing channel axis when the frame has one.
"""
import ctypes

import numpy as np

from . import _lib
from . import device as D
from ._lib import check, lib

_U8 = {"uint8": _lib.FOTO_U8}


def _contiguous(shape, strides, item, what):
    if not D.c_contiguous(shape, strides, item):
        raise ValueError(f"{what} must be C-contiguous")


def flow_arg(flow, layout="planar"):
    """(_lib.Flow, records, h, w, has_record_axis) of a device flow array; ValueError for a wrong
    shape, dtype or a non-contiguous array, before the library is touched."""
    if layout not in D._LAYOUTS:
        raise ValueError(f"layout {layout!r}: 'planar' ([R][3][h][w] = u, v, m) or 'interleaved' ([R][h][w][2] = (u, v))")
    ptr, typestr, shape, strides, _ = D.device_interface(flow)
    if typestr not in ("<f4", "<f8"):
        raise ValueError(f"flow: typestr {typestr!r}; a flow is float32 or float64")
    if len(shape) not in (3, 4):
        raise ValueError(f"flow of shape {shape}: (3, h, w) / (R, 3, h, w) planar or (h, w, 2) / (R, h, w, 2) interleaved")
    batched = len(shape) == 4
    rec = shape[1:] if batched else shape
    R = shape[0] if batched else 1
    if layout == "planar":
        ok, (h, w) = rec[0] == 3, rec[1:]
    else:
        ok, (h, w) = rec[2] == 2, rec[:2]
    if not ok or R < 1 or h < 1 or w < 1:
        raise ValueError(f"flow of shape {shape} is not a {layout} flow: " +
                         ("(3, h, w) or (R, 3, h, w)" if layout == "planar" else "(h, w, 2) or (R, h, w, 2)"))
    _contiguous(shape, strides, np.dtype(typestr).itemsize, "flow")
    fl = _lib.Flow()
    fl.data, fl.dtype, fl.layout, fl.records = ptr, D._DTYPES[typestr][0], D._LAYOUTS[layout], int(R)
    fl._keep = flow
    return fl, int(R), int(h), int(w), batched


def source_arg(src, channels_last=True, divisor=None):
    """(_lib.Image of channel 0, channels, stride_c in elements, has_channel_axis) of a device
    frame: 2-D (h, w), or 3-D (h, w, C) (``channels_last``) / (C, h, w); uint8 / float32 /
    float64, any strides that are multiples of the item size."""
    ptr, typestr, shape, strides, _ = D.device_interface(src)
    if typestr not in D._DTYPES:
        raise ValueError(f"src: typestr {typestr!r}; frames are uint8 ('|u1'), float32 ('<f4') or float64 ('<f8')")
    if len(shape) not in (2, 3):
        raise ValueError(f"src of shape {shape}: a frame is (h, w), (h, w, C) or (C, h, w)")
    code, npdt = D._DTYPES[typestr]
    item = np.dtype(npdt).itemsize
    if strides is None:
        strides = D.packed_strides(shape, item)
    strides = tuple(int(s) for s in strides)
    if any(s % item for s in strides):
        raise ValueError(f"src: byte strides {strides} are not multiples of the {item}-byte item size")
    has_c = len(shape) == 3
    if not has_c:
        (h, w), (sy, sx), C, sc = shape, strides, 1, item
    elif channels_last:
        (h, w, C), (sy, sx, sc) = shape, strides
    else:
        (C, h, w), (sc, sy, sx) = shape, strides
    if C < 1:
        raise ValueError(f"src of shape {shape} has no channel")
    im = D.make_image(ptr, code, sy // item, sx // item, divisor, (h, w), src)
    return im, int(C), (sc // item if C > 1 else 1), has_c


def reconstruct(src, flow, *, layout="planar", use_m=True, dtype="uint8", out=None, stream=None, channels_last=True,
                divisor=None):
    """clip(apply_opticalflow(src / divisor, u, v, w, h, m), 0, 1) of every record of ``flow`` and
    every channel of ``src`` in one launch (foto_render_warp_dev): a DeviceArray (or ``out``) of
    shape ([R,] h, w [, C]) and ``dtype`` -- "uint8" is the reference's truncating
    np.uint8(255 * x) (main.py:142), "float32" / "float64" the clipped values.  ``use_m`` scales
    the frame by 1 + m and needs the planar layout; pass ``use_m=False`` for an interleaved flow.
    ``divisor`` defaults to 255 for a uint8 frame and 1 otherwise."""
    fl, R, h, w, batched = flow_arg(flow, layout)
    im, C, sc, has_c = source_arg(src, channels_last, divisor)
    if im.shape != (h, w):
        raise ValueError(f"src is {im.shape[0]} x {im.shape[1]} (h x w), the flow {h} x {w}")
    if use_m and layout != "planar":
        raise ValueError("use_m needs the planar layout: an interleaved flow carries no m (pass use_m=False)")
    shape = ((R,) if batched else ()) + (h, w) + ((C,) if has_c else ())
    out, ptr, code = D._shaped_target(out, dtype, D._FRAME_DTYPES, shape, "reconstructions")
    st = D.stream_handle(stream, src, flow)
    check(lib().foto_render_warp_dev(ctypes.byref(im), C, sc, ctypes.byref(fl), 1 if use_m else 0, w, h,
                                     ctypes.c_void_p(ptr), code, ctypes.c_void_p(st)))
    return out


def luminosity(flow, *, out=None, stream=None):
    """np.uint8(255 * clip((m + 1) / 2, 0, 1)) (main.py:146) of a planar flow
    (foto_render_lum_dev): a uint8 DeviceArray (or ``out``) of shape ([R,] h, w)."""
    fl, R, h, w, batched = flow_arg(flow, "planar")
    out, ptr, _ = D._shaped_target(out, "uint8", _U8, ((R,) if batched else ()) + (h, w), "luminosity maps")
    check(lib().foto_render_lum_dev(ctypes.byref(fl), w, h, ctypes.c_void_p(ptr),
                                    ctypes.c_void_p(D.stream_handle(stream, flow))))
    return out


def flow_color(flow, *, layout="planar", maxmotion=0.0, out=None, maxrad=None, stream=None):
    """The Middlebury colour code of every record (foto_render_color_dev): a uint8 RGB DeviceArray
    (or ``out``) of shape ([R,] h, w, 3).  ``maxmotion`` > 0 replaces the per-record maximum flow
    magnitude as the radius of full saturation.  ``maxrad``: a float64 device array of R values
    that receives the radius actually used (no host synchronisation either way)."""
    fl, R, h, w, batched = flow_arg(flow, layout)
    mr = None
    if maxrad is not None:
        mptr, typestr, mshape, mstrides, _ = D.device_interface(maxrad)
        if typestr != "<f8" or int(np.prod(mshape, dtype=np.int64)) != R:
            raise ValueError(f"maxrad: expected {R} float64 values on the device, got {typestr} of shape {mshape}")
        _contiguous(mshape, mstrides, 8, "maxrad")
        mr = ctypes.c_void_p(mptr)
    out, ptr, _ = D._shaped_target(out, "uint8", _U8, ((R,) if batched else ()) + (h, w, 3), "colour codes")
    check(lib().foto_render_color_dev(ctypes.byref(fl), w, h, float(maxmotion), ctypes.c_void_p(ptr), mr,
                                      ctypes.c_void_p(D.stream_handle(stream, flow))))
    return out


# -------------------------------------------------------------------- host conveniences

def _host_flow(flow):
    a = np.asarray(flow)
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    return D.DeviceArray.from_numpy(a)


def reconstruct_host(src, flow, **kw):
    """reconstruct() on numpy arrays: ``src`` uint8 / float32 / float64 (other dtypes go through
    float64), ``flow`` float32 / float64; uploaded, rendered, downloaded."""
    s = np.asarray(src)
    if s.dtype not in (np.uint8, np.float32, np.float64):
        s = s.astype(np.float64)
    return reconstruct(D.DeviceArray.from_numpy(s), _host_flow(flow), **kw).to_numpy()


def flow_color_host(flow, *, return_maxrad=False, **kw):
    """flow_color() on a numpy flow; with ``return_maxrad`` also the radii used, (image, maxrad)."""
    d = _host_flow(flow)
    if not return_maxrad:
        return flow_color(d, **kw).to_numpy()
    R = d.shape[0] if d.ndim == 4 else 1
    mr = D.DeviceArray((R,), np.float64)
    img = flow_color(d, maxrad=mr, **kw).to_numpy()
    return img, mr.to_numpy()
