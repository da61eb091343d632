"""Frame preparation on the device (include/foto.h, "frame preparation"): the stages before a solve
-- what utils.openGrayscaleImage, run.sh:18-70 and the bin/ tools do to a frame on the host -- on
frames that already live in device memory, and the way back for a flow solved at a reduced size.

``gray``            PIL's convert('L') of an RGB / RGBA frame
``resize``          PIL's Image.resize, bit for bit (box, bilinear, bicubic, lanczos), on a plan
                    that is made once per (size, size, filter) and reused (``ResizePlan``)
``resize_flow``     a flow buffer through the same plan, u and v scaled with the size
``normalize_pair``  bin/normalize_image.py: each frame over its sum, both over the larger maximum
``illuminate``      bin/create_lum_dataset.py's rectangles and discs (``lum_shapes`` draws them)
``difference``      bin/data_diff.py: the rescaled frame difference
``resize_coeffs``   the coefficient tables of one axis, on the host (no GPU)

Frames are device arrays (``DeviceArray``, torch tensors, anything with
``__cuda_array_interface__``): (h, w), (h, w, C) or, with ``channels_last=False``, (C, h, w); uint8,
float32 or float64; any strides.  Results are new DeviceArrays (or ``out``); nothing leaves HBM.
"""
import ctypes
import random
import sys

import numpy as np

from . import _lib
from . import device as D
from ._lib import check, lib
from .render import flow_arg, source_arg

TILE_X = _lib.FOTO_PREP_TILE_X
MAX_SHAPES = _lib.FOTO_PREP_MAX_SHAPES
FILTERS = {"box": _lib.FOTO_FILTER_BOX, "bilinear": _lib.FOTO_FILTER_BILINEAR, "bicubic": _lib.FOTO_FILTER_BICUBIC,
           "lanczos": _lib.FOTO_FILTER_LANCZOS}
ROUTES = {"auto": _lib.FOTO_RESIZE_ROUTE_AUTO, "lds": _lib.FOTO_RESIZE_ROUTE_LDS,
          "direct": _lib.FOTO_RESIZE_ROUTE_DIRECT}
_NAMES = {_lib.FOTO_U8: "uint8", _lib.FOTO_F32: "float32", _lib.FOTO_F64: "float64"}


def _filter(name):
    if name not in FILTERS:
        raise ValueError(f"filter {name!r}: one of {', '.join(FILTERS)}")
    return FILTERS[name]


def _route(name):
    if name not in ROUTES:
        raise ValueError(f"route {name!r}: one of {', '.join(ROUTES)}")
    return ROUTES[name]


def _size(size, w, h):
    """(ow, oh) of ``size``: a pair (ow, oh), "WxH", or a scale factor S (PIL's rounding of run.py:
    max(1, round(w S)))."""
    if isinstance(size, str):
        if "x" in size.lower():
            a, _, b = size.lower().partition("x")
            size = (int(a), int(b))
        else:
            size = float(size)
    if isinstance(size, (int, float, np.integer, np.floating)) and not isinstance(size, bool):
        s = float(size)
        if not (s > 0 and np.isfinite(s)):
            raise ValueError(f"size {size!r}: a scale factor must be finite and > 0")
        size = (max(1, round(w * s)), max(1, round(h * s)))
    try:
        ow, oh = (int(x) for x in size)
    except (TypeError, ValueError):
        raise ValueError(f"size {size!r}: (ow, oh), 'WxH' or a scale factor") from None
    if ow < 1 or oh < 1:
        raise ValueError(f"size {(ow, oh)}: both must be >= 1")
    return ow, oh


def resize_coeffs(n_in, n_out, filter="lanczos"):
    """Pillow's precompute_coeffs for one axis, computed by the library's host code (no GPU):
    (ksize, bounds int32 (n_out, 2) = (first tap, count), kk float64 (n_out, ksize), the 22-bit
    fixed-point table int32 (n_out, ksize))."""
    f = _filter(filter)
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resize_coeffs: n_in = {n_in}, n_out = {n_out}: both must be >= 1")
    ks = ctypes.c_int(0)
    check(lib().foto_resize_coeffs(n_in, n_out, f, ctypes.byref(ks), None, None, None, 0))
    bounds = np.zeros((n_out, 2), np.int32)
    kk = np.zeros((n_out, ks.value), np.float64)
    ki = np.zeros((n_out, ks.value), np.int32)
    check(lib().foto_resize_coeffs(n_in, n_out, f, ctypes.byref(ks), bounds.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                   _lib.dptr(kk), ki.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), kk.size))
    return ks.value, bounds, kk, ki


# -------------------------------------------------------------------- grey

def gray(src, *, channels_last=True, out=None, stream=None):
    """PIL's convert('L') of an RGB / RGBA device frame (foto_prep_gray_dev): (h, w) of the frame's
    dtype; uint8 is PIL's (19595 R + 38470 G + 7471 B + 0x8000) >> 16, floats use the same weights
    over 65536 in float64.  Alpha is ignored."""
    im, C, sc, has_c = source_arg(src, channels_last)
    if not has_c or C not in (3, 4):
        raise ValueError(f"gray: a colour frame has 3 (RGB) or 4 (RGBA) channels, got {C if has_c else 'no channel axis'}")
    h, w = im.shape
    out, ptr, _ = D._shaped_target(out, _NAMES[im.dtype], D._FRAME_DTYPES, (h, w), "grey frames")
    check(lib().foto_prep_gray_dev(ctypes.byref(im), C, sc, w, h, ctypes.c_void_p(ptr),
                                   ctypes.c_void_p(D.stream_handle(stream, src))))
    return out


# -------------------------------------------------------------------- resize

class ResizePlan:
    """foto_resize_plan: the coefficient tables of (w, h) -> (ow, oh) for one filter, uploaded once;
    every frame of a video, and the flow on the way back, reuses it."""

    def __init__(self, w, h, ow, oh, filter="lanczos"):
        self.w, self.h, self.ow, self.oh, self.filter = int(w), int(h), int(ow), int(oh), filter
        f = _filter(filter)
        if min(self.w, self.h, self.ow, self.oh) < 1:
            raise ValueError(f"ResizePlan: sizes {(self.w, self.h)} -> {(self.ow, self.oh)}: all must be >= 1")
        p = ctypes.c_void_p()
        check(lib().foto_resize_plan_create(self.w, self.h, self.ow, self.oh, f, ctypes.byref(p)))
        self._p = p

    def info(self):
        """{ksize_x, ksize_y, span_x}: taps per output of each axis and the widest input span of a
        horizontal tile (the LDS route holds 512)."""
        v = (ctypes.c_int * 8)()
        check(lib().foto_resize_plan_info(self._p, v))
        return {"ksize_x": v[5], "ksize_y": v[6], "span_x": v[7]}

    def resize(self, src, *, channels_last=True, route="auto", out=None, stream=None):
        """The frame resized: (oh, ow) or (oh, ow, C) of the frame's dtype; a (C, h, w) frame
        (``channels_last=False``) gives (C, oh, ow).  All channels go through in one call."""
        rt = _route(route)
        im, C, sc, has_c = source_arg(src, channels_last)
        if im.shape != (self.h, self.w):
            raise ValueError(f"resize: the frame is {im.shape[0]} x {im.shape[1]} (h x w), the plan {self.h} x {self.w}")
        name = _NAMES[im.dtype]
        st = ctypes.c_void_p(D.stream_handle(stream, src))
        planar = has_c and not channels_last
        shape = (C, self.oh, self.ow) if planar else (self.oh, self.ow) + ((C,) if has_c else ())
        out, ptr, _ = D._shaped_target(out, name, D._FRAME_DTYPES, shape, "resized frames")
        check(lib().foto_resize_dev(self._p, ctypes.byref(im), C, sc, ctypes.c_void_p(ptr), 1 if planar else 0, rt, st))
        return out

    def resize_flow(self, flow, *, layout="planar", route="auto", out=None, stream=None):
        """Every record and plane of a flow buffer through the float path of the plan; u is scaled
        by ow / w and v by oh / h before the final rounding, m is not.  Same dtype and layout."""
        rt = _route(route)
        fl, R, h, w, batched = flow_arg(flow, layout)
        if (h, w) != (self.h, self.w):
            raise ValueError(f"resize_flow: the flow is {h} x {w} (h x w), the plan {self.h} x {self.w}")
        rec = (3, self.oh, self.ow) if layout == "planar" else (self.oh, self.ow, 2)
        name = _NAMES[fl.dtype]
        out, ptr, _ = D._shaped_target(out, name, D._OUT_DTYPES, ((R,) if batched else ()) + rec, "flow records")
        check(lib().foto_flow_resize_dev(self._p, ctypes.byref(fl), ctypes.c_void_p(ptr), rt,
                                         ctypes.c_void_p(D.stream_handle(stream, flow))))
        return out

    def close(self):
        if getattr(self, "_p", None):
            lib().foto_resize_plan_destroy(self._p)
            self._p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


_plans = {}
PLAN_CACHE_MAX = 8


def cached_plan(w, h, ow, oh, filter="lanczos"):
    """The ResizePlan of this (sizes, filter), made on first use and kept (the last PLAN_CACHE_MAX)."""
    key = (int(w), int(h), int(ow), int(oh), filter)
    p = _plans.pop(key, None)
    if p is None:
        p = ResizePlan(*key)
        while len(_plans) >= PLAN_CACHE_MAX:
            _plans.pop(next(iter(_plans))).close()
    _plans[key] = p
    return p


def resize(src, size, filter="lanczos", *, channels_last=True, route="auto", out=None, stream=None):
    """PIL's ``Image.resize(size, filter)`` of a device frame, bit for bit for uint8 ('L') and
    float32 ('F'); float64 likewise in double.  ``size``: (ow, oh), "WxH" or a scale factor."""
    _filter(filter)
    im = source_arg(src, channels_last)[0]
    h, w = im.shape
    ow, oh = _size(size, w, h)
    return cached_plan(w, h, ow, oh, filter).resize(src, channels_last=channels_last, route=route, out=out, stream=stream)


def resize_flow(flow, size, filter="bilinear", *, layout="planar", route="auto", out=None, stream=None):
    """A flow buffer resized to ``size`` = (ow, oh) (or "WxH", or a scale factor), its u and v
    scaled with it: the flow of a half-resolution solve at the size of the caller's frames."""
    _filter(filter)
    _, _, h, w, _ = flow_arg(flow, layout)
    ow, oh = _size(size, w, h)
    return cached_plan(w, h, ow, oh, filter).resize_flow(flow, layout=layout, route=route, out=out, stream=stream)


# -------------------------------------------------------------------- pointwise stages

def _out_dtype(dtype):
    return D._dtype_name(dtype, D._FRAME_DTYPES, "prepared frames")


def normalize_pair(f0, f1, *, dtype="uint8", out0=None, out1=None, stream=None):
    """bin/normalize_image.py on a device pair (foto_prep_normalize_pair_dev): each frame over its
    fixed-order sum, both over max(max0 / S0, max1 / S1).  ``dtype`` "uint8" is the tool's
    truncating np.uint8(255 clip(x, 0, 1)), "float32" / "float64" the values.  Returns (out0,
    out1, {"S0", "S1", "max0", "max1"}); the call waits for the statistics."""
    a, b = D._pair(f0, f1)
    dtype = _out_dtype(dtype)
    h, w = a.shape
    out0, p0, code = D._shaped_target(out0, dtype, D._FRAME_DTYPES, (h, w), "prepared frames")
    out1, p1, _ = D._shaped_target(out1, dtype, D._FRAME_DTYPES, (h, w), "prepared frames")
    st = np.zeros(4, np.float64)
    check(lib().foto_prep_normalize_pair_dev(ctypes.byref(a), ctypes.byref(b), w, h, ctypes.c_void_p(p0),
                                             ctypes.c_void_p(p1), code, _lib.dptr(st),
                                             ctypes.c_void_p(D.stream_handle(stream, f0, f1))))
    return out0, out1, dict(zip(("S0", "S1", "max0", "max1"), (float(x) for x in st)))


def lum_shapes(w, h, seed):
    """The four shapes bin/create_lum_dataset.py draws for ``seed``: two rectangles, two discs, with
    Python's ``random`` in the reference's order (bin/create_lum_dataset.py:23-38, 48-56).
    ("rect", L_x, L_y, r_x, r_y, v) and ("circle", R, c_x, c_y, v)."""
    random.seed(seed)
    shapes = []
    for _ in range(2):
        L_x = random.randint(10, w - 1)
        L_y = random.randint(10, h - 1)
        r_x = random.randint(int(L_x / 2), int(w - L_x / 2))
        r_y = random.randint(int(L_y / 2), int(h - L_y / 2))
        shapes.append(("rect", L_x, L_y, r_x, r_y, random.uniform(-0.25, 0.25)))
    for _ in range(2):
        R = random.randint(10, min(w, h)) / 2
        c_x = random.randint(int(R), int(w - R))
        c_y = random.randint(int(R), int(h - R))
        shapes.append(("circle", R, c_x, c_y, random.uniform(-0.25, 0.25)))
    return shapes


def shape_array(shapes):
    """The foto_lum_shape array of a list of ("rect", L_x, L_y, r_x, r_y, v) / ("circle", R, c_x,
    c_y, v) tuples; ValueError for a wrong kind, length, count or a non-finite number."""
    shapes = list(shapes)
    if len(shapes) > MAX_SHAPES:
        raise ValueError(f"illuminate: {len(shapes)} shapes; at most {MAX_SHAPES}")
    arr = (_lib.LumShape * max(len(shapes), 1))()
    for k, s in enumerate(shapes):
        kind, n = {"rect": (_lib.FOTO_LUM_RECT, 4), "circle": (_lib.FOTO_LUM_CIRCLE, 3)}.get(s[0], (None, 0))
        if kind is None or len(s) != n + 2:
            raise ValueError(f"illuminate: shape {k} = {s!r}: ('rect', L_x, L_y, r_x, r_y, v) or ('circle', R, c_x, c_y, v)")
        vals = [float(x) for x in s[1:]]
        if not all(np.isfinite(vals)):
            raise ValueError(f"illuminate: shape {k} = {s!r} has a non-finite number")
        arr[k].kind = kind
        for j in range(n):
            arr[k].p[j] = vals[j]
        arr[k].v = vals[-1]
    return arr, len(shapes)


def illuminate(src, shapes, *, dtype="uint8", out=None, stream=None):
    """bin/create_lum_dataset.py's additions on a grey device frame (foto_prep_illuminate_dev):
    ``shapes`` (``lum_shapes``' tuples, at most MAX_SHAPES) are added per pixel in list order."""
    im = D.as_image(src)
    dtype = _out_dtype(dtype)
    arr, n = shape_array(shapes)
    h, w = im.shape
    out, ptr, code = D._shaped_target(out, dtype, D._FRAME_DTYPES, (h, w), "prepared frames")
    check(lib().foto_prep_illuminate_dev(ctypes.byref(im), w, h, arr, n, ctypes.c_void_p(ptr), code,
                                         ctypes.c_void_p(D.stream_handle(stream, src))))
    return out


def difference(f0, f1, *, dtype="uint8", out=None, stream=None, return_minmax=False):
    """bin/data_diff.py on a device pair (foto_prep_diff_dev): (d - min d) / (max d - min d), d =
    f1 - f0.  A constant difference is 0 / 0: 0 as uint8, NaN as float."""
    a, b = D._pair(f0, f1)
    dtype = _out_dtype(dtype)
    h, w = a.shape
    out, ptr, code = D._shaped_target(out, dtype, D._FRAME_DTYPES, (h, w), "prepared frames")
    mm = np.zeros(2, np.float64)
    check(lib().foto_prep_diff_dev(ctypes.byref(a), ctypes.byref(b), w, h, ctypes.c_void_p(ptr), code,
                                   _lib.dptr(mm) if return_minmax else None,
                                   ctypes.c_void_p(D.stream_handle(stream, f0, f1))))
    return (out, (float(mm[0]), float(mm[1]))) if return_minmax else out
