"""Rendering entries (include/foto.h, "rendering"), the parts that need no GPU: foto_flow_check,
every argument error the entries report before they touch a device (through the C ABI, on pointers
that are never dereferenced), the ctypes structure against the C one, and the ValueErrors of
foto.render for shape, dtype and contiguity, raised before the library is called."""
import ctypes
import math

import pytest

from conftest import PKG  # noqa: F401  (puts the package on sys.path)

from foto import _lib, render

W, H = 37, 29
ARG = _lib.FOTO_ERR_ARG
PTR = 0x7f0000010000   # a well-aligned address; argument errors return before anything reads it


def _flow(data=PTR, dtype=_lib.FOTO_F32, layout=0, records=3):
    fl = _lib.Flow()
    fl.data, fl.dtype, fl.layout, fl.records = data, dtype, layout, records
    return fl


def _img(data=PTR + 0x100000, dtype=_lib.FOTO_U8, sy=3 * W, sx=3, divisor=255.0):
    im = _lib.Image()
    im.data, im.dtype, im.stride_y, im.stride_x, im.divisor = data, dtype, sy, sx, divisor
    return im


OUT = PTR + 0x200000


# ------------------------------------------------------------------ foto_flow_check

@pytest.mark.parametrize("name,fl", [
    ("float32 planar", _flow()),
    ("float64 interleaved", _flow(dtype=_lib.FOTO_F64, layout=1)),
    ("one record", _flow(records=1)),
    ("float32 at a 4-byte address", _flow(data=PTR + 4)),
])
def test_flow_check_accepts(name, fl):
    assert _lib.lib().foto_flow_check(ctypes.byref(fl), W, H) == 0, (name, _lib.lib().foto_last_error())


FLOW_REJECTS = [
    ("null data", _flow(data=0)),
    ("dtype uint8", _flow(dtype=_lib.FOTO_U8)),
    ("dtype 3", _flow(dtype=3)),
    ("dtype -1", _flow(dtype=-1)),
    ("layout 2", _flow(layout=2)),
    ("layout -1", _flow(layout=-1)),
    ("records 0", _flow(records=0)),
    ("records -2", _flow(records=-2)),
    ("float32 at a 2-byte address", _flow(data=PTR + 2)),
    ("float64 at a 4-byte address", _flow(data=PTR + 4, dtype=_lib.FOTO_F64)),
]


@pytest.mark.parametrize("name,fl", FLOW_REJECTS)
def test_flow_check_rejects(name, fl):
    L = _lib.lib()
    assert L.foto_flow_check(ctypes.byref(fl), W, H) == ARG, name
    assert L.foto_last_error(), name
    # and every entry reports the same before it touches a device
    im = _img()
    assert L.foto_render_warp_dev(ctypes.byref(im), 3, 1, ctypes.byref(fl), 0, W, H, ctypes.c_void_p(OUT),
                                  _lib.FOTO_U8, None) == ARG, name
    assert L.foto_render_lum_dev(ctypes.byref(fl), W, H, ctypes.c_void_p(OUT), None) == ARG, name
    assert L.foto_render_color_dev(ctypes.byref(fl), W, H, 0.0, ctypes.c_void_p(OUT), None, None) == ARG, name


def test_flow_check_null_and_sizes():
    L = _lib.lib()
    assert L.foto_flow_check(None, W, H) == ARG
    assert L.foto_flow_check(ctypes.byref(_flow()), 0, H) == ARG
    assert L.foto_flow_check(ctypes.byref(_flow()), W, 0) == ARG
    assert L.foto_flow_check(ctypes.byref(_flow()), -3, H) == ARG


def test_flow_struct_layout():
    assert ctypes.sizeof(_lib.Flow) == 24   # (foto_render.hip asserts the same of foto_flow)
    assert (_lib.Flow.data.offset, _lib.Flow.dtype.offset, _lib.Flow.layout.offset, _lib.Flow.records.offset) == \
        (0, 8, 12, 16)


# ------------------------------------------------------------------ argument errors before any device call

def _warp(im=None, channels=3, stride_c=1, fl=None, use_m=1, w=W, h=H, out=OUT, out_dtype=_lib.FOTO_U8):
    im = ctypes.byref(im) if im is not None else None
    fl = ctypes.byref(fl) if fl is not None else None
    return _lib.lib().foto_render_warp_dev(im, channels, stride_c, fl, use_m, w, h, ctypes.c_void_p(out), out_dtype,
                                           None)


@pytest.mark.parametrize("name,kw", [
    ("null src", dict(im=None)),
    ("null flow", dict(fl=None)),
    ("null out", dict(out=0)),
    ("w 0", dict(w=0)),
    ("h 0", dict(h=0)),
    ("h < 0", dict(h=-1)),
    ("channels 0", dict(channels=0)),
    ("channels < 0", dict(channels=-3)),
    ("stride_c 0", dict(stride_c=0)),
    ("stride_c < 0", dict(stride_c=-1)),
    ("image: null data", dict(im=_img(data=0))),
    ("image: dtype 3", dict(im=_img(dtype=3))),
    ("image: stride_x 0", dict(im=_img(sx=0))),
    ("image: stride_y < 0", dict(im=_img(sy=-3 * W))),
    ("image: divisor 0", dict(im=_img(divisor=0.0))),
    ("image: divisor nan", dict(im=_img(divisor=math.nan))),
    ("image: rows overlap", dict(im=_img(sy=3 * W - 3))),
    ("image: float64 at an odd address", dict(im=_img(data=PTR + 1, dtype=_lib.FOTO_F64))),
    ("use_m 1 with layout 1", dict(fl=_flow(layout=1), use_m=1)),
    ("use_m 2", dict(use_m=2)),
    ("out_dtype -1", dict(out_dtype=-1)),
    ("out_dtype 3", dict(out_dtype=3)),
    ("float64 out at a 4-byte address", dict(out=OUT + 4, out_dtype=_lib.FOTO_F64)),
])
def test_warp_argument_errors(name, kw):
    args = dict(im=_img(), fl=_flow())
    args.update(kw)
    assert _warp(**args) == ARG, name
    assert _lib.lib().foto_last_error(), name


def test_lum_argument_errors():
    L = _lib.lib()
    out = ctypes.c_void_p(OUT)
    assert L.foto_render_lum_dev(None, W, H, out, None) == ARG
    assert L.foto_render_lum_dev(ctypes.byref(_flow()), W, H, None, None) == ARG
    assert L.foto_render_lum_dev(ctypes.byref(_flow()), 0, H, out, None) == ARG
    assert L.foto_render_lum_dev(ctypes.byref(_flow()), W, 0, out, None) == ARG
    assert L.foto_render_lum_dev(ctypes.byref(_flow(layout=1)), W, H, out, None) == ARG   # no m in layout 1


def test_color_argument_errors():
    L = _lib.lib()
    out = ctypes.c_void_p(OUT)
    fl = ctypes.byref(_flow(layout=1))
    assert L.foto_render_color_dev(None, W, H, 0.0, out, None, None) == ARG
    assert L.foto_render_color_dev(fl, W, H, 0.0, None, None, None) == ARG
    assert L.foto_render_color_dev(fl, 0, H, 0.0, out, None, None) == ARG
    assert L.foto_render_color_dev(fl, W, -1, 0.0, out, None, None) == ARG
    for bad in (math.nan, math.inf, -math.inf):
        assert L.foto_render_color_dev(fl, W, H, bad, out, None, None) == ARG, bad
    assert L.foto_render_color_dev(fl, W, H, 0.0, out, ctypes.c_void_p(OUT + 0x10004), None) == ARG   # misaligned maxrad


# ------------------------------------------------------------------ foto.render: ValueError before the library

class Fake:
    """An object exposing a hand-written __cuda_array_interface__."""

    def __init__(self, shape, typestr, strides=None, ptr=PTR):
        self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(ptr, False), version=3,
                                             strides=strides)


def test_flow_arg_shapes():
    fl, R, h, w, batched = render.flow_arg(Fake((3, H, W), "<f4"))
    assert (fl.data, fl.dtype, fl.layout, fl.records, R, h, w, batched) == (PTR, _lib.FOTO_F32, 0, 1, 1, H, W, False)
    fl, R, h, w, batched = render.flow_arg(Fake((5, 3, H, W), "<f8"))
    assert (fl.dtype, fl.layout, fl.records, h, w, batched) == (_lib.FOTO_F64, 0, 5, H, W, True)
    fl, R, h, w, batched = render.flow_arg(Fake((H, W, 2), "<f4"), "interleaved")
    assert (fl.layout, fl.records, h, w, batched) == (1, 1, H, W, False)
    fl, R, h, w, batched = render.flow_arg(Fake((5, H, W, 2), "<f4"), "interleaved")
    assert (fl.layout, fl.records, h, w, batched) == (1, 5, H, W, True)
    assert _lib.lib().foto_flow_check(ctypes.byref(fl), w, h) == 0
    # explicit strides that are the contiguous ones
    render.flow_arg(Fake((3, H, W), "<f4", strides=(H * W * 4, W * 4, 4)))


@pytest.mark.parametrize("name,flow,layout", [
    ("2-D", Fake((H, W), "<f4"), "planar"),
    ("5-D", Fake((1, 1, 3, H, W), "<f4"), "planar"),
    ("two planes", Fake((2, H, W), "<f4"), "planar"),
    ("interleaved shape as planar", Fake((H, W, 2), "<f4"), "planar"),
    ("planar shape as interleaved", Fake((3, H, W), "<f4"), "interleaved"),
    ("three components interleaved", Fake((4, H, W, 3), "<f4"), "interleaved"),
    ("no records", Fake((0, 3, H, W), "<f4"), "planar"),
    ("uint8", Fake((3, H, W), "|u1"), "planar"),
    ("float16", Fake((3, H, W), "<f2"), "planar"),
    ("row-padded", Fake((3, H, W), "<f4", strides=(H * (W + 3) * 4, (W + 3) * 4, 4)), "planar"),
    ("transposed", Fake((3, H, W), "<f4", strides=(H * W * 4, 4, H * 4)), "planar"),
    ("layout name", Fake((3, H, W), "<f4"), "flo"),
])
def test_flow_arg_rejects(name, flow, layout):
    with pytest.raises(ValueError):
        render.flow_arg(flow, layout)
    with pytest.raises(ValueError):
        render.flow_color(flow, layout=layout)
    if layout == "planar":
        with pytest.raises(ValueError):
            render.luminosity(flow)


def test_source_arg_strides():
    im, C, sc, has_c = render.source_arg(Fake((H, W, 3), "|u1"))                       # interleaved HWC
    assert (im.dtype, im.stride_y, im.stride_x, im.divisor, C, sc, has_c, im.shape) == \
        (_lib.FOTO_U8, 3 * W, 3, 255.0, 3, 1, True, (H, W))
    im, C, sc, has_c = render.source_arg(Fake((3, H, W), "<f4"), channels_last=False)   # planar CHW
    assert (im.dtype, im.stride_y, im.stride_x, im.divisor, C, sc) == (_lib.FOTO_F32, W, 1, 1.0, 3, H * W)
    im, C, sc, has_c = render.source_arg(Fake((H, W), "<f8", strides=((W + 5) * 8, 8)))  # row-padded grey
    assert (im.stride_y, im.stride_x, C, sc, has_c) == (W + 5, 1, 1, 1, False)
    im, C, sc, has_c = render.source_arg(Fake((H, W), "|u1", strides=(3 * W, 3)), divisor=1.0)   # one channel of HWC
    assert (im.stride_y, im.stride_x, im.divisor, C) == (3 * W, 3, 1.0, 1)
    for bad in (Fake((W,), "|u1"), Fake((1, 3, H, W), "|u1"), Fake((H, W, 3), "<i4"), Fake((H, W, 3), "<f2"),
                Fake((H, W), "<f8", strides=(W * 8 + 4, 8)), Fake((H, W, 0), "|u1")):
        with pytest.raises(ValueError):
            render.source_arg(bad)


def test_reconstruct_value_errors():
    flow, src = Fake((4, 3, H, W), "<f4"), Fake((H, W, 3), "|u1", ptr=PTR + 0x100000)
    with pytest.raises(ValueError):
        render.reconstruct(Fake((W, H, 3), "|u1"), flow)                        # frame and flow differ in size
    with pytest.raises(ValueError):
        render.reconstruct(src, Fake((4, H, W, 2), "<f4"), layout="interleaved")   # use_m without an m
    with pytest.raises(ValueError):
        render.reconstruct(src, flow, dtype="int16")
    for out in (Fake((4, H, W), "|u1", ptr=OUT),                               # the channel axis is missing
                Fake((4, H, W, 3), "<f4", ptr=OUT),                            # not the requested dtype
                Fake((4, H, W, 3), "|u1", strides=(H * W * 4, W * 4, 4, 1), ptr=OUT)):   # not contiguous
        with pytest.raises(ValueError):
            render.reconstruct(src, flow, out=out)
    with pytest.raises(ValueError):
        render.luminosity(flow, out=Fake((4, H, W), "<f4", ptr=OUT))
    with pytest.raises(ValueError):
        render.luminosity(flow, out=Fake((4, H, W, 1), "|u1", ptr=OUT))
    with pytest.raises(ValueError):
        render.flow_color(flow, out=Fake((4, H, W), "|u1", ptr=OUT))
    with pytest.raises(ValueError):
        render.flow_color(flow, maxrad=Fake((3,), "<f8", ptr=OUT))               # 4 records need 4 values
    with pytest.raises(ValueError):
        render.flow_color(flow, maxrad=Fake((4,), "<f4", ptr=OUT))
    with pytest.raises(TypeError):
        render.reconstruct(src, [[0.0]])                                         # a host object
