"""Device-buffer interface, the parts that need no GPU: foto_image_check (pure host validation
of the strided descriptor), foto.device.as_image on hand-written __cuda_array_interface__
objects, and the one-HIP-runtime-per-process rule (foto.device.runtime_check), each ordering in
a fresh child process."""
import ctypes
import math
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, REPO

from foto import _lib
from foto import device as D


def _img(data=0x10000, dtype=_lib.FOTO_F64, sy=37, sx=1, divisor=1.0):
    im = _lib.Image()
    im.data, im.dtype, im.stride_y, im.stride_x, im.divisor = data, dtype, sy, sx, divisor
    return im


def _check(im, w=37, h=29):
    return _lib.lib().foto_image_check(ctypes.byref(im), w, h)


@pytest.mark.parametrize("name,im", [
    ("contiguous", _img()),
    ("row-padded", _img(sy=41)),
    ("channel of [H][W][3]", _img(sy=37 * 3, sx=3)),
    ("transposed", _img(sy=1, sx=29)),
    ("transposed, padded", _img(sy=1, sx=32)),
    ("uint8 / 255, odd address", _img(data=0x10001, dtype=_lib.FOTO_U8, divisor=255.0)),
    ("float32, 4-byte aligned", _img(data=0x10004, dtype=_lib.FOTO_F32)),
    ("negative divisor", _img(divisor=-2.0)),
])
def test_image_check_accepts(name, im):
    assert _check(im) == 0, (name, _lib.lib().foto_last_error())


@pytest.mark.parametrize("name,im", [
    ("null data", _img(data=0)),
    ("dtype -1", _img(dtype=-1)),
    ("dtype 3", _img(dtype=3)),
    ("dtype 7", _img(dtype=7)),
    ("stride_x 0", _img(sx=0)),
    ("stride_y 0", _img(sy=0)),
    ("stride_x < 0", _img(sx=-1)),
    ("stride_y < 0", _img(sy=-37)),
    ("divisor 0", _img(divisor=0.0)),
    ("divisor -0", _img(divisor=-0.0)),
    ("divisor inf", _img(divisor=math.inf)),
    ("divisor nan", _img(divisor=math.nan)),
    ("float64 at an odd address", _img(data=0x10001)),
    ("float64 at a 4-byte address", _img(data=0x10004)),
    ("float32 at a 2-byte address", _img(data=0x10002, dtype=_lib.FOTO_F32)),
    ("rows overlap (pitch w - 1)", _img(sy=36)),
    ("rows overlap (stride_x 3, pitch 3 w - 3)", _img(sy=3 * 36, sx=3)),
    ("columns overlap (transposed, pitch h - 1)", _img(sy=1, sx=28)),
    ("equal strides", _img(sy=5, sx=5)),
])
def test_image_check_rejects(name, im):
    assert _check(im) == _lib.FOTO_ERR_ARG, name
    assert _lib.lib().foto_last_error(), name   # every failure has a message


def test_image_check_null_and_sizes():
    L = _lib.lib()
    assert L.foto_image_check(None, 4, 4) == _lib.FOTO_ERR_ARG
    assert _check(_img(), w=0) == _lib.FOTO_ERR_ARG
    assert _check(_img(), h=0) == _lib.FOTO_ERR_ARG
    # a single row or column cannot overlap itself, whatever the other stride
    assert _check(_img(sy=1, sx=1), w=37, h=1) == 0
    assert _check(_img(sy=1, sx=1), w=1, h=29) == 0


def test_image_struct_layout():
    assert ctypes.sizeof(_lib.Image) == 40   # (foto_dev.hip asserts the same of foto_image)
    assert _lib.Image.stride_y.offset == 16 and _lib.Image.divisor.offset == 32


class Fake:
    """An object exposing a hand-written __cuda_array_interface__."""

    def __init__(self, shape, typestr, strides=None, ptr=0x7f0000000000, **extra):
        self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(ptr, False), version=3,
                                             strides=strides, **extra)


@pytest.mark.parametrize("typestr,code,item,divisor", [
    ("|u1", _lib.FOTO_U8, 1, 255.0),
    ("<f4", _lib.FOTO_F32, 4, 1.0),
    ("<f8", _lib.FOTO_F64, 8, 1.0),
])
def test_as_image_dtypes_and_strides(typestr, code, item, divisor):
    im = D.as_image(Fake((29, 37), typestr))
    assert (im.dtype, im.stride_y, im.stride_x, im.divisor, im.shape) == (code, 37, 1, divisor, (29, 37))
    assert im.data == 0x7f0000000000
    assert _check(im) == 0
    # byte strides -> element strides: row-padded, a channel of [H][W][3], transposed
    im = D.as_image(Fake((29, 37), typestr, strides=(41 * item, item)))
    assert (im.stride_y, im.stride_x) == (41, 1)
    im = D.as_image(Fake((29, 37), typestr, strides=(37 * 3 * item, 3 * item)))
    assert (im.stride_y, im.stride_x) == (111, 3)
    im = D.as_image(Fake((29, 37), typestr, strides=(item, 29 * item)))
    assert (im.stride_y, im.stride_x) == (1, 29) and _check(im) == 0
    assert D.as_image(Fake((29, 37), typestr), divisor=2.0).divisor == 2.0


def test_as_image_explicit_mapping():
    im = D.as_image({"ptr": 0x1000, "typestr": "<f4", "shape": (4, 6), "strides": (32, 4)})
    assert (im.data, im.dtype, im.stride_y, im.stride_x, im.shape) == (0x1000, _lib.FOTO_F32, 8, 1, (4, 6))


def test_as_image_rejections():
    with pytest.raises(ValueError):
        D.as_image(Fake((3, 29, 37), "<f8"))            # 3-D
    with pytest.raises(ValueError):
        D.as_image(Fake((37,), "<f8"))                  # 1-D
    with pytest.raises(TypeError):
        D.as_image(Fake((29, 37), "<f2"))               # float16
    with pytest.raises(TypeError):
        D.as_image(Fake((29, 37), ">f8"))               # not native byte order
    with pytest.raises(ValueError):
        D.as_image(Fake((29, 37), "<f8", strides=(37 * 8 + 4, 8)))   # byte stride not a multiple of 8
    with pytest.raises(ValueError):
        D.as_image(Fake((29, 37), "<f4", strides=(37 * 4, 2)))
    with pytest.raises(TypeError):
        D.as_image(np.zeros((29, 37)))                  # a host array has no device interface


def test_stream_handle():
    class S:
        cuda_stream = 0xabc0
    assert D.stream_handle(None) == 0
    assert D.stream_handle(None, Fake((2, 2), "<f8")) == 0
    assert D.stream_handle(None, Fake((2, 2), "<f8", stream=1)) == 0          # legacy default stream
    assert D.stream_handle(None, Fake((2, 2), "<f8", stream=2)) == 2          # per-thread default
    assert D.stream_handle(None, Fake((2, 2), "<f8", stream=0x5550)) == 0x5550
    assert D.stream_handle(S(), Fake((2, 2), "<f8", stream=0x5550)) == 0xabc0  # explicit wins
    assert D.stream_handle(0x10) == 0x10
    with pytest.raises(ValueError):
        D.stream_handle(None, Fake((2, 2), "<f8", stream=0))


_CHILD = r"""
import sys
sys.path[:0] = [{repo!r}, {pkg!r}]
from foto import _lib, device
{first}
{second}
found = device.mapped_hip_runtimes()
print("RUNTIMES", len(found), found)
try:
    device.runtime_check()
    print("CHECK ok")
except _lib.FotoError as e:
    print("CHECK raised:", e)
"""


def _child(first, second):
    code = _CHILD.format(repo=REPO, pkg=PKG, first=first, second=second)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_runtime_rule_torch_first():
    out = _child("import torch", "_lib.lib()")
    assert "RUNTIMES 1 " in out, out
    assert "CHECK ok" in out, out


def test_runtime_rule_foto_first():
    out = _child("_lib.lib()", "import torch")
    assert "CHECK raised:" in out, out
    msg = out.split("CHECK raised:", 1)[1]
    assert msg.count("libamdhip64") >= 2 and "import torch before the first foto call" in msg, out
