"""Frame preparation (include/foto.h, "frame preparation"), the parts that need no GPU: the numpy
restatement tests/prep_ref.py -- the yardstick of tests/test_gpu_prep.py -- against Pillow itself
(Image.resize for modes 'L' and 'F' with the four filters, convert('L')) and against the
repository's bin/ tools, all bit for bit; the library's host-side coefficient tables
(foto_resize_coeffs) against the restatement's, bit for bit, integer tables included; the header,
the bindings and the struct layout; every argument error the entries report before they touch a
device (on pointers that are never dereferenced) and the ValueErrors of foto.prep raised before the
library is called."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import PKG, REPO  # noqa: F401  (puts the package on sys.path)

import prep_ref as R
from foto import _lib, prep

sys.path.insert(0, os.path.join(PKG, "bin"))

ARG = _lib.FOTO_ERR_ARG
PTR = 0x7f0000010000   # a well-aligned address; argument errors return before anything reads it
OUT, OUT1 = PTR + 0x100000, PTR + 0x200000
W, H = 37, 29
SHAPES = [((53, 37), (26, 18)), ((53, 37), (27, 19)), ((64, 40), (32, 20)), ((29, 31), (58, 62)),
          ((29, 31), (17, 45)), ((16, 16), (7, 16)), ((200, 9), (3, 9)), ((7, 5), (1, 1))]
AXES = sorted({(a, b) for (w, h), (ow, oh) in SHAPES for a, b in ((w, ow), (h, oh))} | {(640, 7)})


def _pil_filters():
    from PIL import Image
    return {"box": Image.BOX, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}


# ------------------------------------------------------------------ the restatement against Pillow

@pytest.mark.parametrize("src,dst", SHAPES)
def test_restatement_equals_pillow_resize(src, dst):
    from PIL import Image
    (w, h), size = src, dst
    rng = np.random.default_rng(w * 100 + size[0])
    a8 = rng.integers(0, 256, (h, w), dtype=np.uint8)
    af = (rng.random((h, w)) * 300 - 20).astype(np.float32)
    for name, f in _pil_filters().items():
        p8 = np.asarray(Image.fromarray(a8, "L").resize(size, f))
        assert np.array_equal(p8, R.resize(a8, size, name)), ("L", name)
        pf = np.asarray(Image.fromarray(af, "F").resize(size, f))
        assert np.array_equal(pf.view(np.uint32), R.resize(af, size, name).view(np.uint32)), ("F", name)


def test_restatement_equals_pillow_gray():
    from PIL import Image
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (33, 41, 3), dtype=np.uint8)
    assert np.array_equal(np.asarray(Image.fromarray(rgb, "RGB").convert("L")), R.gray(rgb))
    rgba = np.concatenate([rgb, rng.integers(0, 256, (33, 41, 1), dtype=np.uint8)], axis=2)
    assert np.array_equal(R.gray(rgba), R.gray(rgb))
    # every grey level of a grey RGB pixel maps to itself: the weights sum to 65536
    g = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    assert np.array_equal(R.gray(g)[0], np.arange(256))


def test_restatement_float64_is_the_float32_path_in_double():
    """No Pillow mode holds float64; on float32-representable input whose every pass result is
    exact in float32 (box halving of small integers) the two paths agree."""
    a = np.random.default_rng(6).integers(0, 64, (8, 16)).astype(np.float32) * 4
    R.same_bits(R.resize(a, (8, 4), "box").astype(np.float64), R.resize(a.astype(np.float64), (8, 4), "box"))


# ------------------------------------------------------------------ the library's tables

@pytest.mark.parametrize("n_in,n_out", AXES)
def test_library_tables_equal_the_restatement(n_in, n_out):
    for name in prep.FILTERS:
        ks, bounds, kk, ki = prep.resize_coeffs(n_in, n_out, name)
        rks, rbounds, rkk = R.coeffs(n_in, n_out, name)
        assert ks == rks and np.array_equal(bounds, rbounds), name
        assert np.array_equal(kk.view(np.uint64), rkk.view(np.uint64)), name
        assert np.array_equal(ki, R.coeffs_int(rkk)), name
    if (n_in, n_out) == (640, 7):
        assert prep.resize_coeffs(640, 7, "lanczos")[0] == 551


def test_resize_coeffs_argument_errors():
    L = _lib.lib()
    ks = ctypes.c_int()
    kk = (ctypes.c_double * 4)()
    assert L.foto_resize_coeffs(10, 5, 3, None, None, None, None, 0) == ARG
    assert L.foto_resize_coeffs(0, 5, 3, ctypes.byref(ks), None, None, None, 0) == ARG
    assert L.foto_resize_coeffs(10, 0, 3, ctypes.byref(ks), None, None, None, 0) == ARG
    assert L.foto_resize_coeffs(10, 5, 4, ctypes.byref(ks), None, None, None, 0) == ARG
    assert L.foto_resize_coeffs(10, 5, -1, ctypes.byref(ks), None, None, None, 0) == ARG
    assert L.foto_resize_coeffs(10, 5, 3, ctypes.byref(ks), None, kk, None, 4) == ARG   # cap too small
    assert L.foto_resize_coeffs(10, 5, 3, ctypes.byref(ks), None, None, None, 0) == 0 and ks.value == 13
    for bad in (dict(n_in=0, n_out=3), dict(n_in=3, n_out=0), dict(n_in=3, n_out=3, filter="hamming")):
        with pytest.raises(ValueError):
            prep.resize_coeffs(**bad)


# ------------------------------------------------------------------ the restatement against bin/

def test_difference_equals_bin_data_diff():
    from data_diff import frame_diff
    rng = np.random.default_rng(7)
    a, b = rng.integers(0, 256, (48, 64), dtype=np.uint8), rng.integers(0, 256, (48, 64), dtype=np.uint8)
    want = frame_diff(a.ravel() / 255, b.ravel() / 255).reshape(48, 64)
    R.same_bits(R.difference(a, b, "float64"), want)
    R.same_bits(R.difference(a, b, "uint8"), np.uint8(255 * np.clip(want, 0, 1)))


@pytest.mark.parametrize("seed", [1, 12345, 31337])
def test_illuminate_equals_bin_create_lum_dataset(seed):
    from create_lum_dataset import lum_image
    w, h = 64, 48
    f = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    want = lum_image(f.ravel() / 255, w, h, seed).reshape(h, w)
    shapes = prep.lum_shapes(w, h, seed)
    assert [s[0] for s in shapes] == ["rect", "rect", "circle", "circle"]
    R.same_bits(R.illuminate(f, shapes, "float64"), want)
    R.same_bits(R.illuminate(f, shapes, "uint8"), np.uint8(255 * np.clip(want, 0, 1)))


def test_normalize_pair_equals_bin_normalize_image():
    from normalize_image import normalize_pair
    rng = np.random.default_rng(8)
    a, b = rng.integers(0, 256, (30, 40), dtype=np.uint8), rng.integers(0, 200, (30, 40), dtype=np.uint8)
    fa, fb = a.ravel() / 255, b.ravel() / 255
    w0, w1 = normalize_pair(fa, fb)
    g0, g1, (m0, m1) = R.normalize_pair(a, b, np.sum(fa), np.sum(fb), "float64")
    R.same_bits(g0.ravel(), w0)
    R.same_bits(g1.ravel(), w1)
    assert (m0, m1) == (fa.max(), fb.max())
    u0, _, _ = R.normalize_pair(a, b, np.sum(fa), np.sum(fb), "uint8")
    R.same_bits(u0.ravel(), np.uint8(255 * np.clip(w0, 0, 1)))


# ------------------------------------------------------------------ the header and the bindings

ENTRIES = ("foto_prep_gray_dev", "foto_resize_coeffs", "foto_resize_plan_create", "foto_resize_plan_device",
           "foto_resize_plan_info", "foto_resize_dev", "foto_flow_resize_dev", "foto_prep_normalize_pair_dev",
           "foto_prep_illuminate_dev", "foto_prep_diff_dev")


def test_header_and_bindings():
    src = open(os.path.join(REPO, "include", "foto.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert re.search(r"\bvoid foto_resize_plan_destroy\(", src) and "foto_resize_plan_destroy" in _lib.SIGNATURES
    for name, val in (("FILTER_BOX", 0), ("FILTER_BILINEAR", 1), ("FILTER_BICUBIC", 2), ("FILTER_LANCZOS", 3),
                      ("PREP_TILE_X", prep.TILE_X), ("PREP_MAX_SHAPES", 8), ("RESIZE_ROUTE_AUTO", 0),
                      ("RESIZE_ROUTE_LDS", 1), ("RESIZE_ROUTE_DIRECT", 2), ("LUM_RECT", 0), ("LUM_CIRCLE", 1)):
        assert re.search(rf"#define FOTO_{name} {val}\b", src), name
        assert getattr(_lib, "FOTO_" + name) == val
    assert src.index("frame preparation") > src.index("flow filtering")
    import foto
    assert foto.prep is prep and prep.TILE_X == 64 and list(prep.FILTERS) == ["box", "bilinear", "bicubic", "lanczos"]
    assert callable(foto.device.prepare_pair)
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "foto_prep.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1)


def test_oversized_tables_are_refused_before_any_allocation():
    """n_out * ksize of an axis is bounded by FOTO_RESIZE_MAX_TABLE: a reduction of 2^30 -> 1 would
    overflow the int tap count, 2^30 -> 2^30 would ask for tens of GB on the host."""
    L = _lib.lib()
    ks = ctypes.c_int()
    p = ctypes.c_void_p()
    hdr = open(os.path.join(REPO, "include", "foto.h")).read()
    assert re.search(r"#define FOTO_RESIZE_MAX_TABLE \(1 << 22\)", hdr) and _lib.FOTO_RESIZE_MAX_TABLE == 1 << 22
    for n_in, n_out in ((1 << 30, 1), (1 << 30, 1 << 30), (1, 1 << 30)):
        for filt in range(4):
            assert L.foto_resize_coeffs(n_in, n_out, filt, ctypes.byref(ks), None, None, None, 0) == ARG, (n_in, n_out)
            assert "FOTO_RESIZE_MAX_TABLE" in _err()
        assert L.foto_resize_plan_create(n_in, 1, n_out, 1, 3, ctypes.byref(p)) == ARG and not p.value
        assert L.foto_resize_plan_create(1, n_in, 1, n_out, 3, ctypes.byref(p)) == ARG and not p.value
    assert L.foto_resize_coeffs(1 << 21, 1, 3, ctypes.byref(ks), None, None, None, 0) == ARG   # 6 * 2^21 + 1 taps
    # the largest tables that pass: a 2x Lanczos reduction to 2^18 outputs (13 taps), box of 2^20 -> 1
    assert L.foto_resize_coeffs(1 << 19, 1 << 18, 3, ctypes.byref(ks), None, None, None, 0) == 0 and ks.value == 13
    assert L.foto_resize_coeffs(1 << 20, 1, 0, ctypes.byref(ks), None, None, None, 0) == 0 and ks.value == (1 << 20) + 1
    with pytest.raises(_lib.FotoError, match="FOTO_RESIZE_MAX_TABLE"):
        prep.resize_coeffs(1 << 30, 1)


def test_lum_shape_struct_layout():
    S = _lib.LumShape
    assert ctypes.sizeof(S) == 48   # (foto_prep.hip asserts the same of foto_lum_shape)
    src = open(os.path.join(PKG, "csrc", "foto_prep.hip")).read()
    assert re.search(r"static_assert\(sizeof\(foto_lum_shape\) == 48\b", src)
    assert [(f[0], getattr(S, f[0]).offset) for f in S._fields_] == [("kind", 0), ("reserved", 4), ("p", 8), ("v", 40)]
    hdr = open(os.path.join(REPO, "include", "foto.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} foto_lum_shape;", hdr).group(1)
    assert re.findall(r"\b(\w+)(?:\[[^\]]*\])?;", body) == [f[0] for f in S._fields_]
    assert ctypes.sizeof(_lib.Image) == 40 and ctypes.sizeof(_lib.Flow) == 24


# ------------------------------------------------------------------ argument errors before a device

def _image(data=PTR, dtype=_lib.FOTO_U8, sy=W, sx=1, divisor=255.0):
    im = _lib.Image()
    im.data, im.dtype, im.stride_y, im.stride_x, im.divisor = data, dtype, sy, sx, divisor
    return im


def _ref(x):
    return ctypes.byref(x) if x is not None else None


def _shapes(*items):
    arr = (_lib.LumShape * max(len(items), 1))()
    for k, (kind, p, v) in enumerate(items):
        arr[k].kind, arr[k].v = kind, v
        for j, x in enumerate(p):
            arr[k].p[j] = x
    return arr


def _err():
    return _lib.lib().foto_last_error().decode()


GRAY_REJECTS = [
    ("null image", dict(src=None)),
    ("null out", dict(out=0)),
    ("1 channel", dict(channels=1)),
    ("5 channels", dict(channels=5)),
    ("stride_c 0", dict(stride_c=0)),
    ("w 0", dict(w=0)),
    ("null data", dict(src=_image(data=0, sy=3 * W, sx=3))),
    ("dtype 3", dict(src=_image(dtype=3, sy=3 * W, sx=3))),
    ("overlapping rows", dict(src=_image(sy=W - 1, sx=3))),
    ("float64 out at a 4-byte address", dict(src=_image(dtype=_lib.FOTO_F64, sy=3 * W, sx=3, divisor=1.0), out=OUT + 4)),
]


@pytest.mark.parametrize("what,kw", GRAY_REJECTS, ids=[r[0] for r in GRAY_REJECTS])
def test_gray_rejects_before_a_device(what, kw):
    a = dict(src=_image(sy=3 * W, sx=3), channels=3, stride_c=1, w=W, h=H, out=OUT)
    a.update(kw)
    rc = _lib.lib().foto_prep_gray_dev(_ref(a["src"]), a["channels"], a["stride_c"], a["w"], a["h"],
                                       ctypes.c_void_p(a["out"]), None)
    assert rc == ARG and "foto_prep_gray_dev" in _err(), what


def test_plan_create_rejects():
    L = _lib.lib()
    p = ctypes.c_void_p()
    for args in ((0, 5, 3, 3, 3), (5, 0, 3, 3, 3), (5, 5, 0, 3, 3), (5, 5, 3, -1, 3), (5, 5, 3, 3, 4), (5, 5, 3, 3, -1),
                 (1 << 16, 1 << 15, 3, 3, 3)):
        assert L.foto_resize_plan_create(*args, ctypes.byref(p)) == ARG and not p.value, args
    assert L.foto_resize_plan_create(5, 5, 3, 3, 3, None) == ARG
    assert L.foto_resize_plan_device(None) == -1
    assert L.foto_resize_plan_info(None, None) == ARG
    assert L.foto_resize_dev(None, _ref(_image()), 1, 1, ctypes.c_void_p(OUT), 0, 0, None) == ARG
    fl = _lib.Flow()
    fl.data, fl.dtype, fl.layout, fl.records = PTR, _lib.FOTO_F32, 0, 1
    assert L.foto_flow_resize_dev(None, _ref(fl), ctypes.c_void_p(OUT), 0, None) == ARG


PAIR_REJECTS = [
    ("null f0", dict(f0=None)),
    ("null f1", dict(f1=None)),
    ("h 0", dict(h=0)),
    ("stride 0", dict(f0=_image(sx=0))),
    ("divisor nan", dict(f1=_image(divisor=float("nan")))),
    ("null out", dict(out=0)),
    ("out_dtype 3", dict(out_dtype=3)),
    ("out_dtype -1", dict(out_dtype=-1)),
    ("float32 out at an odd address", dict(out=OUT + 2, out_dtype=_lib.FOTO_F32)),
]


@pytest.mark.parametrize("what,kw", PAIR_REJECTS, ids=[r[0] for r in PAIR_REJECTS])
def test_pair_entries_reject_before_a_device(what, kw):
    a = dict(f0=_image(), f1=_image(data=PTR + 0x80000), w=W, h=H, out=OUT, out_dtype=_lib.FOTO_U8)
    a.update(kw)
    st = (ctypes.c_double * 4)()
    L = _lib.lib()
    rc = L.foto_prep_normalize_pair_dev(_ref(a["f0"]), _ref(a["f1"]), a["w"], a["h"], ctypes.c_void_p(a["out"]),
                                        ctypes.c_void_p(OUT1), a["out_dtype"], st, None)
    assert rc == ARG and "foto_prep_normalize_pair_dev" in _err(), what
    rc = L.foto_prep_diff_dev(_ref(a["f0"]), _ref(a["f1"]), a["w"], a["h"], ctypes.c_void_p(a["out"]), a["out_dtype"],
                              None, None)
    assert rc == ARG and "foto_prep_diff_dev" in _err(), what


def test_normalize_needs_its_statistics_and_second_output():
    L = _lib.lib()
    st = (ctypes.c_double * 4)()
    a, b = _image(), _image(data=PTR + 0x80000)
    assert L.foto_prep_normalize_pair_dev(_ref(a), _ref(b), W, H, ctypes.c_void_p(OUT), ctypes.c_void_p(OUT1), 0, None,
                                          None) == ARG
    assert L.foto_prep_normalize_pair_dev(_ref(a), _ref(b), W, H, ctypes.c_void_p(OUT), None, 0, st, None) == ARG


LUM_REJECTS = [
    ("null image", dict(src=None)),
    ("null out", dict(out=0)),
    ("out_dtype 3", dict(out_dtype=3)),
    ("9 shapes", dict(count=9)),
    ("-1 shapes", dict(count=-1)),
    ("null shapes", dict(shapes=None, count=1)),
    ("kind 2", dict(shapes=_shapes((2, (1, 1, 1, 1), 0.1)), count=1)),
    ("value nan", dict(shapes=_shapes((0, (4, 4, 8, 8), float("nan"))), count=1)),
    ("rectangle bound inf", dict(shapes=_shapes((0, (float("inf"), 4, 8, 8), 0.1)), count=1)),
    ("rectangle bound 1e12", dict(shapes=_shapes((0, (4, 4, 1e12, 8), 0.1)), count=1)),
    ("radius nan", dict(shapes=_shapes((1, (float("nan"), 4, 8, 0), 0.1)), count=1)),
]


@pytest.mark.parametrize("what,kw", LUM_REJECTS, ids=[r[0] for r in LUM_REJECTS])
def test_illuminate_rejects_before_a_device(what, kw):
    a = dict(src=_image(), shapes=_shapes((0, (4, 4, 8, 8), 0.1)), count=1, out=OUT, out_dtype=_lib.FOTO_U8)
    a.update(kw)
    rc = _lib.lib().foto_prep_illuminate_dev(_ref(a["src"]), W, H, a["shapes"], a["count"], ctypes.c_void_p(a["out"]),
                                             a["out_dtype"], None)
    assert rc == ARG and "foto_prep_illuminate_dev" in _err(), what


# ------------------------------------------------------------------ foto.prep raises before the library

class _Fake:
    """A device array that is never read: the checks under test come before the library."""

    def __init__(self, shape, typestr="|u1"):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (PTR, False), "version": 3,
                                         "strides": None}


def test_python_errors_come_before_the_library(monkeypatch):
    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(prep, "lib", boom)
    monkeypatch.setattr(prep.D, "runtime_check", lambda: None)
    grey, rgb = _Fake((H, W)), _Fake((H, W, 3))
    with pytest.raises(ValueError, match="3 .RGB. or 4"):
        prep.gray(grey)
    with pytest.raises(ValueError, match="3 .RGB. or 4"):
        prep.gray(_Fake((H, W, 2)))
    with pytest.raises(ValueError, match="typestr"):
        prep.gray(_Fake((H, W, 3), "<i4"))
    with pytest.raises(ValueError, match="filter"):
        prep.resize(grey, (10, 10), "hamming")
    with pytest.raises(ValueError, match="size"):
        prep.resize(grey, (0, 10))
    with pytest.raises(ValueError, match="size"):
        prep.resize(grey, -0.5)
    with pytest.raises(ValueError, match="size"):
        prep.resize(grey, (1, 2, 3))
    with pytest.raises(ValueError, match="filter"):
        prep.resize_flow(_Fake((3, H, W), "<f4"), (10, 10), "nearest")
    with pytest.raises(ValueError, match="float32 or float64"):
        prep.resize_flow(_Fake((3, H, W)), (10, 10))
    with pytest.raises(ValueError, match="layout"):
        prep.resize_flow(_Fake((3, H, W), "<f4"), (10, 10), layout="hwc")
    with pytest.raises(ValueError, match="differ in shape"):
        prep.normalize_pair(grey, _Fake((H, W + 1)))
    with pytest.raises(ValueError, match="dtype"):
        prep.normalize_pair(grey, grey, dtype="int16")
    with pytest.raises(ValueError, match="dtype"):
        prep.difference(grey, grey, dtype="float16")
    with pytest.raises(ValueError, match="2-D"):
        prep.illuminate(rgb, [])
    with pytest.raises(ValueError, match="at most 8"):
        prep.illuminate(grey, [("circle", 1, 2, 3, 0.1)] * 9)
    with pytest.raises(ValueError, match="shape 0"):
        prep.illuminate(grey, [("ellipse", 1, 2, 3, 0.1)])
    with pytest.raises(ValueError, match="shape 0"):
        prep.illuminate(grey, [("rect", 1, 2, 3, 0.1)])
    with pytest.raises(ValueError, match="non-finite"):
        prep.illuminate(grey, [("circle", 1, 2, float("inf"), 0.1)])
    with pytest.raises(ValueError, match="route"):
        prep.ResizePlan.resize(object.__new__(prep.ResizePlan), grey, route="fast")


def test_size_forms():
    assert prep._size((26, 18), 53, 37) == (26, 18)
    assert prep._size("26x18", 53, 37) == (26, 18) and prep._size("26X18", 53, 37) == (26, 18)
    assert prep._size(0.5, 53, 37) == (max(1, round(53 * 0.5)), max(1, round(37 * 0.5))) == (26, 18)
    assert prep._size("0.5", 64, 40) == (32, 20)
    assert prep._size(0.01, 7, 5) == (1, 1)


def test_lum_shapes_are_the_reference_draws():
    import random
    shapes = prep.lum_shapes(64, 48, 99)
    random.seed(99)
    L_x = random.randint(10, 63)
    assert shapes[0][1] == L_x and len(shapes) == 4
    assert all(-0.25 <= s[-1] <= 0.25 for s in shapes)


def test_cli_switches_are_off_by_default():
    import main as M
    import run
    a = M.build_parser().parse_args(["f0.png", "f1.png"])
    assert (a.resize, a.resize_filter, a.normalize_pair, a.flow_full_size) == (None, "lanczos", False, False)
    a = M.build_parser().parse_args(["f0.png", "f1.png", "--resize", "320x240", "--resize-filter", "bicubic",
                                     "--normalize-pair", "--flow-full-size"])
    assert (a.resize, a.resize_filter, a.normalize_pair, a.flow_full_size) == ("320x240", "bicubic", True, True)
    with pytest.raises(SystemExit):
        M.build_parser().parse_args(["f0.png", "f1.png", "--resize-filter", "hamming"])
    with pytest.raises(SystemExit, match="--flow-full-size needs --resize"):
        M.main(["f0.png", "f1.png", "--algo=GN", "--flow-full-size"])
    assert run.parse_args(["prepare"]).device is False and run.parse_args(["prepare", "--device"]).device is True
    assert run.parse_args(["run", "--devices", "0,0"]).device is False


def test_lum_image_is_unchanged_by_the_shared_draw():
    """bin/create_lum_dataset.py keeps its own draws; prep.lum_shapes restates them: the same
    `random` calls, so the same state afterwards."""
    import random
    from create_lum_dataset import lum_image
    lum_image(np.zeros(64 * 48), 64, 48, 5)
    after_tool = random.random()
    prep.lum_shapes(64, 48, 5)
    assert random.random() == after_tool
