"""Flow filtering (include/foto.h, "flow filtering"), the parts that need no GPU: the header and the
bindings, the layout and the defaults of foto_median_opts, every argument error foto_filter_check
and foto_flow_median_dev report before they touch a device (on pointers that are never
dereferenced), the ValueErrors / TypeErrors of foto.filter raised before the library is called,
tables(), main.py's flags being off by default, and the properties of the numpy restatement
tests/filter_ref.py that the GPU tests rest on: it agrees with scipy.ndimage.median_filter where
both are defined, returns the lower median on an even count, and does not depend on the window
order."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import PKG, REPO  # noqa: F401  (puts the package on sys.path)

import filter_ref as R
from foto import _lib
from foto import filter as F

W, H = 37, 29
ARG = _lib.FOTO_ERR_ARG
PTR = 0x7f0000010000   # a well-aligned address; argument errors return before anything reads it
GUIDE, MASK, OUT, VALID, TABLE = (PTR + k * 0x100000 for k in range(1, 6))


def _flow(data=PTR, dtype=_lib.FOTO_F32, layout=0, records=3):
    fl = _lib.Flow()
    fl.data, fl.dtype, fl.layout, fl.records = data, dtype, layout, records
    return fl


def _image(data=GUIDE, dtype=_lib.FOTO_U8, sy=W, sx=1, divisor=255.0):
    im = _lib.Image()
    im.data, im.dtype, im.stride_y, im.stride_x, im.divisor = data, dtype, sy, sx, divisor
    return im


def _opts(**kw):
    o = _lib.MedianOpts()
    assert _lib.lib().foto_median_opts_default(ctypes.byref(o)) == 0
    for k, v in kw.items():
        if k == "centre":
            o.spatial[o.radius * (2 * o.radius + 1) + o.radius] = v
        elif k == "range0":
            o.range[0] = v
        else:
            setattr(o, k, v)
    return o


def _ref(x):
    return ctypes.byref(x) if x is not None else None


def _args(**kw):
    a = dict(fl=_flow(), guide=None, channels=1, stride_c=1, mask=None, w=W, h=H, opts=_opts())
    a.update(kw)
    return a


def _check(a):
    return _lib.lib().foto_filter_check(_ref(a["fl"]), _ref(a["guide"]), a["channels"], a["stride_c"], _ref(a["mask"]),
                                        a["w"], a["h"], _ref(a["opts"]))


def _median(a, out=OUT, dtype=_lib.FOTO_F32, layout=0, valid=VALID, table=TABLE):
    return _lib.lib().foto_flow_median_dev(_ref(a["fl"]), _ref(a["guide"]), a["channels"], a["stride_c"], _ref(a["mask"]),
                                           a["w"], a["h"], _ref(a["opts"]), ctypes.c_void_p(out), dtype, layout,
                                           ctypes.c_void_p(valid), ctypes.c_void_p(table), None)


# ------------------------------------------------------------------ the header and the bindings

def test_header_and_bindings():
    src = open(os.path.join(REPO, "include", "foto.h")).read()
    for name in ("foto_median_opts_default", "foto_filter_check", "foto_flow_median_dev"):
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    for name, val in (("MAX_RADIUS", 7), ("MAX_ROUNDS", 64), ("MAX_RANGE", 256),
                      ("TILE_W", _lib.FOTO_MEDIAN_TILE_W), ("TILE_H", _lib.FOTO_MEDIAN_TILE_H)):
        assert re.search(rf"#define FOTO_MEDIAN_{name} {val}\b", src), name
        assert getattr(_lib, "FOTO_MEDIAN_" + name) == val
    assert src.index("flow filtering") > src.index("flow algebra")
    import foto
    assert foto.filter is F and (F.MAX_RADIUS, F.MAX_ROUNDS, F.MAX_RANGE, F.FILL_ROUNDS) == (7, 64, 256, 8)


def test_median_opts_struct_layout():
    S = _lib.MedianOpts
    assert ctypes.sizeof(S) == 992   # (foto_filter.hip asserts the same of foto_median_opts)
    src = open(os.path.join(PKG, "csrc", "foto_filter.hip")).read()
    assert re.search(r"static_assert\(sizeof\(foto_median_opts\) == 992\b", src)
    assert [(f[0], getattr(S, f[0]).offset) for f in S._fields_] == [
        ("radius", 0), ("rounds", 4), ("fill_only", 8), ("n_range", 12), ("range_scale", 16), ("spatial", 24),
        ("range", 24 + 2 * 225)]
    hdr = open(os.path.join(REPO, "include", "foto.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} foto_median_opts;", hdr).group(1)
    names = re.findall(r"\b(\w+)(?:\[[^\]]*\])?;", body)
    assert names == [f[0] for f in S._fields_]


def test_median_opts_default_values():
    o = _opts()
    assert (o.radius, o.rounds, o.fill_only, o.n_range, o.range_scale) == (2, 1, 0, 1, 255.0)
    assert list(o.spatial) == [1] * 225 and list(o.range) == [1] * 256
    assert _lib.lib().foto_median_opts_default(None) == ARG


# ------------------------------------------------------------------ argument errors before a device

@pytest.mark.parametrize("kw", [
    dict(),
    dict(w=1, h=1),
    dict(fl=_flow(dtype=_lib.FOTO_F64, layout=1, records=1)),
    dict(guide=_image()),
    dict(guide=_image(sy=3 * W, sx=3), channels=3, stride_c=1),
    dict(guide=_image(dtype=_lib.FOTO_F64, sy=W + 5, divisor=1.0), mask=_image(data=MASK, divisor=1.0)),
    dict(opts=_opts(radius=7, rounds=64, fill_only=1, n_range=256, range_scale=1e-3)),
    dict(opts=_opts(radius=1)),
])
def test_filter_check_accepts(kw):
    assert _check(_args(**kw)) == 0, (kw, _lib.lib().foto_last_error())


REJECTS = [
    ("null flow", dict(fl=None)),
    ("null data", dict(fl=_flow(data=0))),
    ("flow dtype uint8", dict(fl=_flow(dtype=_lib.FOTO_U8))),
    ("flow layout 2", dict(fl=_flow(layout=2))),
    ("records 0", dict(fl=_flow(records=0))),
    ("float64 at a 4-byte address", dict(fl=_flow(data=PTR + 4, dtype=_lib.FOTO_F64))),
    ("w 0", dict(w=0)),
    ("h < 0", dict(h=-2)),
    ("guide: null data", dict(guide=_image(data=0))),
    ("guide: dtype 3", dict(guide=_image(dtype=3))),
    ("guide: stride 0", dict(guide=_image(sx=0))),
    ("guide: divisor 0", dict(guide=_image(divisor=0.0))),
    ("guide: rows overlap", dict(guide=_image(sy=W - 1))),
    ("guide: channels 0", dict(guide=_image(), channels=0)),
    ("guide: stride_c 0", dict(guide=_image(), channels=3, stride_c=0)),
    ("guide: stride_c < 0", dict(guide=_image(), channels=3, stride_c=-1)),
    ("mask: null data", dict(mask=_image(data=0))),
    ("mask: float32 at a 2-byte address", dict(mask=_image(data=MASK + 2, dtype=_lib.FOTO_F32))),
    ("null opts", dict(opts=None)),
    ("radius 0", dict(opts=_opts(radius=0))),
    ("radius 8", dict(opts=_opts(radius=8))),
    ("rounds 0", dict(opts=_opts(rounds=0))),
    ("rounds 65", dict(opts=_opts(rounds=65))),
    ("fill_only 2", dict(opts=_opts(fill_only=2))),
    ("n_range 0", dict(opts=_opts(n_range=0))),
    ("n_range 257", dict(opts=_opts(n_range=257))),
    ("range_scale 0", dict(opts=_opts(range_scale=0.0))),
    ("range_scale < 0", dict(opts=_opts(range_scale=-1.0))),
    ("range_scale nan", dict(opts=_opts(range_scale=math.nan))),
    ("range_scale inf", dict(opts=_opts(range_scale=math.inf))),
    ("zero centre", dict(opts=_opts(centre=0))),
    ("zero centre at radius 7", dict(opts=_opts(radius=7, centre=0))),
    ("zero range[0]", dict(opts=_opts(range0=0))),
]


@pytest.mark.parametrize("name,kw", REJECTS)
def test_filter_check_rejects(name, kw):
    L = _lib.lib()
    a = _args(**kw)
    assert _check(a) == ARG, name
    assert L.foto_last_error(), name
    assert _median(a) == ARG, name            # and the entry reports the same before it touches a device


@pytest.mark.parametrize("name,kw", [
    ("null out", dict(out=0)),
    ("out_dtype uint8", dict(dtype=_lib.FOTO_U8)),
    ("out_dtype 3", dict(dtype=3)),
    ("out_layout 2", dict(layout=2)),
    ("out_layout -1", dict(layout=-1)),
    ("float64 out at a 4-byte address", dict(out=OUT + 4, dtype=_lib.FOTO_F64)),
    ("float32 out at a 2-byte address", dict(out=OUT + 2)),
    ("table at a 4-byte address", dict(table=TABLE + 4)),
])
def test_output_argument_errors(name, kw):
    assert _median(_args(), **kw) == ARG, name
    assert _lib.lib().foto_last_error(), name


# ------------------------------------------------------------------ what Python raises itself

class Fake:
    """An object exposing a hand-written __cuda_array_interface__."""

    def __init__(self, shape, typestr, strides=None, ptr=PTR):
        self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(ptr, False), version=3,
                                             strides=strides)


def test_filter_value_errors():
    flow = Fake((3, 3, H, W), "<f4")
    sp, rg = F.tables(2, 1.5, 0.1)
    for kw in (dict(in_layout="pairs"), dict(layout="pairs"), dict(dtype="uint8"), dict(radius=0), dict(radius=8),
               dict(radius=1.5), dict(rounds=0), dict(rounds=65), dict(range_scale=0.0), dict(range_scale=math.nan),
               dict(spatial=np.ones((3, 3), np.uint16)),                   # radius 2 takes 5 x 5
               dict(spatial=np.ones((5, 5))),                              # float weights
               dict(spatial=np.zeros((5, 5), np.uint16)),                  # a zero centre
               dict(spatial=np.full((5, 5), 70000)),                       # not a uint16
               dict(range=np.zeros(4, np.uint16)), dict(range=np.ones(257, np.uint16)), dict(range=np.ones((2, 2), np.uint16)),
               dict(guide=Fake((H + 1, W), "|u1", ptr=GUIDE)),             # another size
               dict(guide=Fake((H, W), "<i4", ptr=GUIDE)),                 # not a frame dtype
               dict(mask=Fake((H, W + 1), "|u1", ptr=MASK)),
               dict(mask=Fake((H, W, 3), "|u1", ptr=MASK)),
               dict(out=Fake((3, 3, H, W), "<f8", ptr=OUT)),               # out of another dtype
               dict(valid_out=Fake((3, H, W), "<f4", ptr=VALID)),
               dict(table_out=Fake((3, 3), "<f8", ptr=TABLE))):
        with pytest.raises((ValueError, TypeError)):
            F.median(flow, **kw)
    assert sp.shape == (5, 5) and rg.shape == (256,)
    with pytest.raises(TypeError):
        F.median(flow, guide=np.zeros((H, W), np.uint8))                    # host and device mixed
    with pytest.raises(TypeError):
        F.median(flow, mask=np.ones((H, W), np.uint8))
    with pytest.raises(ValueError):
        F.median(np.zeros((3, H, W)), out=Fake((3, H, W), "<f8", ptr=OUT))  # numpy in, numpy out
    with pytest.raises(TypeError):
        F.fill(flow, Fake((H, W), "|u1", ptr=MASK), fill_only=False)
    with pytest.raises(TypeError):
        F.median(object())
    bare = _image()                                                         # a foto_image not made by as_image: no shape
    with pytest.raises(TypeError):
        F.median(flow, guide=bare)
    with pytest.raises(TypeError):
        F.median(flow, mask=bare)


def test_tables():
    for radius in (1, 2, 7):
        sp, rg = F.tables(radius)
        assert sp.dtype == rg.dtype == np.uint16 and sp.shape == (2 * radius + 1,) * 2 and np.all(sp == 1)
        assert rg.shape == (1,) and rg[0] == 1
        sp, rg = F.tables(radius, sigma_s=1.5, sigma_r=0.05)
        assert sp.dtype == rg.dtype == np.uint16 and sp.shape == (2 * radius + 1,) * 2 and rg.shape == (256,)
        assert sp[radius, radius] == 1024 == sp.max() and rg[0] == 1024 == rg.max()
        assert np.array_equal(sp, sp.T) and np.array_equal(sp, sp[::-1]) and np.array_equal(sp, sp[:, ::-1])
        assert np.all(np.diff(rg.astype(int)) <= 0) and rg[-1] == 0
        d = np.arange(-radius, radius + 1.0)
        assert np.array_equal(sp, np.round(1024 * np.exp(-(d[:, None] ** 2 + d[None] ** 2) / (2 * 1.5 ** 2))))
        assert np.array_equal(rg, np.round(1024 * np.exp(-(np.arange(256) / 255.0) ** 2 / (2 * 0.05 ** 2))))
    sp, rg = F.tables(3, sigma_s=0.05, sigma_r=1e-4, levels=16, scale=15.0, unit=1)
    assert sp[3, 3] == 1 and sp.sum() == 1 and rg.shape == (16,) and rg[0] == 1 and rg.sum() == 1   # centres forced >= 1
    assert F.tables(2, unit=65535, sigma_s=1e6)[0].max() == 65535
    for bad in (dict(radius=0), dict(radius=8), dict(radius=2, sigma_s=0.0), dict(radius=2, sigma_r=-1.0),
                dict(radius=2, sigma_r=0.1, levels=257), dict(radius=2, sigma_r=0.1, scale=0.0), dict(radius=2, unit=65536)):
        with pytest.raises(ValueError):
            F.tables(**bad)
    o = F.median_opts(3, 5, True, *F.tables(3, 2.0, 0.1, levels=32), range_scale=31.0)
    assert (o.radius, o.rounds, o.fill_only, o.n_range, o.range_scale) == (3, 5, 1, 32, 31.0)
    assert list(o.spatial[:49]) == F.tables(3, 2.0)[0].ravel().tolist() and o.spatial[24] == 1024
    assert _check(_args(opts=o)) == 0


def test_cli_flags_are_off_by_default():
    import main as M
    p = M.build_parser()
    a = p.parse_args(["a", "b"])
    assert (a.median, a.median_rounds, a.fill_occluded) == (0, 1, False)
    a = p.parse_args(["a", "b", "--algo=GN", "--median", "3", "--median-rounds", "2", "--fill-occluded"])
    assert (a.median, a.median_rounds, a.fill_occluded) == (3, 2, True)
    for bad in (["--median", "8"], ["--median", "-1"], ["--median-rounds", "0"], ["--median-rounds", "65"]):
        with pytest.raises(SystemExit):                                     # rejected by the parser, before any solve
            p.parse_args(["a", "b"] + bad)


# ------------------------------------------------------------------ the restatement's own properties

def test_ref_keys_are_ordered_like_the_values():
    x = np.array([-np.inf, -3.5, -5e-324, -0.0, 0.0, 5e-324, 2.0, np.inf])
    k = R.keys(x)
    assert np.all(np.diff(k.astype(object)) > 0)
    assert R.keys(np.array([-0.0]))[0] + 1 == R.keys(np.array([0.0]))[0]


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_ref_interior_equals_scipy_median_filter(radius):
    """All-ones tables, no guide, no mask: a full window holds an odd count of equal weights, so the
    lower weighted median is the plain median -- scipy.ndimage.median_filter, exactly."""
    import scipy.ndimage as ndi
    h, w = 17, 23
    f = R.random_flow(1, h, w, "planar", np.float64, seed=radius)
    out, valid, table = R.median(f, radius=radius)
    s = slice(radius, -radius)
    for c in (0, 1):
        want = ndi.median_filter(f[0, c], size=2 * radius + 1)
        assert np.array_equal(out[0, c][s, s], want[s, s])
    assert np.array_equal(R.bits(out[0, 2]), R.bits(f[0, 2]))        # m passes through
    assert valid.all() and list(table[0]) == [w * h, 0, 0, 0]


def test_ref_even_count_gives_the_lower_median():
    # a 2 x 2 frame at R = 1: every window is the whole frame, 4 candidates of weight 1
    f = np.zeros((1, 3, 2, 2))
    f[0, 0] = [[4.0, 1.0], [3.0, 2.0]]
    f[0, 1] = [[-1.0, -4.0], [-2.0, -3.0]]
    out, _, _ = R.median(f, radius=1)
    assert np.all(out[0, 0] == 2.0) and np.all(out[0, 1] == -3.0)      # the 2nd smallest of 4, never the mean
    # three distinct values, equal weights, an even count: 2 cum == T is hit exactly at the lower one
    g = np.zeros((1, 3, 1, 4))
    g[0, 0, 0] = [7.0, 5.0, 5.0, 9.0]
    out, _, _ = R.median(g, radius=3)
    assert np.all(out[0, 0] == 5.0)
    g[0, 0, 0] = [7.0, 5.0, 9.0, 9.0]
    assert np.all(R.median(g, radius=3)[0][0, 0] == 7.0)
    # -0.0 sorts below +0.0
    z = np.zeros((1, 3, 1, 2))
    z[0, 0, 0] = [0.0, -0.0]
    assert np.all(np.signbit(R.median(z, radius=1)[0][0, 0]))


def test_ref_window_order_does_not_matter():
    h, w = 9, 11
    f = R.random_flow(2, h, w, "interleaved", np.float32, seed=4)
    f[0, 2, 3] = np.nan
    f[..., 0] = np.round(f[..., 0])                                     # many ties
    guide = np.random.default_rng(5).integers(0, 256, (h, w, 3), dtype=np.uint8)
    mask = np.random.default_rng(6).random((h, w)) > 0.3
    sp, rg = F.tables(2, 1.5, 0.2)
    kw = dict(layout="interleaved", guide=guide, mask=mask, radius=2, rounds=2, spatial=sp, rng=rg)
    a = R.median(f, **kw)
    b = R.median(f, shuffle=np.random.default_rng(7), **kw)
    for x, y in zip(a, b):
        R.same_bits(x, y)
    assert a[2][0, 1] > 0 and a[2].sum() == 2 * w * h


def test_ref_holes_fill_from_the_rim():
    h, w, radius = 12, 13, 1
    f = R.random_flow(1, h, w, "planar", np.float64, seed=8)
    mask = np.ones((h, w), np.uint8)
    mask[3:8, 4:9] = 0                                                  # side 2R + 3 = 5: rings of 16, 8, 1
    filled = []
    for rounds in (1, 2, 3):
        out, valid, table = R.median(f, mask=mask, radius=radius, rounds=rounds, fill_only=True)
        assert np.array_equal(R.bits(out[0, :2][:, mask == 1]), R.bits(f[0, :2][:, mask == 1]))
        assert table[0].sum() == w * h and table[0, 0] == w * h - 25 and valid.sum() == table[0, 0] + table[0, 1]
        filled.append(int(table[0, 1]))
    assert filled == [16, 24, 25]
    out, valid, table = R.median(f, mask=np.zeros((h, w)), radius=radius, rounds=3)
    assert np.array_equal(R.bits(out), R.bits(f)) and not valid.any() and list(table[0]) == [0, 0, w * h, 0]
