"""Scoring entries (include/foto.h, "scoring"), the parts that need no GPU: the numpy restatement
tests/score_ref.py against the oracle's EE / AE / IE on the reference's own vectors (io.npz), the
argument rules of foto_score_check, every argument error the entries report before they touch a
device (on pointers that are never dereferenced), the ctypes structure against the C one, the
ValueErrors of foto.evaluate raised before the library is called, and main.py's --stats flag being
off by default."""
import ctypes
import math

import numpy as np
import pytest

from conftest import PKG  # noqa: F401  (puts the package on sys.path)

import score_ref
from foto import _lib, evaluate
from oracle import foto_oracle as O

W, H = 37, 29
ARG = _lib.FOTO_ERR_ARG
PTR = 0x7f0000010000   # a well-aligned address; argument errors return before anything reads it
GT, MASK, TABLE, MAPS = PTR + 0x100000, PTR + 0x200000, PTR + 0x300000, PTR + 0x400000


def _flow(data=PTR, dtype=_lib.FOTO_F32, layout=0, records=3):
    fl = _lib.Flow()
    fl.data, fl.dtype, fl.layout, fl.records = data, dtype, layout, records
    return fl


def _gt(**kw):
    args = dict(data=GT, layout=1, records=1)
    args.update(kw)
    return _flow(**args)


def _img(data=MASK, dtype=_lib.FOTO_U8, sy=W, sx=1, divisor=1.0):
    im = _lib.Image()
    im.data, im.dtype, im.stride_y, im.stride_x, im.divisor = data, dtype, sy, sx, divisor
    return im


def _opts(**kw):
    o = _lib.ScoreOpts()
    assert _lib.lib().foto_score_opts_default(ctypes.byref(o)) == 0
    for k, v in kw.items():
        if isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                getattr(o, k)[i] = x
        else:
            setattr(o, k, v)
    return o


def _ref(x):
    return ctypes.byref(x) if x is not None else None


# ------------------------------------------------------------------ score_ref against the oracle

def test_score_ref_gives_the_oracle_on_io(gold):
    d = gold("io.npz")
    w, h = (int(x) for x in d["wh"])
    flow = np.stack([d["u"].reshape(h, w), d["v"].reshape(h, w), np.zeros((h, w))])
    gt = np.stack([d["uGT"], d["vGT"]], axis=-1).reshape(h, w, 2)
    table, maps = score_ref.score_flow(flow, gt)
    aee, sdee = O.EE(w, h, d["u"], d["v"], d["uGT"], d["vGT"])
    aae, sdae = O.AE(w, h, d["u"], d["v"], d["uGT"], d["vGT"])
    assert table[0, 0] == w * h
    np.testing.assert_allclose(table[0, [2, 3, 14, 15]], [aee, sdee, aae, sdae], rtol=1e-14)
    np.testing.assert_allclose(table[0, [2, 3]], d["ee"], rtol=1e-13)   # the reference's own outputs
    np.testing.assert_allclose(table[0, [14, 15]], d["ae"], rtol=1e-13)
    assert np.all(table[0, 25:] == 0) and np.isnan(table[0, 8]) and np.isnan(table[0, 12])
    # the order statistics are samples, the fractions counts
    ee = maps[0, 0].ravel()
    ee = ee[ee <= 50]   # (io.npz has pixels above the cap: they are in the map, not in the statistics)
    assert table[0, 1] == ee.size < w * h
    assert table[0, 4] == ee.max() and all(a in ee for a in table[0, 9:12])
    assert table[0, 5] == np.count_nonzero(ee > 0.5) / ee.size
    rec = np.clip(d["rec"], 0, 1)   # (main.py:109-110: the reference scores the clipped reconstruction)
    fr = score_ref.score_frames(rec.reshape(h, w), d["f2"].reshape(h, w))
    np.testing.assert_allclose(fr[0, 1], O.IE(w, h, rec, d["f2"]), rtol=1e-14)
    np.testing.assert_allclose(fr[0, 1], d["ie"], rtol=1e-13)
    assert fr[0, 0] == w * h and fr[0, 2] <= fr[0, 1] and fr[0, 3] >= fr[0, 1]   # ne_eps = 1: NE <= IE <= max


def test_score_ref_rank_and_ties():
    assert [score_ref.rank(p, 10) for p in (0.001, 10, 10.5, 50, 95, 100)] == [1, 1, 2, 5, 10, 10]
    flow = np.zeros((3, 4, 5))
    flow[0], flow[1] = 3.0, 4.0
    table, _ = score_ref.score_flow(flow, np.zeros((4, 5, 2)))
    assert np.all(table[0, [2, 4, 9, 10, 11]] == 5.0) and table[0, 3] == 0.0
    assert np.all(table[0, 5:8] == 1.0)


# ------------------------------------------------------------------ foto_score_check

def _check(fl=None, gt=None, mask=None, w=W, h=H, opts=None):
    return _lib.lib().foto_score_check(_ref(fl), _ref(gt), _ref(mask), w, h, _ref(opts))


def test_score_check_accepts():
    L = _lib.lib()
    for kw in (dict(), dict(mask=_img()), dict(opts=_opts()), dict(gt=_gt(records=3, layout=0, dtype=_lib.FOTO_F64)),
               dict(opts=_opts(ee_cap=math.inf)), dict(opts=_opts(n_ee_thr=0, n_ae_thr=0, n_pct=0)),
               dict(opts=_opts(n_pct=4, pct=[100.0, 1e-9, 50.0, 99.0])),
               dict(opts=_opts(n_ee_thr=4, ee_thr=[0.0, 1.0, 2.0, 3.0])),
               dict(mask=_img(dtype=_lib.FOTO_F64, sy=2 * W, sx=2))):
        args = dict(fl=_flow(), gt=_gt())
        args.update(kw)
        assert _check(**args) == 0, (kw, L.foto_last_error())


def test_score_opts_default_values():
    o = _opts()
    assert (o.ee_cap, o.n_ee_thr, o.n_ae_thr, o.n_pct, o.reserved) == (50.0, 3, 3, 3, 0)
    assert list(o.ee_thr)[:3] == [0.5, 1.0, 2.0] and list(o.pct)[:3] == [50.0, 75.0, 95.0]
    assert list(o.ae_thr)[:3] == [float(np.deg2rad(x)) for x in (2.5, 5.0, 10.0)]
    assert tuple(o.ae_thr)[:3] == evaluate.AE_THRESHOLDS == score_ref.AE_THR
    assert _lib.lib().foto_score_opts_default(None) == ARG


REJECTS = [
    ("null flow", dict(fl=None)),
    ("null gt", dict(gt=None)),
    ("flow: null data", dict(fl=_flow(data=0))),
    ("flow: dtype uint8", dict(fl=_flow(dtype=_lib.FOTO_U8))),
    ("flow: layout 2", dict(fl=_flow(layout=2))),
    ("flow: records 0", dict(fl=_flow(records=0))),
    ("flow: records above the limit", dict(fl=_flow(records=65536), gt=_gt())),
    ("gt: dtype 3", dict(gt=_gt(dtype=3))),
    ("gt: float64 at a 4-byte address", dict(gt=_gt(data=GT + 4, dtype=_lib.FOTO_F64))),
    ("gt: 2 records for 3", dict(gt=_gt(records=2))),
    ("gt: 4 records for 3", dict(gt=_gt(records=4))),
    ("w 0", dict(w=0)),
    ("h < 0", dict(h=-1)),
    ("w h = 2^31", dict(w=65536, h=32768)),
    ("mask: null data", dict(mask=_img(data=0))),
    ("mask: dtype 3", dict(mask=_img(dtype=3))),
    ("mask: stride_x 0", dict(mask=_img(sx=0))),
    ("mask: rows overlap", dict(mask=_img(sy=W - 1))),
    ("ee_cap 0", dict(opts=_opts(ee_cap=0.0))),
    ("ee_cap < 0", dict(opts=_opts(ee_cap=-1.0))),
    ("ee_cap nan", dict(opts=_opts(ee_cap=math.nan))),
    ("n_ee_thr 5", dict(opts=_opts(n_ee_thr=5))),
    ("n_ae_thr -1", dict(opts=_opts(n_ae_thr=-1))),
    ("n_pct 5", dict(opts=_opts(n_pct=5))),
    ("ee_thr < 0", dict(opts=_opts(ee_thr=[0.5, -1.0, 2.0]))),
    ("ee_thr inf", dict(opts=_opts(ee_thr=[math.inf]))),
    ("ae_thr nan", dict(opts=_opts(ae_thr=[0.1, 0.2, math.nan]))),
    ("pct 0", dict(opts=_opts(pct=[0.0]))),
    ("pct > 100", dict(opts=_opts(pct=[50.0, 100.5]))),
    ("pct nan", dict(opts=_opts(pct=[math.nan]))),
    ("pct < 0", dict(opts=_opts(pct=[-5.0]))),
]


@pytest.mark.parametrize("name,kw", REJECTS)
def test_score_check_rejects(name, kw):
    L = _lib.lib()
    args = dict(fl=_flow(), gt=_gt(), mask=None, w=W, h=H, opts=None)
    args.update(kw)
    assert _check(**args) == ARG, name
    assert L.foto_last_error(), name
    # and both entries report the same before they touch a device
    a = (_ref(args["fl"]), _ref(args["gt"]), _ref(args["mask"]), args["w"], args["h"], _ref(args["opts"]),
         ctypes.c_void_p(TABLE), ctypes.c_void_p(MAPS), _lib.FOTO_F32)
    assert L.foto_score_flow_dev(*a, None) == ARG, name
    assert L.foto_score_flow(*a) == ARG, name


def test_unused_slots_are_not_judged():
    """Only the first n_* values of a list are arguments."""
    assert _check(fl=_flow(), gt=_gt(), opts=_opts(n_pct=1, pct=[50.0, -1.0, math.nan, 200.0])) == 0
    assert _check(fl=_flow(), gt=_gt(), opts=_opts(n_ee_thr=0, ee_thr=[-1.0])) == 0


@pytest.mark.parametrize("name,table,maps,maps_dtype", [
    ("null table", 0, MAPS, _lib.FOTO_F32),
    ("table at a 4-byte address", TABLE + 4, 0, _lib.FOTO_F64),
    ("maps_dtype uint8", TABLE, MAPS, _lib.FOTO_U8),
    ("maps_dtype 3", TABLE, MAPS, 3),
    ("float64 maps at a 4-byte address", TABLE, MAPS + 4, _lib.FOTO_F64),
])
def test_score_flow_output_errors(name, table, maps, maps_dtype):
    L = _lib.lib()
    a = (_ref(_flow()), _ref(_gt()), None, W, H, None, ctypes.c_void_p(table), ctypes.c_void_p(maps), maps_dtype)
    assert L.foto_score_flow_dev(*a, None) == ARG, name
    assert L.foto_score_flow(*a) == ARG, name
    assert L.foto_last_error(), name


def _frames(fr="d", count=4, stride_rec=W * H, tr="d", mask=None, w=W, h=H, eps=1.0, table=TABLE):
    fr = _img(data=PTR) if fr == "d" else fr
    tr = _img(data=GT, dtype=_lib.FOTO_F64) if tr == "d" else tr
    return _lib.lib().foto_score_frames_dev(_ref(fr), count, stride_rec, _ref(tr), _ref(mask), w, h, eps,
                                            ctypes.c_void_p(table), None)


@pytest.mark.parametrize("name,kw", [
    ("null frames", dict(fr=None)),
    ("null truth", dict(tr=None)),
    ("null table", dict(table=0)),
    ("count 0", dict(count=0)),
    ("count < 0", dict(count=-2)),
    ("count above the limit", dict(count=65536)),
    ("stride_rec 0", dict(stride_rec=0)),
    ("stride_rec < 0", dict(stride_rec=-W * H)),
    ("w 0", dict(w=0)),
    ("h 0", dict(h=0)),
    ("w h = 2^31", dict(w=65536, h=32768)),
    ("frames: dtype 3", dict(fr=_img(data=PTR, dtype=3))),
    ("frames: divisor 0", dict(fr=_img(data=PTR, divisor=0.0))),
    ("truth: stride_y < 0", dict(tr=_img(data=GT, sy=-W))),
    ("mask: null data", dict(mask=_img(data=0))),
    ("ne_eps < 0", dict(eps=-1.0)),
    ("ne_eps nan", dict(eps=math.nan)),
    ("ne_eps inf", dict(eps=math.inf)),
    ("table at a 4-byte address", dict(table=TABLE + 4)),
])
def test_score_frames_argument_errors(name, kw):
    assert _frames(**kw) == ARG, name
    assert _lib.lib().foto_last_error(), name


# ------------------------------------------------------------------ the structure

def test_score_opts_struct_layout():
    S = _lib.ScoreOpts
    assert ctypes.sizeof(S) == 120   # (foto_score.hip asserts the same of foto_score_opts)
    assert (S.ee_cap.offset, S.n_ee_thr.offset, S.n_ae_thr.offset, S.n_pct.offset, S.reserved.offset,
            S.ee_thr.offset, S.ae_thr.offset, S.pct.offset) == (0, 8, 12, 16, 20, 24, 56, 88)
    assert (_lib.FOTO_SCORE_COLS, evaluate.SCORE_COLS, score_ref.COLS) == (32, 32, 32)
    # the header's words
    import os
    import re
    from conftest import REPO
    src = open(os.path.join(REPO, "include", "foto.h")).read()
    assert re.search(r"#define FOTO_SCORE_COLS 32\b", src) and re.search(r"#define FOTO_SCORE_MAX_RECORDS 65535\b", src)
    body = re.search(r"typedef struct \{([^}]*)\} foto_score_opts;", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"\s+", " ", f.strip()) for f in body.split(";") if f.strip()]
    assert fields == ["double ee_cap", "int n_ee_thr", "int n_ae_thr", "int n_pct", "int reserved", "double ee_thr[4]",
                      "double ae_thr[4]", "double pct[4]"]


# ------------------------------------------------------------------ foto.evaluate: errors before the library

class Fake:
    """An object exposing a hand-written __cuda_array_interface__."""

    def __init__(self, shape, typestr, strides=None, ptr=PTR):
        self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(ptr, False), version=3,
                                             strides=strides)


def test_score_flow_value_errors():
    flow = Fake((3, 3, H, W), "<f4")
    gt = Fake((H, W, 2), "<f4", ptr=GT)
    with pytest.raises(ValueError):
        evaluate.score_flow(flow, gt, gt_layout="pairs")
    with pytest.raises(ValueError):
        evaluate.score_flow(flow, Fake((W, H, 2), "<f4", ptr=GT))                   # another size
    with pytest.raises(ValueError):
        evaluate.score_flow(flow, Fake((2, H, W, 2), "<f4", ptr=GT))                # 2 records for 3
    with pytest.raises(ValueError):
        evaluate.score_flow(flow, gt, percentiles=(1, 2, 3, 4, 5))
    with pytest.raises(ValueError):
        evaluate.score_flow(flow, gt, mask=Fake((H, W + 1), "|u1", ptr=MASK))
    with pytest.raises(ValueError):
        evaluate.score_flow(flow, gt, out=Fake((3, 31), "<f8", ptr=TABLE))
    with pytest.raises(ValueError):
        evaluate.score_flow(flow, gt, maps=Fake((3, 2, H, W), "|u1", ptr=MAPS))
    with pytest.raises(TypeError):
        evaluate.score_flow(np.zeros((3, H, W)), gt)                                # host and device mixed
    with pytest.raises(ValueError):
        evaluate.score_flow(np.zeros((3, H, W), np.int32), np.zeros((H, W, 2), np.float32))
    with pytest.raises(ValueError):
        evaluate.score_frames(Fake((4, H, W), "<f2"), Fake((H, W), "<f4", ptr=GT))
    with pytest.raises(ValueError):
        evaluate.score_frames(Fake((4, H, W), "<f4"), Fake((H, W + 1), "<f4", ptr=GT))


def test_score_opts_from_python():
    o = evaluate.score_opts(ee_cap=math.inf, ee_thresholds=(3.0,), ae_thresholds=(), percentiles=(100.0, 25.0))
    assert (o.ee_cap, o.n_ee_thr, o.n_ae_thr, o.n_pct) == (math.inf, 1, 0, 2)
    assert o.ee_thr[0] == 3.0 and list(o.pct)[:2] == [100.0, 25.0]
    assert _check(fl=_flow(), gt=_gt(), opts=o) == 0
    assert _check(fl=_flow(), gt=_gt(), opts=evaluate.score_opts()) == 0


# ------------------------------------------------------------------ main.py

def test_cli_stats_is_off_by_default():
    import main as M
    p = M.build_parser()
    assert p.parse_args(["a", "b"]).stats is False
    assert p.parse_args(["a", "b", "--ground-truth=g.flo"]).stats is False
    assert p.parse_args(["a", "b", "--ground-truth=g.flo", "--stats"]).stats is True
