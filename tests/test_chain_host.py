"""Flow algebra (include/foto.h, "flow algebra"), the parts that need no GPU: the argument rules of
foto_chain_check and every argument error the three entries report before they touch a device (on
pointers that are never dereferenced), the defaults and signatures as Python sees them, the
ValueErrors of foto.chain raised before the library is called, main.py's --save-consistency being
off by default, and the properties of the numpy reference tests/chain_ref.py that the GPU tests'
conditions rest on -- shown satisfiable here, before a GPU sees them."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import PKG, REPO  # noqa: F401  (puts the package on sys.path)

import chain_ref as R
from chain_ref import CONS, SHIFTS
from foto import _lib, chain

W, H = 37, 29
ARG = _lib.FOTO_ERR_ARG
PTR = 0x7f0000010000   # a well-aligned address; argument errors return before anything reads it
BWD, OUT, TABLE, ERR = PTR + 0x100000, PTR + 0x200000, PTR + 0x300000, PTR + 0x400000


def _flow(data=PTR, dtype=_lib.FOTO_F32, layout=0, records=3):
    fl = _lib.Flow()
    fl.data, fl.dtype, fl.layout, fl.records = data, dtype, layout, records
    return fl


def _ref(x):
    return ctypes.byref(x) if x is not None else None


def _check(a=None, b=None, w=W, h=H):
    return _lib.lib().foto_chain_check(_ref(a), _ref(b), w, h)


# ------------------------------------------------------------------ foto_chain_check

@pytest.mark.parametrize("kw", [
    dict(),
    dict(b=_flow(data=BWD)),
    dict(b=_flow(data=BWD, records=1)),
    dict(a=_flow(dtype=_lib.FOTO_F64, layout=1, records=1), b=_flow(data=BWD, layout=1, records=1)),
    dict(w=2, h=2),
    dict(a=_flow(data=PTR + 4, layout=1)),   # pairs need no more than the element's alignment
    dict(a=_flow(records=100000)),
])
def test_chain_check_accepts(kw):
    args = dict(a=_flow())
    args.update(kw)
    assert _check(**args) == 0, (kw, _lib.lib().foto_last_error())


REJECTS = [
    ("null flow", dict(a=None)),
    ("null data", dict(a=_flow(data=0))),
    ("dtype uint8", dict(a=_flow(dtype=_lib.FOTO_U8))),
    ("dtype 3", dict(a=_flow(dtype=3))),
    ("layout 2", dict(a=_flow(layout=2))),
    ("records 0", dict(a=_flow(records=0))),
    ("float64 at a 4-byte address", dict(a=_flow(data=PTR + 4, dtype=_lib.FOTO_F64))),
    ("w 1", dict(w=1)),
    ("h 1", dict(h=1)),
    ("w 0", dict(w=0)),
    ("h < 0", dict(h=-3)),
    ("w h = 2^31", dict(w=65536, h=32768)),
    ("bwd: null data", dict(b=_flow(data=0))),
    ("bwd: layout -1", dict(b=_flow(data=BWD, layout=-1))),
    ("bwd: 2 records for 3", dict(b=_flow(data=BWD, records=2))),
    ("bwd: 4 records for 3", dict(b=_flow(data=BWD, records=4))),
]


@pytest.mark.parametrize("name,kw", REJECTS)
def test_chain_check_rejects(name, kw):
    L = _lib.lib()
    args = dict(a=_flow(), b=None, w=W, h=H)
    args.update(kw)
    assert _check(**args) == ARG, name
    assert L.foto_last_error(), name
    # and the entries report the same before they touch a device
    a, b, w, h = _ref(args["a"]), _ref(args["b"]), args["w"], args["h"]
    if args["b"] is None:
        assert L.foto_flow_compose_dev(a, w, h, 0, ctypes.c_void_p(OUT), _lib.FOTO_F32, 0, None) == ARG, name
        assert L.foto_flow_invert_dev(a, w, h, 6, ctypes.c_void_p(OUT), _lib.FOTO_F32, 0, None) == ARG, name
    else:
        assert L.foto_flow_consistency_dev(a, b, w, h, 0.01, 0.5, ctypes.c_void_p(OUT), None, 0, ctypes.c_void_p(TABLE),
                                           None) == ARG, name


@pytest.mark.parametrize("name,kw", [
    ("null out", dict(out=0)),
    ("out_dtype uint8", dict(dtype=_lib.FOTO_U8)),
    ("out_dtype 3", dict(dtype=3)),
    ("out_layout 2", dict(layout=2)),
    ("float64 out at a 4-byte address", dict(out=OUT + 4, dtype=_lib.FOTO_F64)),
    ("float32 out at a 2-byte address", dict(out=OUT + 2)),
    ("iters 0", dict(iters=0)),
    ("iters 65", dict(iters=_lib.FOTO_INV_ITERS_MAX + 1)),
    ("last_only 2", dict(last_only=2)),
])
def test_flow_output_errors(name, kw):
    L = _lib.lib()
    a = dict(out=OUT, dtype=_lib.FOTO_F32, layout=0, iters=6, last_only=0)
    a.update(kw)
    fl = _flow()
    if "iters" not in kw:
        assert L.foto_flow_compose_dev(_ref(fl), W, H, a["last_only"], ctypes.c_void_p(a["out"]), a["dtype"], a["layout"],
                                       None) == ARG, name
    if "last_only" not in kw:
        assert L.foto_flow_invert_dev(_ref(fl), W, H, a["iters"], ctypes.c_void_p(a["out"]), a["dtype"], a["layout"],
                                      None) == ARG, name
    assert L.foto_last_error(), name


@pytest.mark.parametrize("name,kw", [
    ("null bwd", dict(bwd=None)),
    ("alpha1 < 0", dict(alpha1=-0.01)),
    ("alpha1 nan", dict(alpha1=math.nan)),
    ("alpha2 < 0", dict(alpha2=-1.0)),
    ("alpha2 inf", dict(alpha2=math.inf)),
    ("null valid", dict(valid=0)),
    ("null table", dict(table=0)),
    ("table at a 4-byte address", dict(table=TABLE + 4)),
    ("err_dtype uint8", dict(err=ERR, err_dtype=_lib.FOTO_U8)),
    ("float64 err at a 4-byte address", dict(err=ERR + 4, err_dtype=_lib.FOTO_F64)),
])
def test_consistency_argument_errors(name, kw):
    L = _lib.lib()
    a = dict(bwd=_flow(data=BWD), alpha1=0.01, alpha2=0.5, valid=OUT, err=0, err_dtype=_lib.FOTO_F32, table=TABLE)
    a.update(kw)
    assert L.foto_flow_consistency_dev(_ref(_flow()), _ref(a["bwd"]), W, H, a["alpha1"], a["alpha2"],
                                       ctypes.c_void_p(a["valid"]), ctypes.c_void_p(a["err"]), a["err_dtype"],
                                       ctypes.c_void_p(a["table"]), None) == ARG, name
    assert L.foto_last_error(), name


# ------------------------------------------------------------------ what Python sees

def test_defaults_and_header():
    assert (chain.INV_ITERS_DEFAULT, chain.INV_ITERS_MAX) == (_lib.FOTO_INV_ITERS_DEFAULT, _lib.FOTO_INV_ITERS_MAX) == (6, 64)
    assert (chain.ALPHA1, chain.ALPHA2) == (R.ALPHA1, R.ALPHA2) == (0.01, 0.5)
    assert len(chain.CLASSES) == 4
    import foto
    assert foto.compose is chain.compose and foto.invert is chain.invert and foto.consistency is chain.consistency
    from foto import device
    assert callable(device.bb_sequence)
    src = open(os.path.join(REPO, "include", "foto.h")).read()
    assert re.search(r"#define FOTO_CONSISTENCY_ALPHA1 0\.01\b", src) and re.search(r"#define FOTO_CONSISTENCY_ALPHA2 0\.5\b", src)
    for name in ("foto_chain_check", "foto_flow_compose_dev", "foto_flow_invert_dev", "foto_flow_consistency_dev"):
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert src.index("flow algebra") > src.index("scoring")


class Fake:
    """An object exposing a hand-written __cuda_array_interface__."""

    def __init__(self, shape, typestr, strides=None, ptr=PTR):
        self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(ptr, False), version=3,
                                             strides=strides)


def test_chain_value_errors():
    flow = Fake((3, 3, H, W), "<f4")
    with pytest.raises(ValueError):
        chain.compose(flow, in_layout="pairs")
    with pytest.raises(ValueError):
        chain.compose(flow, layout="pairs")
    with pytest.raises(ValueError):
        chain.compose(flow, dtype="uint8")
    with pytest.raises(ValueError):
        chain.compose(Fake((3, 3, 1, W), "<f4"))                                   # h < 2
    with pytest.raises(ValueError):
        chain.compose(flow, out=Fake((3, 3, H, W), "<f8", ptr=OUT))                 # out of another dtype
    with pytest.raises(ValueError):
        chain.compose(flow, last_only=True, out=Fake((3, 3, H, W), "<f4", ptr=OUT))  # one record expected
    with pytest.raises(ValueError):
        chain.invert(flow, iters=0)
    with pytest.raises(ValueError):
        chain.invert(flow, iters=65)
    with pytest.raises(ValueError):
        chain.invert(np.zeros((3, H, W)), out=Fake((3, H, W), "<f8", ptr=OUT))
    with pytest.raises(ValueError):
        chain.consistency(flow, Fake((2, 3, H, W), "<f4", ptr=BWD))                 # 2 records for 3
    with pytest.raises(ValueError):
        chain.consistency(flow, Fake((3, 3, H + 1, W), "<f4", ptr=BWD))
    with pytest.raises(ValueError):
        chain.consistency(flow, Fake((3, 3, H, W), "<f4", ptr=BWD), alpha1=-1.0)
    with pytest.raises(ValueError):
        chain.consistency(flow, Fake((3, 3, H, W), "<f4", ptr=BWD), alpha2=math.nan)
    with pytest.raises(TypeError):
        chain.consistency(np.zeros((3, H, W)), Fake((3, H, W), "<f8", ptr=BWD))      # host and device mixed


def test_cli_save_consistency_is_off_by_default():
    import main as M
    p = M.build_parser()
    assert p.parse_args(["a", "b"]).save_consistency is None
    assert p.parse_args(["a", "b", "--algo=foto", "--save-lum=l.png"]).save_consistency is None
    assert p.parse_args(["a", "b", "--save-consistency=c.png"]).save_consistency == "c.png"


# ------------------------------------------------------------------ the reference's own properties

def test_ref_integer_shifts_compose_to_their_sum():
    """Where the whole path stays inside the frame every sample falls on a pixel (fractions 0), so
    C_k is the sum of the first k + 1 shifts exactly."""
    h, w = 48, 64
    C = R.compose(R.shifts_flow(SHIFTS, h, w))
    run = np.cumsum(np.array(SHIFTS, dtype=np.float64), axis=0)
    x, y = R.grid(h, w)
    inside = np.ones((h, w), bool)
    for k in range(len(SHIFTS)):
        inside &= (x + run[k, 0] >= 0) & (x + run[k, 0] <= w - 1) & (y + run[k, 1] >= 0) & (y + run[k, 1] <= h - 1)
        assert np.all(C[k, 0][inside] == run[k, 0]) and np.all(C[k, 1][inside] == run[k, 1])
    assert np.count_nonzero(inside) > h * w // 2
    assert np.array_equal(R.compose(R.shifts_flow(SHIFTS, h, w), last_only=True)[0], C[-1])


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_ref_compose_of_one_record_is_the_identity(layout):
    f = R.random_flow(1, H, W, layout, np.float64, 5)
    f.reshape(-1)[7] = np.nan
    assert np.array_equal(R.compose(f, layout).view(np.uint64), f.view(np.uint64))
    assert np.array_equal(R.compose(f, layout, last_only=True).view(np.uint64), f.view(np.uint64))


def test_ref_gain_rule_and_nan_pocket():
    f = R.random_flow(3, H, W, "planar", np.float64, 6)
    C = R.compose(f)
    x, y = R.grid(H, W)
    g = (1 + f[0, 2]) * (1 + R.S(f[1, 2], x + C[0, 0], y + C[0, 1]))
    np.testing.assert_allclose(1 + C[1, 2], g, rtol=1e-15)
    assert np.all(R.compose(f, "planar", "interleaved") == np.moveaxis(C[:, :2], 1, -1))
    inter = np.ascontiguousarray(np.moveaxis(f[:, :2], 1, -1))
    Ci = R.compose(inter, "interleaved", "planar")
    assert np.array_equal(Ci[:, :2], C[:, :2]) and not np.any(Ci[:, 2]) and not np.any(np.signbit(Ci[:, 2]))
    # one NaN in record 1: record 0 is clean, records 1 and 2 are NaN where the path samples it, a few pixels
    g = f.copy()
    g[1, 0, 14, 18] = np.nan
    Cn = R.compose(g)
    bad = np.isnan(Cn[:, :2]).any(axis=1)
    assert not bad[0].any() and 0 < bad[1].sum() <= bad[2].sum() < 40
    assert np.array_equal(Cn[:, :2][~np.stack([bad, bad], 1)], C[:, :2][~np.stack([bad, bad], 1)])


def test_ref_contractive_inversion_meets_its_bound():
    """|J F| < 0.4 on the smooth flow and |F| < 2: sixteen rounds leave at most 0.4^16 * 2 = 9e-7,
    so 1e-6 is the bound -- derived, and met by numpy here before the device is asked."""
    F = R.smooth_flow()
    x, y = R.grid(48, 64)
    ux, uy = 1.5 / 8, 1.5 / 10     # the largest partial derivatives
    vx, vy = 1 / 9, 1 / 7
    assert math.hypot(math.hypot(ux, uy), math.hypot(vx, vy)) < 0.4          # Frobenius >= spectral norm
    assert 0.4 ** 16 * 2 < 1e-6
    res = [R.inversion_residual(F, R.invert(F, it)) for it in (1, 6, 16)]
    assert res[2] <= 1e-6 and res[0] > res[1] > res[2], res


@pytest.mark.parametrize("w,h,K,seed", CONS)
def test_ref_consistency_cases_are_clear_of_the_threshold(w, h, K, seed):
    for dtype in (np.float64, np.float32):
        for kb in (None, 1):
            f, b = R.cons_case(K, h, w, seed, dtype=dtype, bwd_records=kb)
            valid, table, err, cls, margin = R.consistency(f, b)
            assert margin.min() > 1e-9, margin.min()
            assert np.all(table.sum(axis=1) == w * h)
            assert np.array_equal(np.isnan(err), cls == 3) and table[0, 3] >= 1
            if w * h > 1000:
                assert np.all(table.sum(axis=0) > 0), table     # every class occurs
            assert R.consistency(f, b, alpha1=0.0, alpha2=0.125)[4].min() > 1e-9


def test_ref_consistency_mixed_dtypes_and_layouts():
    w, h, K, seed = CONS[2]
    combos = [(d, l) for d in (np.float32, np.float64) for l in ("planar", "interleaved")]
    for df, lf in combos:
        for db, lb in combos:
            f, b = R.cons_case(K, h, w, seed, layout=lf, dtype=df, bwd_layout=lb, bwd_dtype=db)
            assert (f.dtype, b.dtype) == (df, db) and f.shape[-1] == (w if lf == "planar" else 2)
            _, table, _, _, margin = R.consistency(f, b, lf, lb)
            assert margin.min() > 1e-9 and np.all(table.sum(axis=0) > 0)
    f, b = R.cons_case(1, 29, 37, 21)     # the case the GPU test pokes +-inf into
    assert R.consistency(f, b)[4].min() > 1e-9


def test_ref_maps_a_planes_are_the_backward_flow():
    """main.py --save-consistency takes the a-planes of maps at s = Nt - 1 as they are: they hold
    a - p, where the frame-1 pixel came from, which is B of F(p) + B(p + F(p)) = 0; negated they fail."""
    import interp_ref as I
    Nt, Ny, Nx = 6, 24, 32
    phi = I.smooth_phi(Nt, Ny, Nx, dv=0.6)
    fwd, bwd = I.maps(phi, 0.0)[2:], I.maps(phi, Nt - 1.0)[:2]
    z = np.zeros((1, Ny, Nx))
    F = np.concatenate([fwd, z])[None]
    assert np.abs(fwd).max() > 1.0
    assert R.consistency(F, np.concatenate([bwd, z])[None])[1][0, 0] == Ny * Nx
    assert R.consistency(F, np.concatenate([-bwd, z])[None])[1][0, 1] > Ny * Nx // 2


def test_ref_smooth_and_step_flows():
    F = R.smooth_flow()
    _, table, _, cls, margin = R.consistency(F, R.invert(F, 16))
    assert table[0, 1] == 0 and table[0, 3] == 0 and table[0, 0] > 0.9 * 64 * 48 and margin.min() > 1e-9
    fwd, bwd = R.step_flow()
    _, table, _, cls, margin = R.consistency(fwd, bwd)
    cols = np.unique(np.nonzero(cls[0] == 1)[1])
    assert list(cols) == [29, 30, 31, 32, 33, 34] and table[0, 1] == 6 * 48 and margin.min() > 1e-9
