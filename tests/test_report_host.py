"""CPU checks of the transport report's host side (include/foto.h: foto_bb_report / _dev,
foto_report_from_state; foto.report.TransportReport; foto.device.report_target): the boundary,
the target validation, the derived values, and the argument errors that need no device."""
import math
import os
import re

import numpy as np
import pytest

from conftest import REPO

from foto import _lib, device, ops  # noqa: E402
from foto import report as R  # noqa: E402

HEADER = os.path.join(REPO, "include", "foto.h")
COLS = ["MASS", "KINETIC", "VACUUM", "CONT", "HJ_NUM", "HJ_DEN", "DUAL", "DIST_T"]
PTR = 0x7F0000000000   # never dereferenced: these calls stop before the library


def header_macros():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(FOTO_REPORT_\w+)\s+(\d+)\s*$", src, re.M)}


def test_header_symbols_and_prototypes():
    import test_cabi
    names = test_cabi.header_functions()
    L = _lib.lib()
    for fn in ("foto_bb_report", "foto_bb_report_dev", "foto_report_from_state"):
        assert fn in names and fn in _lib.SIGNATURES and hasattr(L, fn)
        assert getattr(L, fn).argtypes == _lib.SIGNATURES[fn][1]
    macros = header_macros()
    assert "FOTO_REPORT_COLS" in macros and "FOTO_REPORT_MASS" in macros   # the table's width and its first column


def test_column_indices():
    macros = header_macros()
    assert macros.pop("FOTO_REPORT_COLS") == 8 == R.REPORT_COLS
    assert macros == {"FOTO_REPORT_" + c: i for i, c in enumerate(COLS)}
    assert R.COLUMNS == {c: i for i, c in enumerate(COLS)}
    assert [getattr(R, c) for c in COLS] == list(range(8))


class Fake:
    def __init__(self, shape, typestr, strides=None, ptr=PTR):
        self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(ptr, False), version=3,
                                             strides=strides)


def test_report_target_accepts():
    for good in (Fake((6, 8), "<f8"), Fake((6, 8), "<f8", strides=(64, 8))):
        out, ptr = device.report_target(good, 6)
        assert out is good and ptr == PTR


@pytest.mark.parametrize("name,bad", [
    ("wrong shape", Fake((5, 8), "<f8")),
    ("one axis", Fake((48,), "<f8")),
    ("float32", Fake((6, 8), "<f4")),
    ("transposed", Fake((8, 6), "<f8", strides=(8, 64))),
    ("transposed square", None),
    ("padded", Fake((6, 8), "<f8", strides=(80, 8))),
])
def test_report_target_rejects(name, bad):
    Nt = 6
    if bad is None:   # the transpose of an (8, 8) table has the right shape and the wrong strides
        bad, Nt = Fake((8, 8), "<f8", strides=(8, 64)), 8
    with pytest.raises(ValueError):
        device.report_target(bad, Nt)


# a hand-written table: 4 planes; sum DUAL = -1.5 < 0
TABLE = np.array([
    # MASS  KINETIC VACUUM CONT   HJ_NUM HJ_DEN DUAL  DIST_T
    [10.0,  2.0,    0.0,   0.25,  1.0,   4.0,   -7.5,  9.0],
    [10.5,  4.0,    0.5,   1.0,   2.0,   6.0,   0.0,   4.0],
    [9.75,  3.0,    0.0,   0.5,   0.5,   5.0,   0.0,   1.0],
    [10.0,  1.0,    0.25,  0.5,   0.5,   1.0,   6.0,   0.0],
])


def test_derived_values():
    Nt, Nx, Ny = 4, 5, 3
    rep = R.TransportReport(TABLE, Nt, Nx, Ny)
    assert rep.table.shape == (4, 8) and rep.table.dtype == np.float64 and (rep.Nt, rep.Nx, rep.Ny) == (4, 5, 3)
    for i, c in enumerate(COLS):
        v = getattr(rep, c.lower())
        assert v.shape == (4,) and np.array_equal(v, TABLE[:, i]) and np.shares_memory(v, rep.table)
    assert rep.crit == math.sqrt(4.0 / (16.0 + 1e-10))
    assert rep.action == 0.5 * 2.0 + 4.0 + 3.0 + 0.5 * 1.0 == 8.5
    assert rep.action_dual == -1.5
    assert rep.w2 == math.sqrt(2.0 * 3 * 8.5)
    assert math.isnan(rep.w2_dual)
    np.testing.assert_array_equal(rep.ie, 255.0 * np.sqrt(np.array([9.0, 4.0, 1.0, 0.0]) / 15.0))
    assert rep.continuity == math.sqrt(2.25) == 1.5
    assert rep.mass_drift == 10.5 - 9.75
    # a non-negative dual sum has a root
    t2 = TABLE.copy()
    t2[3, R.DUAL] = 9.5
    assert R.TransportReport(t2, Nt, Nx, Ny).w2_dual == math.sqrt(2.0 * 3 * 2.0)
    assert "TransportReport(Nt=4" in repr(rep)


def test_report_is_immutable():
    src = TABLE.copy()
    rep = R.TransportReport(src, 4, 5, 3)
    src[0, 0] = -1.0                       # the record holds its own copy
    assert rep.table[0, 0] == 10.0
    with pytest.raises(ValueError):
        rep.table[0, 0] = 1.0
    with pytest.raises(ValueError):
        rep.mass[0] = 1.0
    with pytest.raises(AttributeError):
        rep.Nt = 5
    with pytest.raises(AttributeError):
        rep.extra = 1
    with pytest.raises(ValueError):
        R.TransportReport(TABLE, 5, 5, 3)


def test_from_state_argument_errors_without_gpu():
    """A null pointer and Nt = 1 are refused before any device is touched: FOTO_ERR_ARG on a
    machine without a GPU as well."""
    L = _lib.lib()
    Nt, Nx, Ny = 3, 4, 2
    N = Nt * Nx * Ny
    mu, phi, r0, rT, out = np.zeros(3 * N), np.zeros(N), np.zeros(Nx * Ny), np.zeros(Nx * Ny), np.full((Nt, 8), 7.25)
    null = _lib._D()
    args = [_lib.dptr(mu), _lib.dptr(phi), _lib.dptr(r0), _lib.dptr(rT)]
    for k in range(4):
        a = list(args)
        a[k] = null
        assert L.foto_report_from_state(*a, Nt, Nx, Ny, _lib.dptr(out)) == _lib.FOTO_ERR_ARG
    assert L.foto_report_from_state(*args, Nt, Nx, Ny, null) == _lib.FOTO_ERR_ARG
    for shape in ((1, Nx, Ny), (0, Nx, Ny), (Nt, 0, Ny), (Nt, Nx, 0), (Nt, -1, Ny)):
        assert L.foto_report_from_state(*args, *shape, _lib.dptr(out)) == _lib.FOTO_ERR_ARG
    assert b"foto_report_from_state" in L.foto_last_error()
    assert (out == 7.25).all()
    with pytest.raises(_lib.FotoError):
        ops.report_from_state(mu[:3 * Nx * Ny], phi[:Nx * Ny], r0, rT, 1, Nx, Ny)
    # the context entries refuse a null context the same way
    assert L.foto_bb_report(None, _lib.dptr(out)) == _lib.FOTO_ERR_ARG
    assert L.foto_bb_report_dev(None, None, None) == _lib.FOTO_ERR_ARG
