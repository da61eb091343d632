"""Point tracking, the parts that need no GPU: the target and point validation of
foto.device.track_target / track_points / track_source on hand-written __cuda_array_interface__
mappings (ValueError before the library is touched), the ctypes prototypes of the three new
header symbols, and the argument errors of foto_track_from_phi, which come before any device is
touched."""
import ctypes

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the package on sys.path)

from foto import _lib
from foto import device as D
from test_cabi import header_functions

NEW = ["foto_bb_track", "foto_bb_track_dev", "foto_track_from_phi"]

R, M = 4, 300


def arr(shape, typestr, strides=None):
    """A device array described by hand (never dereferenced: validation only)."""
    return {"ptr": 0x10000, "typestr": typestr, "shape": tuple(shape), "strides": strides}


def test_track_target_accepts():
    out = arr((R, M, 2), "<f4")
    got, ptr, code = D.track_target(out, "float32", R, M)
    assert got is out and ptr == 0x10000 and code == _lib.FOTO_F32
    assert D.track_target(arr((R, M, 2), "<f8"), np.float64, R, M)[2] == _lib.FOTO_F64
    assert D.track_target(arr((1, M, 2), "<f8"), "float64", 1, M)[1] == 0x10000
    # explicit C-contiguous strides are fine
    assert D.track_target(arr((R, M, 2), "<f4", (M * 8, 8, 4)), "float32", R, M)[1] == 0x10000


@pytest.mark.parametrize("name,out,dtype", [
    ("wrong R", arr((R - 1, M, 2), "<f4"), "float32"),
    ("the last record only", arr((1, M, 2), "<f4"), "float32"),
    ("wrong M", arr((R, M + 1, 2), "<f4"), "float32"),
    ("(M, 3)", arr((R, M, 3), "<f4"), "float32"),
    ("no record axis", arr((M, 2), "<f4"), "float32"),
    ("float64 array for a float32 export", arr((R, M, 2), "<f8"), "float32"),
    ("float32 array for a float64 export", arr((R, M, 2), "<f4"), "float64"),
    ("padded records", arr((R, M, 2), "<f4", ((M + 4) * 8, 8, 4)), "float32"),
    ("padded points", arr((R, M, 2), "<f4", (M * 16, 16, 4)), "float32"),
    ("uint8 records", arr((R, M, 2), "|u1"), "uint8"),
    ("float16 records", arr((R, M, 2), "<f2"), "float16"),
])
def test_track_target_rejects(name, out, dtype):
    with pytest.raises(ValueError):
        D.track_target(out, dtype, R, M)


def test_single_point_is_promoted():
    p = D.track_points((3.5, -1.25))
    assert p.shape == (1, 2) and p.dtype == np.float64 and p.tolist() == [[3.5, -1.25]]
    p = D.track_points(np.array([1, 2], dtype=np.int32))
    assert p.shape == (1, 2) and p.dtype == np.float64
    q = D.track_points([[0, 1], [2, 3], [4, 5]])
    assert q.shape == (3, 2) and q.dtype == np.float64 and q.flags.c_contiguous
    q = D.track_points(np.arange(12, dtype=np.float32).reshape(2, 6)[:, ::3])   # a strided view
    assert q.flags.c_contiguous and q.tolist() == [[0.0, 3.0], [6.0, 9.0]]
    assert D.track_points(np.zeros((2, 2))).shape == (2, 2)                     # (2, 2) is two points
    assert D.track_points(np.zeros((0, 2))).shape == (0, 2)                     # (M = 0: the library's FOTO_ERR_ARG)


@pytest.mark.parametrize("bad", [np.zeros(3), np.zeros((4, 3)), np.zeros((2, 4)), np.zeros((2, 2, 2)), 1.5,
                                 np.zeros((2, 1)), []])
def test_points_of_the_wrong_shape(bad):
    with pytest.raises(ValueError):
        D.track_points(bad)


def test_device_points():
    assert D.track_source(arr((M, 2), "<f4")) == (0x10000, _lib.FOTO_F32, M)
    assert D.track_source(arr((M, 2), "<f8", (16, 8))) == (0x10000, _lib.FOTO_F64, M)
    for bad in (arr((M, 3), "<f4"), arr((2,), "<f8"), arr((M, 2), "|u1"), arr((M, 2), "<f2"), arr((M, 2), "<i4"),
                arr((M, 2), "<f4", (16, 4)), arr((M, 2), "<f8", (16, 16)), arr((1, M, 2), "<f4")):
        with pytest.raises(ValueError):
            D.track_source(bad)
    with pytest.raises(TypeError):
        D.track_source(np.zeros((M, 2)))        # a host array has no __cuda_array_interface__


def test_new_symbols_have_prototypes():
    names = header_functions()
    for n in NEW:
        assert n in names, n
        assert n in _lib.SIGNATURES, n
    L = _lib.lib()
    P, Dp, I, I64 = ctypes.c_void_p, _lib._D, ctypes.c_int, ctypes.c_int64
    want = {
        "foto_bb_track": [P, Dp, I64, I, Dp],
        "foto_bb_track_dev": [P, P, I, I64, I, P, I, P],
        "foto_track_from_phi": [Dp, I, I, I, Dp, I64, I, Dp],
    }
    for n, args in want.items():
        fn = getattr(L, n)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == args, n


def test_solver_and_module_members():
    from foto import ops
    from foto.bb import BBSolver
    for m in ("track", "track_device"):
        assert callable(getattr(BBSolver, m))
    assert callable(D.bb_track) and callable(D.track_target) and callable(ops.track_from_phi)


def test_argument_errors_without_gpu():
    """foto_track_from_phi checks its arguments before it touches a device (as
    test_solve_ex_argument_errors_without_gpu), and the context entries a null context."""
    L = _lib.lib()
    E = _lib.FOTO_ERR_ARG
    phi = np.zeros(2 * 3 * 4)
    pts = np.zeros((5, 2))
    out = np.full((1, 5, 2), 7.25)
    null = _lib._D()
    d = _lib.dptr
    assert L.foto_track_from_phi(d(phi), 2, 4, 3, d(pts), 0, 1, d(out)) == E             # M = 0
    assert L.foto_track_from_phi(d(phi), 2, 4, 3, d(pts), -1, 1, d(out)) == E
    assert L.foto_track_from_phi(d(phi), 2, 4, 3, d(pts), 2 ** 31, 1, d(out)) == E       # M > 2^31 - 1
    assert L.foto_track_from_phi(d(phi), 1, 4, 3, d(pts), 5, 1, d(out)) == E             # Nt = 1
    assert L.foto_track_from_phi(d(phi), 2, 4, 3, null, 5, 1, d(out)) == E               # null pts
    assert L.foto_track_from_phi(d(phi), 2, 4, 3, d(pts), 5, 1, null) == E
    assert L.foto_track_from_phi(null, 2, 4, 3, d(pts), 5, 1, d(out)) == E
    assert L.foto_track_from_phi(d(phi), 2, 4, 3, d(pts), 5, 2, d(out)) == E             # all_steps = 2
    assert L.foto_track_from_phi(d(phi), 2, 4, 3, d(pts), 5, -1, d(out)) == E
    assert L.foto_track_from_phi(d(phi), 2, 1, 3, d(pts), 5, 1, d(out)) == E             # Nx = 1
    assert np.all(out == 7.25)
    assert L.foto_bb_track(None, d(pts), 5, 1, d(out)) == E
    assert L.foto_bb_track_dev(None, None, _lib.FOTO_F64, 5, 1, None, _lib.FOTO_F64, None) == E
    with pytest.raises(ValueError):
        from foto import ops
        ops.track_from_phi(phi, 2, 4, 3, np.zeros((5, 3)))
