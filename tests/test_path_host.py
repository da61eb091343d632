"""Transport-path exports, the parts that need no GPU: the target validation of
foto.device.frames_target / path_target on hand-written __cuda_array_interface__ mappings
(ValueError before the library is touched), the K -> np.linspace(0, Nt - 1, K) expansion of the
frame positions, and the ctypes prototypes of the new header symbols."""
import ctypes

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the package on sys.path)

from foto import _lib
from foto import device as D
from test_cabi import header_functions

NEW = ["foto_bb_frames", "foto_bb_frames_dev", "foto_bb_flow_path", "foto_bb_flow_path_dev",
       "foto_flow_path_from_phi"]

H, W, NT = 29, 37, 5


def arr(shape, typestr, strides=None):
    """A device array described by hand (never dereferenced: validation only)."""
    return {"ptr": 0x10000, "typestr": typestr, "shape": tuple(shape), "strides": strides}


def test_frames_target_accepts():
    out = arr((3, H, W), "<f4")
    got, ptr, code = D.frames_target(out, "float32", 3, H, W)
    assert got is out and ptr == 0x10000 and code == _lib.FOTO_F32
    assert D.frames_target(arr((3, H, W), "|u1"), "uint8", 3, H, W)[2] == _lib.FOTO_U8
    assert D.frames_target(arr((3, H, W), "<f8"), np.float64, 3, H, W)[2] == _lib.FOTO_F64
    # explicit C-contiguous strides are fine
    assert D.frames_target(arr((3, H, W), "<f4", (H * W * 4, W * 4, 4)), "float32", 3, H, W)[1] == 0x10000


@pytest.mark.parametrize("name,out,dtype", [
    ("one frame short", arr((2, H, W), "<f4"), "float32"),
    ("transposed frame", arr((3, W, H), "<f4"), "float32"),
    ("flat", arr((3, H * W), "<f4"), "float32"),
    ("float64 array for a float32 export", arr((3, H, W), "<f8"), "float32"),
    ("uint8 array for a float32 export", arr((3, H, W), "|u1"), "float32"),
    ("row-padded", arr((3, H, W), "<f4", (H * 40 * 4, 40 * 4, 4)), "float32"),
    ("every other column", arr((3, H, W), "<f4", (H * W * 8, W * 8, 8)), "float32"),
    ("int16 frames", arr((3, H, W), "<i2"), "int16"),
    ("float16 frames", arr((3, H, W), "<f2"), "float16"),
])
def test_frames_target_rejects(name, out, dtype):
    with pytest.raises(ValueError):
        D.frames_target(out, dtype, 3, H, W)


def test_path_target_accepts():
    out = arr((NT - 1, 3, H, W), "<f8")
    got, ptr, code, layout = D.path_target(out, "float64", "planar", NT, H, W)
    assert got is out and ptr == 0x10000 and (code, layout) == (_lib.FOTO_F64, 0)
    assert D.path_target(arr((NT - 1, H, W, 2), "<f4"), "float32", "interleaved", NT, H, W)[2:] == (_lib.FOTO_F32, 1)


@pytest.mark.parametrize("name,out,dtype,layout", [
    ("Nt records instead of Nt - 1", arr((NT, 3, H, W), "<f8"), "float64", "planar"),
    ("one record's shape", arr((3, H, W), "<f8"), "float64", "planar"),
    ("planar target for interleaved", arr((NT - 1, 3, H, W), "<f4"), "float32", "interleaved"),
    ("interleaved target for planar", arr((NT - 1, H, W, 2), "<f4"), "float32", "planar"),
    ("float32 array for float64", arr((NT - 1, 3, H, W), "<f4"), "float64", "planar"),
    ("uint8 records", arr((NT - 1, 3, H, W), "|u1"), "uint8", "planar"),
    ("unknown layout", arr((NT - 1, 3, H, W), "<f4"), "float32", "chw"),
    ("padded records", arr((NT - 1, 3, H, W), "<f4", (4 * H * W * 4, H * W * 4, W * 4, 4)), "float32", "planar"),
])
def test_path_target_rejects(name, out, dtype, layout):
    with pytest.raises(ValueError):
        D.path_target(out, dtype, layout, NT, H, W)


def test_frame_positions():
    for Nt, K in ((5, 5), (6, 3), (32, 31), (2, 7), (9, 1)):
        got = D.frame_positions(K, Nt)
        assert got.dtype == np.float64 and np.array_equal(got, np.linspace(0, Nt - 1, K))
        assert got[0] == 0.0 and (K == 1 or got[-1] == Nt - 1)
    assert np.array_equal(D.frame_positions(np.int64(4), 7), np.linspace(0, 6, 4))
    got = D.frame_positions([0, 1.5, 4], 5)
    assert got.dtype == np.float64 and got.flags.c_contiguous and got.tolist() == [0.0, 1.5, 4.0]
    assert D.frame_positions(np.arange(6)[::2], 6).tolist() == [0.0, 2.0, 4.0]
    assert D.frame_positions((), 5).shape == (0,)      # (count 0: the library's FOTO_ERR_ARG)
    for bad in (0, -3, 2.5, [[0, 1], [2, 3]], np.zeros((2, 1))):
        with pytest.raises(ValueError):
            D.frame_positions(bad, 5)


def test_new_symbols_have_prototypes():
    names = header_functions()
    for n in NEW:
        assert n in names, n
        assert n in _lib.SIGNATURES, n
    L = _lib.lib()
    P, Dp, I = ctypes.c_void_p, _lib._D, ctypes.c_int
    want = {
        "foto_bb_frames": [P, Dp, I, ctypes.c_double, Dp],
        "foto_bb_frames_dev": [P, Dp, I, ctypes.c_double, P, I, P],
        "foto_bb_flow_path": [P, Dp, Dp, Dp],
        "foto_bb_flow_path_dev": [P, P, I, I, P],
        "foto_flow_path_from_phi": [Dp, I, I, I, Dp, Dp, Dp],
    }
    for n, args in want.items():
        fn = getattr(L, n)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == args, n


def test_solver_and_module_members():
    from foto import ops
    from foto.bb import BBSolver
    for m in ("frames", "frames_device", "flow_path", "flow_path_device"):
        assert callable(getattr(BBSolver, m))
    assert callable(D.bb_path) and callable(ops.flow_path_from_phi)


def test_null_context_is_an_argument_error():
    """The entries check their arguments before they touch a device."""
    L = _lib.lib()
    z = np.zeros(4)
    assert L.foto_bb_frames(None, _lib.dptr(z), 1, 1.0, _lib.dptr(z)) == _lib.FOTO_ERR_ARG
    assert L.foto_bb_frames_dev(None, _lib.dptr(z), 1, 1.0, None, _lib.FOTO_F32, None) == _lib.FOTO_ERR_ARG
    assert L.foto_bb_flow_path(None, _lib.dptr(z), _lib.dptr(z), _lib.dptr(z)) == _lib.FOTO_ERR_ARG
    assert L.foto_bb_flow_path_dev(None, None, _lib.FOTO_F32, 0, None) == _lib.FOTO_ERR_ARG
    assert L.foto_flow_path_from_phi(_lib.dptr(z), 1, 2, 2, _lib.dptr(z), _lib.dptr(z), _lib.dptr(z)) == _lib.FOTO_ERR_ARG
