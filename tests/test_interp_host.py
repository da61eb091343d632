"""Maps and in-betweens, the parts that need no GPU: the properties of the numpy restatement
(tests/interp_ref.py) that the GPU tests rely on, on the seeded inputs they share; the header,
export and ctypes prototypes of the five new symbols; the argument errors that come before any
device is touched; the target validation of foto.device; main.py's two new flags."""
import ctypes

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the package on sys.path)

import interp_ref as R
from foto import _lib
from foto import device as D
from test_cabi import header_functions

NEW = ["foto_bb_maps", "foto_bb_maps_dev", "foto_bb_interp_dev", "foto_maps_from_phi", "foto_interp_from_phi"]

# the GPU parity shapes (Nx, Ny, Nt) and the times of one of them
SHAPES = [(2, 2, 2), (3, 2, 2), (5, 4, 3), (67, 19, 5)]


def times(Nt):
    t = [0.0, 2.0 ** -40, 0.5, float(Nt - 1) - 2.0 ** -20, float(Nt - 1)]
    if Nt > 2:
        t.insert(3, float((Nt - 1) // 2))     # an integer interior time
    return t


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------ the restatement's own properties

@pytest.mark.parametrize("Nx,Ny,Nt", SHAPES)
def test_seeded_phi_is_smooth(Nx, Ny, Nt):
    """low-pass, and max |dV| per pixel < 0.5: theta V is a contraction for every theta <= 1"""
    phi = R.smooth_phi(Nt, Ny, Nx, seed=Nx)
    dv = R.max_dv(phi)
    print(f"{Nx}x{Ny}x{Nt}: max |dV| per pixel {dv:.3f}, max |V| {max(np.abs(f).max() for f in R.node_velocity(phi)):.3f}")
    assert dv < 0.5
    if min(Nx, Ny) > 2:
        assert dv > 0.25      # (scaled to 0.3: the maps are not trivial)


def test_residual_shrinks_with_inv_iters():
    """|z + theta V(z) - p| of the inverse step falls with the round count, by about the Lipschitz
    constant of theta V per round, down to rounding."""
    Nx, Ny, Nt = 67, 19, 5
    phi = R.smooth_phi(Nt, Ny, Nx, seed=Nx)
    y, x = np.meshgrid(np.arange(Ny, dtype=np.float64), np.arange(Nx, dtype=np.float64), indexing="ij")
    res = []
    for it in (1, 2, 4, 6, 8, 16):
        zx, zy = R.inv(phi[1], 1.0, it, x, y)
        fx, fy = R.step(phi[1], zx, zy)
        res.append(float(np.hypot(fx - x, fy - y).max()))
    print("inverse-step residual by rounds 1, 2, 4, 6, 8, 16:", " ".join(f"{r:.2e}" for r in res))
    assert all(b < a for a, b in zip(res[:4], res[1:5]))
    assert res[3] < 1e-2 * res[0] and res[-1] < 1e-9


@pytest.mark.parametrize("Nx,Ny,Nt", SHAPES)
def test_end_times_are_exact(Nx, Ny, Nt):
    phi = R.smooth_phi(Nt, Ny, Nx, seed=Nx)
    zero = np.zeros((Ny, Nx))
    m0, m1 = R.maps(phi, 0.0), R.maps(phi, float(Nt - 1))
    assert same(m0[0], zero) and same(m0[1], zero)           # a = p: +0.0, not -0.0
    assert same(m1[2], zero) and same(m1[3], zero)
    # the b-planes at s = 0 are the forward flow: Nt - 1 steps from the pixel centres
    y, x = np.meshgrid(np.arange(Ny, dtype=np.float64), np.arange(Nx, dtype=np.float64), indexing="ij")
    bx, by = x, y
    for n in range(Nt - 1):
        bx, by = R.step(phi[n], bx, by)
    assert same(m0[2], bx - x) and same(m0[3], by - y)
    # forward after backward closes to the inverse's residual: a at s = Nt-1, pushed through every step
    ax, ay = x + m1[0], y + m1[1]
    for n in range(Nt - 1):
        ax, ay = R.step(phi[n], ax, ay)
    assert np.hypot(ax - x, ay - y).max() < 1e-3


@pytest.mark.parametrize("C", [None, 3])
def test_end_frames_come_back(C):
    Nx, Ny, Nt = 67, 19, 5
    phi = R.smooth_phi(Nt, Ny, Nx, seed=Nx)
    f0, f1 = R.smooth_frames(Ny, Nx, C)
    assert same(R.interp(phi, f0, f1, 0.0), f0) and same(R.interp(phi, f0, f1, float(Nt - 1)), f1)
    u0, u1 = R.u8_frames(Ny, Nx, C)
    assert same(R.to_u8(R.interp(phi, u0, u1, 0.0, divisor=255.0)), u0)
    assert same(R.to_u8(R.interp(phi, u0, u1, float(Nt - 1), divisor=255.0)), u1)


def test_seeded_u8_reference_is_unambiguous():
    """The 8-bit parity test may skip pixels whose 255 x + 0.5 lies within 1e-9 of an integer; on
    the seeded inputs the reference alone keeps them under 1e-4 of all pixels."""
    Nx, Ny, Nt = 67, 19, 5
    phi = R.smooth_phi(Nt, Ny, Nx, seed=Nx)
    u0, u1 = R.u8_frames(Ny, Nx, 3)
    amb = tot = 0
    for s in times(Nt):
        for it in (1, 6):
            x = R.interp(phi, u0, u1, s, it, divisor=255.0)
            amb += int(R.u8_ambiguous(x).sum())
            tot += x.size
    print(f"{amb} of {tot} reference pixels within 1e-9 of an 8-bit rounding boundary")
    assert amb <= 1e-4 * tot


def test_inbetween_beats_crossfade_on_an_exact_translation():
    """phi = (dx x + dy y) / (Nt - 1) on every plane moves every interior pixel by (dx, dy): the
    in-between of a shifted blob is then the shifted blob up to bilinear sampling, the cross-fade
    is two ghosts."""
    Nx, Ny, Nt = 32, 24, 6
    dx, dy = 3.0, 1.5
    y, x = np.meshgrid(np.arange(Ny, dtype=np.float64), np.arange(Nx, dtype=np.float64), indexing="ij")
    phi = np.repeat(((dx * x + dy * y) / (Nt - 1))[None], Nt, axis=0)
    f0, f1, between = R.blob_pair(Ny, Nx, (dx, dy))
    for s in (1.25, 2.5, 3.75):
        w = s / (Nt - 1)
        got = R.interp(phi, f0, f1, s)
        fade = (1 - w) * f0 + w * f1
        e_i = np.sqrt(np.mean((got - between(w)) ** 2))
        e_f = np.sqrt(np.mean((fade - between(w)) ** 2))
        print(f"s = {s}: in-between RMS {255 * e_i:.2f} grey levels, cross-fade {255 * e_f:.2f}")
        assert e_i < e_f


# ------------------------------------------------------------------ header, exports, prototypes

def test_new_symbols_have_prototypes():
    names = header_functions()
    for n in NEW:
        assert n in names, n
        assert n in _lib.SIGNATURES, n
    L = _lib.lib()
    P, Dp, I, I64, Im = ctypes.c_void_p, _lib._D, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(_lib.Image)
    want = {
        "foto_bb_maps": [P, Dp, I, I, Dp],
        "foto_bb_maps_dev": [P, Dp, I, I, P, I, P],
        "foto_bb_interp_dev": [P, Im, Im, I, I64, I64, Dp, I, I, P, I, P],
        "foto_maps_from_phi": [Dp, I, I, I, Dp, I, I, Dp],
        "foto_interp_from_phi": [Dp, I, I, I, Dp, Dp, I, Dp, I, I, Dp],
    }
    for n, args in want.items():
        fn = getattr(L, n)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == args, n


def test_header_constants():
    src = open(REPO + "/include/foto.h").read()
    assert "#define FOTO_INV_ITERS_MAX 64" in src and "#define FOTO_INV_ITERS_DEFAULT 6" in src
    assert (_lib.FOTO_INV_ITERS_MAX, _lib.FOTO_INV_ITERS_DEFAULT) == (64, 6)


def test_solver_and_module_members():
    import inspect
    from foto import ops
    from foto.bb import BBSolver
    for m in ("maps", "maps_device", "interpolate"):
        assert callable(getattr(BBSolver, m))
        assert inspect.signature(getattr(BBSolver, m)).parameters["inv_iters"].default == 6
    assert callable(D.bb_interpolate) and callable(ops.maps_from_phi) and callable(ops.interp_from_phi)


def test_argument_errors_without_gpu():
    """The *_from_phi entries check their arguments before they touch a device, and the context
    entries a null context."""
    L = _lib.lib()
    E = _lib.FOTO_ERR_ARG
    Nt, Nx, Ny = 3, 4, 3
    phi = np.zeros(Nt * Nx * Ny)
    s = np.array([0.0, 1.5])
    out = np.full((2, 4, Ny, Nx), 7.25)
    f = np.zeros((Ny, Nx, 2))
    img = np.full((2, Ny, Nx, 2), 7.25)
    null = _lib._D()
    d = _lib.dptr

    def maps(phi_=None, Nt_=Nt, Nx_=Nx, Ny_=Ny, s_=None, count=2, it=6, out_=None):
        return L.foto_maps_from_phi(d(phi) if phi_ is None else phi_, Nt_, Nx_, Ny_, d(s) if s_ is None else s_,
                                    count, it, d(out) if out_ is None else out_)

    def interp(phi_=None, Nx_=Nx, Ny_=Ny, f0=None, f1=None, C=2, s_=None, count=2, it=6, out_=None):
        return L.foto_interp_from_phi(d(phi) if phi_ is None else phi_, Nt, Nx_, Ny_, d(f) if f0 is None else f0,
                                      d(f) if f1 is None else f1, C, d(s) if s_ is None else s_, count, it,
                                      d(img) if out_ is None else out_)

    for bad in (np.array([0.0, -1e-300]), np.array([0.0, 2.0 + 1e-12]), np.array([np.nan, 1.0]),
                np.array([1.0, np.inf]), np.array([-np.inf, 1.0])):
        assert maps(s_=d(bad)) == E and interp(s_=d(bad)) == E
    for kw in (dict(phi_=null), dict(s_=null), dict(out_=null), dict(count=0), dict(count=-3), dict(it=0),
               dict(it=65), dict(it=-1), dict(Nx_=1), dict(Ny_=1)):
        assert maps(**kw) == E, kw
        assert interp(**kw) == E, kw
    assert maps(Nt_=1) == E
    for kw in (dict(f0=null), dict(f1=null), dict(C=0), dict(C=-1)):
        assert interp(**kw) == E, kw
    assert np.all(out == 7.25) and np.all(img == 7.25)
    z = np.zeros(4)
    assert L.foto_bb_maps(None, d(z), 1, 6, d(z)) == E
    assert L.foto_bb_maps_dev(None, d(z), 1, 6, None, _lib.FOTO_F64, None) == E
    im = _lib.Image(0x10000, _lib.FOTO_F64, 4, 1, 1.0)
    assert L.foto_bb_interp_dev(None, ctypes.byref(im), ctypes.byref(im), 1, 1, 1, d(z), 1, 6, None, _lib.FOTO_F64,
                                None) == E
    assert L.foto_last_error()


# ------------------------------------------------------------------ target validation

def arr(shape, typestr, strides=None):
    """A device array described by hand (never dereferenced: validation only)."""
    return {"ptr": 0x10000, "typestr": typestr, "shape": tuple(shape), "strides": strides}


def test_targets():
    K, h, w = 3, 5, 7
    assert D.maps_target(arr((K, 4, h, w), "<f4"), "float32", K, h, w)[2] == _lib.FOTO_F32
    assert D.maps_target(arr((K, 4, h, w), "<f8"), np.float64, K, h, w)[2] == _lib.FOTO_F64
    for bad, dt in ((arr((K, 3, h, w), "<f4"), "float32"), (arr((K, 4, w, h), "<f4"), "float32"),
                    (arr((K, 4, h, w), "<f8"), "float32"), (arr((K, 4, h, w), "|u1"), "uint8"),
                    (arr((K, 4, h, w), "<f4", (4 * h * w * 8, h * w * 4, w * 4, 4)), "float32")):
        with pytest.raises(ValueError):
            D.maps_target(bad, dt, K, h, w)
    assert D.interp_target(arr((K, h, w, 3), "|u1"), "uint8", K, h, w, 3, True)[2] == _lib.FOTO_U8
    assert D.interp_target(arr((K, h, w), "<f8"), "float64", K, h, w, 1, False)[2] == _lib.FOTO_F64
    for bad, dt, C, has_c in ((arr((K, h, w), "|u1"), "uint8", 3, True), (arr((K, h, w, 1), "<f4"), "float32", 1, False),
                              (arr((K, h, w, 3), "<f2"), "float16", 3, True)):
        with pytest.raises(ValueError):
            D.interp_target(bad, dt, K, h, w, C, has_c)
    a, b, C, sc0, sc1, has_c, own = D.interp_frames(arr((h, w, 3), "|u1"), arr((h, w, 3), "|u1", (w * 4, 4, 1)))
    assert (C, sc0, sc1, has_c, own) == (3, 1, 1, True, "uint8") and (a.stride_x, b.stride_x) == (3, 4)
    assert a.divisor == 255.0
    a, b, C, sc0, sc1, has_c, own = D.interp_frames(arr((2, h, w), "<f4"), arr((2, h, w), "<f4"), channels_last=False)
    assert (C, sc0, has_c, own) == (2, h * w, True, "float32") and a.divisor == 1.0
    with pytest.raises(ValueError):
        D.interp_frames(arr((h, w, 3), "|u1"), arr((h, w), "|u1"))
    with pytest.raises(ValueError):
        D.interp_frames(arr((h, w), "<f8"), arr((h, w + 1), "<f8"))


# ------------------------------------------------------------------ main.py

def test_main_parser_defaults():
    import main as M
    a = M.build_parser().parse_args(["a.png", "b.png"])
    assert a.inbetweens == 0 and a.save_inbetweens is None
    a = M.build_parser().parse_args(["a.png", "b.png", "--algo=foto", "--inbetweens", "3", "--save-inbetweens", "mid_"])
    assert a.inbetweens == 3 and a.save_inbetweens == "mid_"
    t = M.inbetween_times(3, 5)
    assert t.tolist() == [1.0, 2.0, 3.0] and M.inbetween_times(1, 8).tolist() == [3.5]
