"""CPU checks of the coarse-to-fine GN scheme: the level-size rule and the argument errors of the
C ABI (no device is touched), and the numpy restatement (tests/gn_pyr_ref.py) that the GPU tests
measure against, pinned by results of its own."""
import ctypes

import numpy as np
import pytest

import gn_pyr_ref as R
from oracle import foto_oracle as O


def c_sizes(w, h, levels, min_size, cap=16):
    from foto import _lib
    wl, hl, n = (ctypes.c_int * cap)(), (ctypes.c_int * cap)(), ctypes.c_int(-1)
    rc = _lib.lib().foto_gn_pyr_sizes(w, h, levels, min_size, wl, hl, cap, ctypes.byref(n))
    return rc, [(wl[l], hl[l]) for l in range(max(n.value, 0))]


@pytest.mark.parametrize("w,h,levels,expect", [
    (96, 80, 4, [(96, 80), (48, 40), (24, 20)]),
    (71, 77, 3, [(71, 77), (36, 39), (18, 20)]),
    (33, 17, 7, [(33, 17)]),
])
def test_sizes_table(w, h, levels, expect):
    rc, got = c_sizes(w, h, levels, 16)
    assert rc == 0 and got == expect
    assert R.sizes(w, h, levels, 16) == expect


@pytest.mark.parametrize("min_size", [2, 16, 100])
@pytest.mark.parametrize("w,h,levels", [(96, 80, 4), (71, 77, 3), (33, 17, 5), (640, 480, 5), (3, 2, 2), (1100, 3, 4)])
def test_sizes_rule(w, h, levels, min_size):
    rc, got = c_sizes(w, h, levels, min_size)
    assert rc == 0
    assert got[0] == (w, h) and 1 <= len(got) <= levels
    for l in range(len(got) - 1):
        assert min(got[l]) >= 2 * min_size
        assert got[l + 1] == (-(-got[l][0] // 2), -(-got[l][1] // 2))
    assert len(got) == levels or min(got[-1]) < 2 * min_size
    assert got == R.sizes(w, h, levels, min_size)
    from foto import gn
    assert gn.pyramid_sizes(w, h, levels, min_size) == got


def test_argument_errors_without_gpu():
    """Every argument error is FOTO_ERR_ARG with a message, found before any HIP call: these pass
    on a machine without a device."""
    from foto import _lib
    L = _lib.lib()
    E = _lib.FOTO_ERR_ARG
    for args in ((96, 80, 0, 16), (96, 80, 3, 1), (1, 80, 3, 16), (96, 1, 3, 16)):
        rc, _ = c_sizes(*args)
        assert rc == E and L.foto_last_error()
    assert c_sizes(640, 480, 5, 16, cap=2)[0] == E
    n = ctypes.c_int(0)
    assert L.foto_gn_pyr_sizes(96, 80, 3, 16, None, None, 16, ctypes.byref(n)) == E
    assert L.foto_gn_pyr_opts_default(None) == E
    o = _lib.GNPyrOpts()
    assert L.foto_gn_pyr_opts_default(ctypes.byref(o)) == 0
    assert (o.levels, o.warps, o.min_size, o.rtol, o.maxiter) == (4, 3, 16, 1e-10, 200000)
    p = ctypes.c_void_p()

    def create(w, h, alpha, lam, **kw):
        oo = _lib.GNPyrOpts(o.levels, o.warps, o.min_size, o.rtol, o.maxiter)
        for k, v in kw.items():
            setattr(oo, k, v)
        return L.foto_gn_pyr_create(w, h, alpha, lam, ctypes.byref(oo), ctypes.byref(p))

    assert create(96, 80, 0.1, 0.2, levels=0) == E
    assert create(96, 80, 0.1, 0.2, warps=0) == E
    assert create(96, 80, 0.1, 0.2, min_size=1) == E
    assert create(1, 80, 0.1, 0.2) == E and create(96, 1, 0.1, 0.2) == E
    assert create(96, 80, 0.0, 0.2) == E and create(96, 80, 0.1, -1.0) == E
    assert create(96, 80, 0.1, 0.2, maxiter=-1) == E
    assert not p.value
    assert L.foto_gn_pyr_create(96, 80, 0.1, 0.2, None, None) == E
    z = np.zeros(16)
    d = _lib.dptr(z)
    assert L.foto_gn_pyr_solve(None, d, d, d, d, d, None) == E
    assert L.foto_gn_pyr_solve_dev(None, None, None, None, 1, 0, None, None) == E
    assert L.foto_gn_pyr_device(None) == -1
    assert L.foto_pyr_down(None, d, 4, 4, d, d) == E and L.foto_pyr_down(d, d, 0, 4, d, d) == E
    assert L.foto_pyr_up(d, d, None, 2, 2, 4, 4, d, d, d) == E and L.foto_pyr_up(d, d, d, 1, 2, 4, 4, d, d, d) == E
    assert L.foto_gn_warp_prior(d, d, d, d, 4, 4, None) == E and L.foto_gn_warp_prior(d, d, d, d, 1, 4, d) == E
    assert L.foto_gn_solve_prior(None, d, 4, 4, 0.1, 0.2, 1e-10, 10, None, None, None, d, d, d, None) == E
    assert L.foto_gn_solve_prior(d, d, 4, 4, 0.1, 0.2, 1e-10, 10, d, None, None, d, d, d, None) == E
    assert ctypes.sizeof(_lib.GNPyrOpts) == 32 and _lib.GNPyrOpts.rtol.offset == 16
    assert _lib.GNPyrStats.levels.offset == 24 and _lib.GNPyrStats.ms_level.offset == 160
    assert ctypes.sizeof(_lib.GNPyrStats) == 160 + 8 * 16 + 16


def test_cli_and_dropin_defaults():
    """The new switches default to the single solve: --gn-levels / --gn-warps 1 / 1, and a
    GLLOpticalFlow that never saw setPyramid has no pyramid."""
    import classical
    import main as M
    a = M.build_parser().parse_args(["a.png", "b.png", "--algo", "GN"])
    assert (a.gn_levels, a.gn_warps) == (1, 1)
    a = M.build_parser().parse_args(["a.png", "b.png", "--algo", "GN", "--gn-levels", "4", "--gn-warps", "3"])
    assert (a.gn_levels, a.gn_warps) == (4, 3)
    g = classical.GLLOpticalFlow(8, 8)
    assert not hasattr(g, "pyramid")
    g.setPyramid(3, 2)
    assert g.pyramid == (3, 2)


def test_restatement_large_displacement():
    """The 45x37 row: the single solve is > 2 px short, the 2 x 2 pyramid is within 0.1 px."""
    w, h, (dx, dy), _, _, _ = R.CASES["45x37"]
    f1, f2 = R.frames("45x37")
    u0, v0, _ = O.gn_solve(f1, f2, w, h, R.ALPHA, R.LAM)
    u, v, _ = R.reference("45x37")
    e0, e = R.interior_epe(u0, v0, w, h, dx, dy), R.interior_epe(u, v, w, h, dx, dy)
    print(f"45x37 ({dx}, {dy}): gn_solve {e0:.3f} px, pyramid {e:.4f} px")
    assert e0 > 2.0 and e < 0.1


def test_restatement_one_level_is_gn_solve():
    w, h = 45, 37
    f1, f2 = R.frames("45x37")
    ref = O.gn_solve(f1, f2, w, h, R.ALPHA, R.LAM)
    got = R.pyramid(f1, f2, w, h, R.ALPHA, R.LAM, 1, 1)
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)
    # a level the size rule refuses changes nothing either
    got = R.pyramid(f1, f2, w, h, R.ALPHA, R.LAM, 3, 1, min_size=32)
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)


def test_restatement_identical_frames_give_zero():
    w, h = 45, 37
    f1, _ = R.frames("45x37")
    for a in R.pyramid(f1, f1, w, h, R.ALPHA, R.LAM, 2, 2):
        assert a.shape == (w * h,) and not a.any()


def test_restatement_pieces():
    """down's clamped taps on odd sizes, sample's clamping and NaN rule, up's scales."""
    f = np.arange(15, dtype=np.float64)   # 3 x 5: f[j][i] = 3 j + i
    c = R.down(f, 3, 5).reshape(3, 2)
    assert c[0, 0] == 0.25 * (0 + 1 + 3 + 4) and c[0, 1] == 0.25 * (2 + 2 + 5 + 5) and c[2, 1] == 14.0
    x = np.array([0.0, 2.0, 1.5, -7.0, 1e9, np.nan, 1.0])
    y = np.array([0.0, 4.0, 0.5, 2.0, 1e9, 0.0, np.nan])
    s = R.sample(f, 3, 5, x, y)
    assert list(s[:5]) == [0.0, 14.0, 3.0, 6.0, 14.0] and np.isnan(s[5]) and np.isnan(s[6])
    one = np.ones(4)
    u, v, m = R.up(one, one, one, 2, 2, 4, 3)
    assert np.array_equal(u, np.full(12, 2.0)) and np.array_equal(v, np.full(12, 1.5)) and np.array_equal(m, np.ones(12))
