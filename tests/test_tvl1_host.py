"""CPU checks of the TV-L1 solver: the CLI's new flags, the C ABI's records and argument errors
(no device is touched), and the numpy restatement (tests/tvl1_ref.py) that the GPU tests measure
against, held to the quality conditions so that those inputs are known to work for the reference
alone."""
import ctypes

import numpy as np
import pytest

import gn_pyr_ref as G
import tvl1_ref as T


def test_cli_flags_and_defaults():
    import main as M
    a = M.build_parser().parse_args(["a.png", "b.png", "--algo", "TVL1"])
    assert (a.tv_lambda, a.tv_theta, a.tv_tau, a.tv_gamma) == (38.0, 0.3, 0.25, 0.1)
    assert (a.tv_levels, a.tv_warps, a.tv_iters) == (4, 5, 30)
    a = M.build_parser().parse_args(["a.png", "b.png", "--algo=TVL1", "--tv-lambda", "20", "--tv-theta", "0.25",
                                     "--tv-tau=0.2", "--tv-gamma", "0", "--tv-levels", "3", "--tv-warps", "2",
                                     "--tv-iters", "7", "--median", "2", "--stats"])
    assert (a.tv_lambda, a.tv_theta, a.tv_tau, a.tv_gamma) == (20.0, 0.25, 0.2, 0.0)
    assert (a.tv_levels, a.tv_warps, a.tv_iters, a.median, a.stats) == (3, 2, 7, 2, True)
    # the other two algorithms' defaults stay what they are
    assert (a.gn_levels, a.gn_warps, a.Nt, a.alpha, a.lambdaa) == (1, 1, 4, 0.1, 0.2)


def test_abi_records_defaults_and_signatures():
    from foto import _lib, tvl1
    L = _lib.lib()
    for name in ("foto_tvl1_opts_default", "foto_tvl1_create", "foto_tvl1_destroy", "foto_tvl1_device",
                 "foto_tvl1_solve", "foto_tvl1_solve_dev", "foto_tvl1_coeffs", "foto_tvl1_iterate"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    # 4 doubles, 5 ints; int, 4 pointers, 2 ints, double
    assert ctypes.sizeof(_lib.TVL1Opts) == 56 and _lib.TVL1Opts.levels.offset == 32
    assert _lib.TVL1Opts.per_launch.offset == 48
    assert ctypes.sizeof(_lib.TVL1Stats) == 56 and _lib.TVL1Stats.wl.offset == 8
    assert _lib.TVL1Stats.levels.offset == 40 and _lib.TVL1Stats.ms_total.offset == 48
    o = _lib.TVL1Opts()
    assert L.foto_tvl1_opts_default(ctypes.byref(o)) == 0
    got = {k: getattr(o, k) for k in tvl1.DEFAULTS}
    assert got == tvl1.DEFAULTS
    assert 1 <= got.pop("per_launch") <= _lib.FOTO_TVL1_MAX_PER_LAUNCH == 8   # (how it runs, not what it computes)
    assert got == T.DEFAULTS == dict(lam=38.0, theta=0.3, tau=0.25, gamma=0.1, levels=4, warps=5, iters=30,
                                     min_size=16)
    with pytest.raises(TypeError):
        tvl1.cached_tvl1(8, 8, bicubic=True)


def test_argument_errors_without_gpu():
    """Every argument error is FOTO_ERR_ARG with a message, found before any HIP call."""
    from foto import _lib
    L = _lib.lib()
    E = _lib.FOTO_ERR_ARG
    assert L.foto_tvl1_opts_default(None) == E
    p = ctypes.c_void_p()

    def create(w, h, **kw):
        o = _lib.TVL1Opts()
        L.foto_tvl1_opts_default(ctypes.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        rc = L.foto_tvl1_create(w, h, ctypes.byref(o), ctypes.byref(p))
        assert rc >= 0 or L.foto_last_error()
        return rc

    assert create(1, 80) == E and create(96, 1) == E and create(0, 0) == E
    for kw in (dict(theta=0.0), dict(theta=-0.3), dict(tau=0.0), dict(tau=-1.0), dict(theta=float("nan")),
               dict(tau=float("inf")), dict(lam=-1.0), dict(gamma=-0.1), dict(levels=0), dict(warps=0),
               dict(iters=0), dict(min_size=1), dict(per_launch=0), dict(per_launch=9)):
        assert create(96, 80, **kw) == E, kw
    assert not p.value
    assert L.foto_tvl1_create(96, 80, None, None) == E
    z = np.zeros(64)
    d = _lib.dptr(z)
    assert L.foto_tvl1_solve(None, d, d, d, d, d, None) == E
    assert L.foto_tvl1_solve_dev(None, None, None, None, 1, 0, None, None) == E
    assert L.foto_tvl1_device(None) == -1
    assert L.foto_tvl1_coeffs(None, d, d, d, 2, 2, 0.1, d) == E and L.foto_tvl1_coeffs(d, d, d, d, 1, 2, 0.1, d) == E
    assert L.foto_tvl1_iterate(d, d, None, 2, 2, 38.0, 0.3, 0.25, 1, 1) == E
    assert L.foto_tvl1_iterate(d, d, d, 2, 1, 38.0, 0.3, 0.25, 1, 1) == E
    assert L.foto_tvl1_iterate(d, d, d, 2, 2, 38.0, 0.0, 0.25, 1, 1) == E
    assert L.foto_tvl1_iterate(d, d, d, 2, 2, 38.0, 0.3, -0.25, 1, 1) == E
    assert L.foto_tvl1_iterate(d, d, d, 2, 2, 38.0, 0.3, 0.25, 0, 1) == E
    assert L.foto_tvl1_iterate(d, d, d, 2, 2, 38.0, 0.3, 0.25, 1, 0) == E
    assert L.foto_tvl1_iterate(d, d, d, 2, 2, 38.0, 0.3, 0.25, 1, 9) == E
    assert L.foto_last_error()


# ------------------------------------------------------------------ the restatement

def test_restatement_pieces():
    """grad_c's zero edges, fwd / div as minus adjoints of each other, the three branches of k."""
    w, h = 5, 4
    rng = np.random.default_rng(0)
    f = rng.random(w * h)
    gx, gy = (a.reshape(h, w) for a in T.grad_c(f, w, h))
    F = f.reshape(h, w)
    assert not gx[:, 0].any() and not gx[:, -1].any() and not gy[0].any() and not gy[-1].any()
    assert gx[2, 1] == 0.5 * (F[2, 2] - F[2, 0]) and gy[1, 3] == 0.5 * (F[2, 3] - F[0, 3])
    a, px, py = rng.random((h, w)), rng.random((h, w)), rng.random((h, w))
    dx, dy = T.fwd(a)
    assert not dx[:, -1].any() and not dy[-1].any()
    assert abs((dx * px + dy * py).sum() + (a * T.div(px, py)).sum()) < 1e-13     # <fwd a, p> = -<a, div p>
    # one pixel per branch; U = 0, P = 0, so U_d after one iteration is k a_d
    lam, theta, tau = 38.0, 0.3, 0.25
    lt = lam * theta
    a1 = np.array([0.5, 0.5, 0.5, 0.0])
    z = np.zeros(4)
    n2 = a1 * a1
    rc = np.array([-2 * lt * 0.25, 2 * lt * 0.25, 0.1, 0.3])   # below, above, between, n2 = 0
    U, P = T.iterate((a1, z, z, n2, rc), [z, z, z], [z] * 6, 2, 2, lam, theta, tau, 1)
    assert list(U[0]) == [lt * 0.5, -lt * 0.5, (-0.1 / 0.25) * 0.5, 0.0]
    assert not U[1].any() and not U[2].any()
    assert np.all(np.abs(np.array(P)) <= 1.0)


def test_restatement_gamma_zero_leaves_w_zero():
    w, h = 45, 37
    f1, f2 = G.frames("45x37")
    U = T.level(f1, f2, [np.zeros(w * h)] * 3, w, h, 38.0, 0.3, 0.25, 0.0, 2, 5)
    assert U[0].any() and U[1].any() and not U[2].any()
    u, v, m = T.reference("45x37", 0.0)
    assert u.any() and not m.any()


def test_restatement_identical_frames_give_zero():
    w, h = 45, 37
    f1, _ = G.frames("45x37")
    for a in T.tvl1(f1, f1, w, h, levels=2, warps=2, iters=5):
        assert a.shape == (w * h,) and not a.any()


def test_restatement_error_propagation():
    """What a per-iteration error of the operator tolerance does to the final flow: every channel
    of every inner iteration perturbed by +-1e-13.  This is the ground of the GPU test's whole-solve
    bound, 1e-6 max(1, max|ref|).  Measured: at most 8.7e-8 (71x77 at gamma 0, where the -rho / n2
    branch amplifies in flat regions), 4.4e-10 and below on the other five."""
    rng = np.random.default_rng(0)

    def pert(n):
        return rng.choice([-1e-13, 1e-13], n)

    worst = 0.0
    for case in G.CASES:
        w, h = G.CASES[case][:2]
        for gamma in T.GAMMAS:
            ref = T.reference(case, gamma)
            got = T.tvl1(*G.frames(case), w, h, gamma=gamma, perturb=pert)
            moved = max(np.abs(a - b).max() for a, b in zip(got, ref))
            worst = max(worst, moved)
            print(f"{case} gamma {gamma}: +-1e-13 per iteration moved the flow by {moved:.3e}")
    assert worst <= 1e-6   # inside the whole-solve bound; DESIGN.md records the figures


def test_restatement_quality_layered():
    """Two layers moving (2, 0) and (-2, 1): TV-L1 keeps the boundary the quadratic GN prior smears.
    Condition: interior EPE <= 0.25 x the GN pyramid's (levels 3, warps 3).  Measured with this
    restatement: 0.147 px against 0.888 px, ratio 0.165."""
    w, h = 96, 80
    f1, f2, tu, tv = T.layered_pair()
    u, v, _ = T.tvl1(f1, f2, w, h)
    gu, gv, _ = G.pyramid(f1, f2, w, h, G.ALPHA, G.LAM, 3, 3)
    e, eg = T.interior_epe(u, v, w, h, tu, tv), T.interior_epe(gu, gv, w, h, tu, tv)
    print(f"layered: TV-L1 {e:.4f} px, GN pyramid {eg:.4f} px, ratio {e / eg:.3f} (bound 0.25)")
    assert e <= 0.25 * eg


def test_restatement_quality_shift_and_brightness():
    """(5, 3) px shift: EPE <= 0.02 px at both gammas (measured 0.0028 and 0.0057).  The same shift
    with a smooth 30 % brightness bump on frame 1: gamma = 0.1 gives <= 0.03 px (0.0110), gamma = 0
    at least ten times that (0.452)."""
    w, h = 96, 80
    e = {}
    for bright in (False, True):
        f1, f2 = T.shift_pair(bright)
        for gamma in T.GAMMAS:
            u, v, m = T.tvl1(f1, f2, w, h, gamma=gamma)
            e[bright, gamma] = T.interior_epe(u, v, w, h, 5.0, 3.0)
            print(f"shift, bump {bright}, gamma {gamma}: interior EPE {e[bright, gamma]:.4f} px")
            assert gamma != 0.0 or not m.any()
    assert e[False, 0.0] <= 0.02 and e[False, 0.1] <= 0.02
    assert e[True, 0.1] <= 0.03
    assert e[True, 0.0] >= 10 * e[True, 0.1]
