"""Entropic transport (include/foto.h, "entropic transport"), the parts that need no GPU: the numpy
restatement tests/sinkhorn_ref.py against a dense Sinkhorn solve with the same truncated kernel, the
host tables, the conditions the GPU tests lean on (met by the restatement alone), and the argument
rules of the Python layer and of the C entries, which come before any device use."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import PKG, REPO  # noqa: F401  (puts the package on sys.path)

import sinkhorn_ref as R  # noqa: E402
from foto import _lib, sinkhorn  # noqa: E402
from foto.synthetic import translating_gaussian  # noqa: E402

ENTRIES = ["foto_sinkhorn_opts_default", "foto_sinkhorn_create", "foto_sinkhorn_destroy", "foto_sinkhorn_set_frames_dev",
           "foto_sinkhorn_iterate_dev", "foto_sinkhorn_flow_dev", "foto_sinkhorn_info_dev", "foto_sinkhorn_scalings_dev",
           "foto_sinkhorn_solve", "foto_sinkhorn_solve_dev"]


# ------------------------------------------------------------------ the restatement against a dense solve

@pytest.mark.parametrize("eps", [0.5, 2.0])
@pytest.mark.parametrize("radius", [1, 3])
@pytest.mark.parametrize("w,h", [(6, 5), (7, 4)])
def test_ref_against_dense_sinkhorn(w, h, radius, eps):
    """The separable, tap-by-tap convolution against matrix products with the dense N x N truncated
    kernel.  Only the summation order (and the rounding of k[dx] k[dy]) differs: fewer than 50 terms
    per output, so n 2^-53 with n < 50 per operation; 1e-12 relative holds a few iterations of it."""
    rng = np.random.default_rng(100 * w + 10 * radius + int(eps))
    f0, f1 = rng.random((h, w)) + 0.1, rng.random((h, w)) + 0.1
    f0[1, 2] = 0.0   # a pixel without mass
    tab = R.tables(eps, radius)
    iters = 4
    ref = R.Ref(w, h, eps, radius).set_frames(f0, f1).iterate(iters)
    a, b, u, v, ok, cost = R.dense_solve(f0, f1, w, h, tab, iters)
    ru, rv, rok = ref.flow()
    info = ref.info()
    for got, want, what in ((ref.a, a, "a"), (ref.b, b, "b"), (ru, u, "u"), (rv, v, "v")):
        scale = np.abs(want).max()
        err = np.abs(got - want).max() / scale
        print(f"{w}x{h} R={radius} eps={eps} {what}: {err:.3e}")
        assert err <= 1e-12, what
    assert np.array_equal(rok.astype(bool), ok) and not rok[1, 2] and ru[1, 2] == 0.0
    assert abs(info["cost"] - cost) <= 1e-12 * abs(cost)
    assert info["w2"] == np.sqrt(2.0 * info["cost"]) and info["iterations"] == iters and info["bad"] == 0


# ------------------------------------------------------------------ tables

def test_tables():
    for eps, rad in ((2.0, 16), (1.0, 32), (8.0, 7), (0.5, 1)):
        t = sinkhorn.tables(eps, rad)
        assert t.shape == (3, rad + 1) and t.dtype == np.float64 and t[0, 0] == 1.0
        d = np.arange(rad + 1, dtype=np.float64)
        assert R.same(t[0], np.exp(-(d * d) / (2.0 * eps)))
        assert R.same(t[1], d * t[0]) and R.same(t[2], (0.5 * (d * d)) * t[0])
        assert R.same(t, R.tables(eps, rad))
        assert np.all(np.diff(t[0]) < 0)
    t = sinkhorn.tables(3.0, 0)
    assert t.shape == (3, 1) and list(t[:, 0]) == [1.0, 0.0, 0.0]
    s = R.signed(R.tables(2.0, 3))
    assert s.shape == (3, 7) and R.same(s[0], s[0][::-1]) and R.same(s[1], -s[1][::-1]) and R.same(s[2], s[2][::-1])


@pytest.mark.parametrize("eps,rad", [(2.0, -1), (2.0, 33), (2.0, 1.5), (0.0, 4), (-1.0, 4), (np.nan, 4),
                                     (np.inf, 4)])
def test_tables_argument_errors(eps, rad):
    with pytest.raises(ValueError):
        sinkhorn.tables(eps, rad)
    with pytest.raises(ValueError):
        R.tables(eps, rad)


# ------------------------------------------------------------------ the conditions the GPU tests lean on

W, H = 40, 24


@pytest.fixture(scope="module")
def gaussians():
    f0, f1 = translating_gaussian(W, H)   # sigma 3, centres 18 and 22: a 4 px shift, tails below 1e-8
    return f0.reshape(H, W), f1.reshape(H, W)


def test_ref_marginal_error_falls(gaussians):
    f0, f1 = gaussians
    ref = R.Ref(W, H, 2.0, 12).set_frames(f0, f1)
    rel, done = [], 0
    for n in (5, 10, 20, 40, 80):
        ref.iterate(n - done)
        done = n
        i = ref.info()
        rel.append(i["marginal_error"] / i["mass0"])
    print("marginal error / mass at 5, 10, 20, 40, 80 iterations:", rel)
    assert all(b < a for a, b in zip(rel, rel[1:]))
    assert rel[3] < 1e-3


def test_ref_debiased_w2_is_the_shift(gaussians):
    f0, f1 = gaussians
    (c01, c00, c11), refs = R.costs(f0, f1, W, H, 2.0, 12, 60)
    d = c01 - 0.5 * c00 - 0.5 * c11
    mass = refs[0].info()["mass0"]
    got = np.sqrt(2.0 * max(d, 0.0)) / np.sqrt(mass)
    print(f"w2_debiased / sqrt(mass) = {got!r}, w2 / sqrt(mass) = {np.sqrt(2 * c01 / mass)!r}")
    assert abs(got - 4.0) <= 1e-3 * 4.0
    assert R.divergence(f0, f1, W, H, 2.0, 12, 60) == (d, np.sqrt(2.0 * max(d, 0.0)))
    # the flow itself: the mass-weighted mean of u is the shift, v has none
    u, v, ok = refs[0].flow()
    mu = refs[0].mu
    assert abs((mu * u).sum() / mu.sum() - 4.0) < 0.02 and abs((mu * v).sum() / mu.sum()) < 1e-6


def test_ref_equal_frames(gaussians):
    """mu = nu: the (mu, nu) solve is the (mu, mu) solve, the divergence exactly 0, and the forward
    and backward flows -- which read b and a, equal at the fixed point alone -- meet as the
    iterations go on."""
    f0, _ = gaussians
    (c01, c00, c11), refs = R.costs(f0, f0, W, H, 2.0, 12, 60)
    assert c01 == c00 == c11 and R.divergence(f0, f0, W, H, 2.0, 12, 60) == (0.0, 0.0)
    uf, vf, okf = refs[0].flow("forward")
    ub, vb, okb = refs[0].flow("backward")
    gap = max(np.abs(uf - ub).max(), np.abs(vf - vb).max())
    print("forward - backward flow at 60 iterations:", gap)
    assert np.array_equal(okf, okb) and gap < 1e-6


# ------------------------------------------------------------------ arguments, before the library is touched

def test_python_argument_errors(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(sinkhorn, "lib", touched)
    for kw in (dict(radius=33), dict(radius=-1), dict(radius=2.0), dict(eps=0.0), dict(eps=-2.0), dict(eps=float("nan"))):
        with pytest.raises(ValueError):
            sinkhorn.Sinkhorn(8, 8, **kw)
    with pytest.raises(ValueError):
        sinkhorn.Sinkhorn(0, 8)
    z = np.zeros((4, 4))
    for kw in (dict(iters=-1), dict(iters=2.5), dict(radius=40), dict(eps=0)):
        with pytest.raises(ValueError):
            sinkhorn.divergence(z, z, **kw)
    with pytest.raises(ValueError):
        sinkhorn.cached_sinkhorn(8, 8, radius=99)


def test_header_and_bindings():
    src = open(os.path.join(REPO, "include", "foto.h")).read()
    L = _lib.lib()
    for name in ENTRIES:
        assert re.search(r"\b(int|void) " + name + r"\(", src), name
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert ctypes.sizeof(_lib.SinkhornOpts) == 16
    for name, val in (("MAX_RADIUS", _lib.FOTO_SINKHORN_MAX_RADIUS), ("TILE_W", _lib.FOTO_SINKHORN_TILE_W),
                      ("TILE_H", _lib.FOTO_SINKHORN_TILE_H)):
        assert re.search(rf"#define FOTO_SINKHORN_{name} {val}\b", src), name
    o = _lib.SinkhornOpts()
    assert L.foto_sinkhorn_opts_default(ctypes.byref(o)) == 0 and (o.radius, o.per_launch_reserved, o.eps) == (16, 0, 2.0)
    assert L.foto_sinkhorn_opts_default(None) == _lib.FOTO_ERR_ARG


def test_c_argument_errors_before_any_device_use():
    L = _lib.lib()
    tab = sinkhorn.tables(2.0, 4)
    p = ctypes.c_void_p()

    def create(w, h, radius, eps, t=tab, out=p):
        o = _lib.SinkhornOpts(radius, 0, eps)
        return L.foto_sinkhorn_create(w, h, ctypes.byref(o), None if t is None else _lib.dptr(t),
                                      None if out is None else ctypes.byref(out))

    for args in ((0, 8, 4, 2.0), (8, 0, 4, 2.0), (65536, 32768, 4, 2.0), (8, 8, -1, 2.0), (8, 8, 33, 2.0), (8, 8, 4, 0.0),
                 (8, 8, 4, -1.0), (8, 8, 4, float("nan")), (8, 8, 4, float("inf"))):
        assert create(*args) == _lib.FOTO_ERR_ARG, args
        assert L.foto_last_error() and p.value is None
    assert create(8, 8, 4, 2.0, t=None) == _lib.FOTO_ERR_ARG and b"tables" in L.foto_last_error()
    assert create(8, 8, 4, 2.0, out=None) == _lib.FOTO_ERR_ARG
    # a null context
    assert L.foto_sinkhorn_iterate_dev(None, 1, None) == _lib.FOTO_ERR_ARG
    assert L.foto_sinkhorn_flow_dev(None, 0, None, _lib.FOTO_F32, 0, None, None) == _lib.FOTO_ERR_ARG
    assert L.foto_sinkhorn_info_dev(None, None, None) == _lib.FOTO_ERR_ARG
    assert L.foto_sinkhorn_scalings_dev(None, None, None, None) == _lib.FOTO_ERR_ARG
    assert L.foto_sinkhorn_set_frames_dev(None, None, None, None) == _lib.FOTO_ERR_ARG
    L.foto_sinkhorn_destroy(None)
