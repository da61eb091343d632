"""Maps and in-betweens on the GPU (include/foto.h: foto_bb_maps / _dev, foto_bb_interp_dev,
foto_maps_from_phi, foto_interp_from_phi; BBSolver.maps / maps_device / interpolate,
ops.maps_from_phi / interp_from_phi, foto.device.bb_interpolate).

Checker.  tests/interp_ref.py, the numpy restatement of the header's definitions, on the seeded
smooth phi of test_interp_host.py (max |dV| per pixel 0.3 < 0.5, asserted there: the inverse step
is a contraction, so it does not amplify a last-bit difference).  Bars: maps rtol 1e-13 / atol
1e-12, the project's bar for the trajectory step (test_track_from_phi_golden); float64 images of
frames in [0, 1] atol 1e-11 (a position error of 1e-12 px times a unit Lipschitz bound, plus
rounding); 8-bit images equal except where the reference's 255 x + 0.5 lies within 1e-9 of an
integer, at most 1e-4 of all pixels.  The measured maxima are printed.

Everything else compares entries of this build with each other, bit for bit.  A wild phi (the
smooth one times 50: trajectories leave the frame, the inverse step does not contract) is only
asked for the same bits twice, and for finite output where the definition itself stays finite
(inv_iters 1; test_wild_phi_is_deterministic_and_finite has the reason and the figures).
"""
import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import PKG, REPO  # noqa: E402  (puts the package on sys.path)

import interp_ref as R  # noqa: E402
from foto import _lib, ops  # noqa: E402
from foto import device as D  # noqa: E402
from foto.bb import BBSolver  # noqa: E402
from foto.device import DeviceArray  # noqa: E402
from foto.synthetic import textured_pair  # noqa: E402
from test_interp_host import SHAPES, times  # noqa: E402


def ibits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(ibits(a), ibits(b))


def pair(w, h, seed=0):
    a, b = textured_pair(w, h, seed=seed)
    return a.reshape(h, w), b.reshape(h, w)


# ------------------------------------------------------------------ 1. parity with the restatement

_ref = {}


def reference(Nx, Ny, Nt, it):
    """The seeded inputs of one shape and the restatement on them, computed once."""
    key = (Nx, Ny, Nt, it)
    if key not in _ref:
        phi = R.smooth_phi(Nt, Ny, Nx, seed=Nx)
        f0, f1 = R.smooth_frames(Ny, Nx, 3)
        T = times(Nt)
        _ref[key] = dict(phi=phi, f0=f0, f1=f1, T=T, maps=np.stack([R.maps(phi, s, it) for s in T]),
                         img=np.stack([R.interp(phi, f0, f1, s, it) for s in T]))
    return _ref[key]


@pytest.mark.parametrize("it", [1, 6])
@pytest.mark.parametrize("Nx,Ny,Nt", SHAPES)
def test_from_phi_parity(Nx, Ny, Nt, it):
    r = reference(Nx, Ny, Nt, it)
    got = ops.maps_from_phi(r["phi"], Nt, Nx, Ny, r["T"], inv_iters=it)
    assert got.shape == (len(r["T"]), 4, Ny, Nx) and got.dtype == np.float64
    img = ops.interp_from_phi(r["phi"], Nt, Nx, Ny, r["f0"], r["f1"], r["T"], inv_iters=it)
    assert img.shape == (len(r["T"]), Ny, Nx, 3)
    print(f"{Nx}x{Ny}x{Nt}, inv_iters {it}: largest |map| {np.abs(r['maps']).max():.3f} px, max |map difference| "
          f"{np.abs(got - r['maps']).max():.3e}, max |image difference| {np.abs(img - r['img']).max():.3e}")
    np.testing.assert_allclose(got, r["maps"], rtol=1e-13, atol=1e-12)
    np.testing.assert_allclose(img, r["img"], rtol=0, atol=1e-11)
    # the exact ends: +0.0 planes, and both frames back bit for bit
    zero = np.zeros((2, Ny, Nx))
    assert same(got[0, :2], zero) and same(got[-1, 2:], zero)
    assert same(img[0], r["f0"]) and same(img[-1], r["f1"])
    u, v, _ = ops.flow_from_phi(r["phi"], Nt, Nx, Ny)
    assert same(got[0, 2].ravel(), u) and same(got[0, 3].ravel(), v)
    # one channel == that channel of the interleaved call; a 2-D frame has no channel axis
    one = ops.interp_from_phi(r["phi"], Nt, Nx, Ny, r["f0"][..., 1], r["f1"][..., 1], r["T"], inv_iters=it)
    assert one.shape == (len(r["T"]), Ny, Nx) and same(one, img[..., 1])
    # two calls, the same bits
    assert same(ops.maps_from_phi(r["phi"], Nt, Nx, Ny, r["T"], inv_iters=it), got)


def test_many_times_in_one_call():
    """130 times: two launches (128 + 2) == the same times one by one"""
    Nx, Ny, Nt = 67, 19, 5
    r = reference(Nx, Ny, Nt, 6)
    T = np.linspace(0.0, Nt - 1.0, 130)
    got = ops.maps_from_phi(r["phi"], Nt, Nx, Ny, T)
    img = ops.interp_from_phi(r["phi"], Nt, Nx, Ny, r["f0"], r["f1"], T)
    for k in (0, 1, 63, 127, 128, 129):
        assert same(ops.maps_from_phi(r["phi"], Nt, Nx, Ny, T[k:k + 1])[0], got[k]), k
        assert same(ops.interp_from_phi(r["phi"], Nt, Nx, Ny, r["f0"], r["f1"], T[k:k + 1])[0], img[k]), k
    np.testing.assert_allclose(got[77], R.maps(r["phi"], T[77], 6), rtol=1e-13, atol=1e-12)


# ------------------------------------------------------------------ 2. wild phi

def test_wild_phi_is_deterministic_and_finite():
    """Smooth phi times 50 (max |dV| per pixel 15): trajectories leave the frame and theta V is no
    contraction.  Outside the frame the cell extrapolates bilinearly, so one round of the inverse
    step (or one forward step) can square a position's distance from the frame: a chain of k rounds
    stays below 1e308 only while 2^k log10(distance) does.  With inv_iters = 1 the longest chain
    here has 5 rounds and steps, and the output must be finite; with inv_iters = 6 (up to 24
    rounds) the definition itself overflows -- the numpy restatement reaches 3.8e306 and then
    non-finite values on this phi -- so only the same bits are asked there, non-finite records
    included, and images that are finite wherever both of a pixel's ends are."""
    Nx, Ny, Nt = 67, 19, 5
    phi = 50.0 * R.smooth_phi(Nt, Ny, Nx, seed=Nx)
    assert R.max_dv(phi) > 10
    f0, f1 = R.smooth_frames(Ny, Nx, 3)
    T = times(Nt)
    for it in (1, 6):
        a = ops.maps_from_phi(phi, Nt, Nx, Ny, T, inv_iters=it)
        assert same(a, ops.maps_from_phi(phi, Nt, Nx, Ny, T, inv_iters=it))
        x = ops.interp_from_phi(phi, Nt, Nx, Ny, f0, f1, T, inv_iters=it)
        assert same(x, ops.interp_from_phi(phi, Nt, Nx, Ny, f0, f1, T, inv_iters=it))
        print(f"inv_iters {it}: {int((~np.isfinite(a)).sum())} of {a.size} map values non-finite, largest finite "
              f"|map| {np.abs(a[np.isfinite(a)]).max():.3e} px")
        if it == 1:
            assert np.isfinite(a).all() and np.isfinite(x).all()
            assert np.abs(a).max() > 10                   # trajectories do leave the neighbourhood
        ok = ~np.isnan(a).any(axis=1)                     # (an infinite end is clamped into the frame)
        assert np.isfinite(x[1:-1][ok[1:-1]]).all()
        fin = x[np.isfinite(x)]
        assert fin.min() >= -1e-12 and fin.max() <= 1.0 + 1e-12    # a convex combination of in-frame samples


def test_nan_pocket_stays_local():
    """A NaN in plane 1 of phi: the records of the pixels whose chains read it are non-finite, every
    other record keeps its bits.  A chain stays within (Nt - 1) max |V| + the stencil's 2 pixels of
    its pixel on this phi (max |V| 0.68: under 5 pixels; 8 asked)."""
    Nx, Ny, Nt = 67, 19, 5
    phi = R.smooth_phi(Nt, Ny, Nx, seed=Nx)
    f0, f1 = R.smooth_frames(Ny, Nx, 3)
    bad = phi.copy()
    j0, i0 = 9, 40
    bad[1, j0, i0] = np.nan
    T = times(Nt)
    clean, got = ops.maps_from_phi(phi, Nt, Nx, Ny, T), ops.maps_from_phi(bad, Nt, Nx, Ny, T)
    ci, gi = (ops.interp_from_phi(p, Nt, Nx, Ny, f0, f1, T) for p in (phi, bad))
    jj, ii = np.meshgrid(np.arange(Ny), np.arange(Nx), indexing="ij")
    far = np.maximum(np.abs(jj - j0), np.abs(ii - i0)) > 8
    assert same(got[:, :, far], clean[:, :, far]) and same(gi[:, far], ci[:, far])
    assert np.isfinite(clean).all() and np.isfinite(ci).all()
    for k in range(len(T)):
        assert not np.isfinite(got[k]).all(), T[k]    # every time's chains cross plane 1 somewhere near the pocket
    assert not np.isfinite(gi[1:-1]).all()


# ------------------------------------------------------------------ 3. the context

ITS = 3
CONFIGS = {
    "stencil-37x29x5": (37, 29, 5, dict(cg_mode=-1)),
    "pipelined-40x30x6": (40, 30, 6, dict(cg_mode=3)),
    "two-shards-40x30x6": (40, 30, 6, dict(cg_mode=3, virtual_ranks=2)),
    "three-shards-40x30x6": (40, 30, 6, dict(cg_mode=3, virtual_ranks=3)),
    "uneven-7x6x5": (7, 6, 5, dict(cg_mode=0, virtual_ranks=2)),
}
_solved = {}


def solved(name):
    """One solve per configuration (3 iterations, no stop rules) and everything the tests compare."""
    if name in _solved:
        return _solved[name]
    Nx, Ny, Nt, opts = CONFIGS[name]
    f0, f1 = pair(Nx, Ny)
    T = times(Nt)
    c0, c1 = R.smooth_frames(Ny, Nx, 3, seed=3)
    u0, u1 = R.u8_frames(Ny, Nx, 3, seed=3)
    r = dict(Nx=Nx, Ny=Ny, Nt=Nt, T=T, c0=c0, c1=c1, u0=u0, u1=u1)
    with BBSolver(f0.ravel(), f1.ravel(), Nt, Nx, Ny, **opts) as s:
        s.iterate(ITS, stop_rules=False)
        r["phi"], r["flow"] = s.phi(), s.flow()
        r["host"] = s.maps(T)
        r["host1"] = s.maps(T, inv_iters=1)
        r["dev64"] = s.maps_device(T, dtype="float64").to_numpy()
        r["dev32"] = s.maps_device(T).to_numpy()
        mine = DeviceArray((len(T), 4, Ny, Nx), np.float64)          # a caller-owned target
        assert s.maps_device(T, out=mine, dtype="float64") is mine
        r["mine"] = mine.to_numpy()
        r["img"] = s.interpolate(c0, c1, T)                          # numpy in, numpy out
        d0, d1 = DeviceArray.from_numpy(c0), DeviceArray.from_numpy(c1)
        r["img_dev"] = s.interpolate(d0, d1, T).to_numpy()           # device in, device out
        r["img32"] = s.interpolate(d0, d1, T, dtype="float32").to_numpy()
        r["img_ch"] = [s.interpolate(d0[:, :, c], d1[:, :, c], T).to_numpy() for c in range(3)]   # strided views
        p0 = DeviceArray.from_numpy(np.ascontiguousarray(c0.transpose(2, 0, 1)))
        p1 = DeviceArray.from_numpy(np.ascontiguousarray(c1.transpose(2, 0, 1)))
        r["img_planar"] = s.interpolate(p0, p1, T, channels_last=False).to_numpy()
        r["u8"] = s.interpolate(u0, u1, T)
        r["u8_f64"] = s.interpolate(u0, u1, T, dtype="float64")
        r["mixed"] = s.interpolate(DeviceArray.from_numpy(u0), DeviceArray.from_numpy((u1 / 255.0).astype(np.float64)), T,
                                   dtype="float64", divisor=None).to_numpy()
        r["flow_after"] = s.flow()
    _solved[name] = r
    return r


@pytest.mark.parametrize("name", list(CONFIGS))
def test_context(name):
    r = solved(name)
    Nx, Ny, Nt, T = r["Nx"], r["Ny"], r["Nt"], r["T"]
    host = r["host"]
    assert host.shape == (len(T), 4, Ny, Nx) and host.dtype == np.float64 and np.isfinite(host).all()
    # the context (virtual ranks: the plane table over every shard's buffer) == the test entry on
    # the gathered phi: 1, 2 and 3 shards read the same planes
    assert same(host, ops.maps_from_phi(r["phi"], Nt, Nx, Ny, T))
    assert same(r["host1"], ops.maps_from_phi(r["phi"], Nt, Nx, Ny, T, inv_iters=1)) and not same(r["host1"], host)
    assert same(r["dev64"], host) and same(r["mine"], host)
    assert same(r["dev32"], host.astype(np.float32))
    # the ends
    zero = np.zeros((2, Ny, Nx))
    assert same(host[0, :2], zero) and same(host[-1, 2:], zero)
    assert same(host[0, 2].ravel(), r["flow"][0]) and same(host[0, 3].ravel(), r["flow"][1])
    for a, b in zip(r["flow"], r["flow_after"]):
        assert same(a, b)
    # images
    img = r["img"]
    assert img.shape == (len(T), Ny, Nx, 3) and img.dtype == np.float64
    assert same(img, ops.interp_from_phi(r["phi"], Nt, Nx, Ny, r["c0"], r["c1"], T))
    assert same(r["img_dev"], img) and same(r["img32"], img.astype(np.float32))
    for c in range(3):                                  # 3 interleaved channels == three one-channel calls
        assert r["img_ch"][c].shape == (len(T), Ny, Nx) and same(r["img_ch"][c], img[..., c])
    assert same(r["img_planar"], img)                   # ([K][Ny][Nx][C] whatever the input's channel axis)
    assert same(img[0], r["c0"]) and same(img[-1], r["c1"])             # F64, divisor 1
    assert r["u8"].dtype == np.uint8 and same(r["u8"][0], r["u0"]) and same(r["u8"][-1], r["u1"])   # U8 -> U8
    # a uint8 frame 0 (divisor 255) with a float64 frame 1 (divisor 1): dtypes may differ per frame
    assert same(r["mixed"][0], r["u0"] / 255.0) and same(r["mixed"][-1], r["u1"] / 255.0)


def test_context_parity_u8_and_float():
    """The solved phi is not the seeded one, but as smooth (asserted); the 8-bit rule against the
    restatement on the downloaded phi, with the stated exception for rounding ties."""
    r = solved("pipelined-40x30x6")
    Nx, Ny, Nt, T = r["Nx"], r["Ny"], r["Nt"], r["T"]
    phi = r["phi"].reshape(Nt, Ny, Nx)
    assert R.max_dv(phi) < 0.5
    want = np.stack([R.interp(phi, r["u0"], r["u1"], s, 6, divisor=255.0) for s in T])
    print(f"max |float64 image difference| {np.abs(r['u8_f64'] - want).max():.3e}")
    np.testing.assert_allclose(r["u8_f64"], want, rtol=0, atol=1e-11)
    np.testing.assert_allclose(r["host"], np.stack([R.maps(phi, s, 6) for s in T]), rtol=1e-13, atol=1e-12)
    amb = R.u8_ambiguous(want)
    print(f"{int(amb.sum())} of {amb.size} reference pixels on an 8-bit rounding tie")
    assert amb.sum() <= 1e-4 * amb.size
    assert np.array_equal(r["u8"][~amb], R.to_u8(want)[~amb])


# ------------------------------------------------------------------ 4. no side effect

def _final(s):
    st = s.stats()
    return dict(crit=np.array(s.crit), cg=np.array(s.cg_its, dtype=np.float64), phi=s.phi(), state=s.state(),
                flow=s.flow(), path=s.flow_path(),
                counters=np.array([st["outer_iters"], st["cg_iters_total"], st["cg_redo"]], dtype=np.float64))


def _assert_same_tree(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        xs = a[k] if isinstance(a[k], tuple) else (a[k],)
        ys = b[k] if isinstance(b[k], tuple) else (b[k],)
        for x, y in zip(xs, ys):
            assert same(x, y), k


@pytest.mark.parametrize("name,straight", [("pipelined-40x30x6", True), ("two-shards-40x30x6", False)])
def test_no_side_effect(name, straight, monkeypatch):
    """Iterate 3, maps and in-betweens (host and device), iterate 3 more: everything is
    bit-identical to 6 iterations straight (the default loop) / to the same two calls without the
    exports in between (virtual ranks)."""
    monkeypatch.delenv("FOTO_PIPE", raising=False)
    Nx, Ny, Nt, opts = CONFIGS[name]
    f0, f1 = pair(Nx, Ny)
    c0, c1 = R.u8_frames(Ny, Nx, 3)
    mk = lambda: BBSolver(f0.ravel(), f1.ravel(), Nt, Nx, Ny, **opts)   # noqa: E731
    with mk() as s:
        s.iterate(3, stop_rules=False)
        before = s.flow()
        a = s.maps(times(Nt))
        assert same(a, s.maps_device(times(Nt), dtype="float64").to_numpy())
        x = s.interpolate(c0, c1, 7)
        assert same(x, s.interpolate(c0, c1, 7)) and same(a, s.maps(times(Nt)))     # two calls, the same bits
        for p, q in zip(before, s.flow()):
            assert same(p, q)
        s.iterate(3, stop_rules=False)
        touched = _final(s)
    with mk() as s:
        for n in ((6,) if straight else (3, 3)):
            s.iterate(n, stop_rules=False)
        plain = _final(s)
    assert len(plain["crit"]) == 6
    _assert_same_tree(touched, plain)


# ------------------------------------------------------------------ 5. rules

def test_rules_and_argument_errors():
    Nx, Ny, Nt = 37, 29, 5
    f0, f1 = pair(Nx, Ny)
    L = _lib.lib()
    E, S = _lib.FOTO_ERR_ARG, _lib.FOTO_ERR_STATE
    U8, F32, F64 = _lib.FOTO_U8, _lib.FOTO_F32, _lib.FOTO_F64
    T = np.array([0.0, 1.5, 4.0])
    K = len(T)
    fill = np.full((K, 4, Ny, Nx), 7.25)
    c0, c1 = R.smooth_frames(Ny, Nx, 3)
    P = ctypes.c_void_p
    with BBSolver(f0.ravel(), f1.ravel(), Nt, Nx, Ny, cg_mode=-1) as s:
        out = DeviceArray.from_numpy(fill)
        host = np.array(fill)
        big = DeviceArray.from_numpy(np.full((K + 2, Ny, Nx, 3), 7.25))       # frames and a target in one allocation
        big[0].copy_from(DeviceArray.from_numpy(c0))
        big[1].copy_from(DeviceArray.from_numpy(c1))
        a, b, C, sc0, sc1, _, _ = D.interp_frames(big[0], big[1])
        img = big[2:]
        img_fill = np.full((K, Ny, Nx, 3), 7.25)

        def maps(s_=T, count=K, it=6, o=None):
            return L.foto_bb_maps(s._ctx, _lib.dptr(s_) if s_ is not None else _lib._D(), count, it,
                                  _lib.dptr(host) if o is None else o)

        def maps_dev(s_=T, count=K, it=6, o=None, dt=F64):
            return L.foto_bb_maps_dev(s._ctx, _lib.dptr(s_) if s_ is not None else _lib._D(), count, it,
                                      P(out.ptr if o is None else o), dt, None)

        def interp(fa=a, fb=b, C_=3, s0=sc0, s1=sc1, s_=T, count=K, it=6, o=None, dt=F64):
            return L.foto_bb_interp_dev(s._ctx, ctypes.byref(fa) if fa is not None else None,
                                        ctypes.byref(fb) if fb is not None else None, C_, s0, s1,
                                        _lib.dptr(s_) if s_ is not None else _lib._D(), count, it,
                                        P(img.ptr if o is None else o), dt, None)

        # before any iteration
        assert maps() == S and maps_dev() == S and interp() == S
        with pytest.raises(_lib.FotoError):
            s.maps(T)
        s.iterate(2, stop_rules=False)
        # argument errors leave `out` untouched
        for bad in (np.array([0.0, -1e-300, 1.0]), np.array([0.0, 4.0 + 1e-12, 1.0]), np.array([np.nan, 1.0, 2.0]),
                    np.array([1.0, np.inf, 2.0])):
            assert maps(s_=bad) == E and maps_dev(s_=bad) == E and interp(s_=bad) == E
        for kw in (dict(s_=None), dict(count=0), dict(count=-1), dict(it=0), dict(it=65), dict(it=-2)):
            assert maps(**kw) == E and maps_dev(**kw) == E and interp(**kw) == E, kw
        assert maps(o=_lib._D()) == E and maps_dev(o=0) == E and interp(o=0) == E                 # null out
        assert maps_dev(dt=U8) == E and maps_dev(dt=3) == E and interp(dt=3) == E and interp(dt=-1) == E
        assert maps_dev(o=host.ctypes.data) == E and interp(o=img_fill.ctypes.data) == E           # host pointers
        assert maps_dev(o=out.ptr + 4) == E and maps_dev(o=out.ptr + 2, dt=F32) == E               # misaligned
        assert interp(o=img.ptr + 4) == E and interp(o=img.ptr + 1, dt=F32) == E
        assert maps_dev(count=K + 1, s_=np.array([0.0, 1.0, 2.0, 3.0])) == E                        # past the allocation
        assert interp(fa=None) == E and interp(fb=None) == E
        assert interp(C_=0) == E and interp(s0=0) == E and interp(s1=-3) == E
        hostim = _lib.Image(c0.ctypes.data, F64, 3 * Nx, 3, 1.0)
        assert interp(fa=hostim) == E and interp(fb=hostim) == E                                    # host frames
        for field, v in (("dtype", 5), ("stride_x", 0), ("divisor", 0.0), ("data", a.data + 4)):
            im = _lib.Image(a.data, a.dtype, a.stride_y, a.stride_x, a.divisor)
            setattr(im, field, v)
            assert interp(fb=im) == E, field
        assert interp(o=big[1].ptr, count=1) == E and interp(o=big[0].ptr + 8 * 3 * Nx * (Ny - 1), count=1) == E   # overlap
        assert same(out.to_numpy(), fill) and same(host, fill) and same(img.to_numpy(), img_fill)
        assert same(big[0].to_numpy(), c0) and same(big[1].to_numpy(), c1)
        # the context is as it was, and the same targets now receive the results
        assert maps() == 0 and maps_dev() == 0 and interp() == 0
        want = ops.maps_from_phi(s.phi(), Nt, Nx, Ny, T)
        assert same(host, want) and same(out.to_numpy(), want)
        assert same(img.to_numpy(), ops.interp_from_phi(s.phi(), Nt, Nx, Ny, c0, c1, T))
        # U8 and F32 targets of the in-between
        assert same(s.interpolate(big[0], big[1], T, dtype="float32").to_numpy(), img.to_numpy().astype(np.float32))
        with pytest.raises(ValueError):
            s.interpolate(c0[:-1], c1[:-1], T)


def test_callback_of_the_default_loop_sees_the_reported_iteration(monkeypatch):
    monkeypatch.delenv("FOTO_PIPE", raising=False)
    Nx, Ny, Nt = 40, 30, 6
    f0, f1 = pair(Nx, Ny)
    c0, c1 = R.smooth_frames(Ny, Nx)
    T = times(Nt)
    seen = {}
    with BBSolver(f0.ravel(), f1.ravel(), Nt, Nx, Ny, cg_mode=3) as s:
        def cb(i, crit, its, info):
            if i == 2:                      # the 3rd iteration; the 4th is already on the stream
                seen["host"] = s.maps(T)
                seen["dev"] = s.maps_device(T, dtype="float64").to_numpy()
                seen["img"] = s.interpolate(c0, c1, T)
                seen["phi"] = s.phi()
        s.iterate(5, stop_rules=False, callback=cb)
        final = s.phi()
    with BBSolver(f0.ravel(), f1.ravel(), Nt, Nx, Ny, cg_mode=3) as s:
        s.iterate(3, stop_rules=False)
        phi3 = s.phi()
        s.iterate(2, stop_rules=False)
        assert same(s.phi(), final)         # the calls from the callback changed nothing
    assert same(seen["phi"], phi3)
    want = ops.maps_from_phi(phi3, Nt, Nx, Ny, T)
    assert same(seen["host"], want) and same(seen["dev"], want)
    assert same(seen["img"], ops.interp_from_phi(phi3, Nt, Nx, Ny, c0, c1, T))


def test_callback_of_the_one_in_flight_loop_is_refused(monkeypatch):
    """FOTO_PIPE=0 (read when the context is made): the next solve overwrites phi, so the calls
    raise FotoError from the callback, and the solve finishes as one that made no call."""
    monkeypatch.setenv("FOTO_PIPE", "0")
    Nx, Ny, Nt = 40, 30, 6
    f0, f1 = pair(Nx, Ny)
    c0, c1 = R.smooth_frames(Ny, Nx)
    T = times(Nt)
    res, refused = [], []
    for call in (True, False):
        with BBSolver(f0.ravel(), f1.ravel(), Nt, Nx, Ny, cg_mode=3) as s:
            def cb(i, crit, its, info):
                if not call or i != 2:
                    return
                for fn in (lambda: s.maps(T), lambda: s.maps_device(T), lambda: s.interpolate(c0, c1, T)):
                    try:
                        fn()
                        refused.append(False)
                    except _lib.FotoError:
                        refused.append(True)
            s.iterate(5, stop_rules=False, callback=cb)
            res.append([np.array(s.crit), s.phi(), *s.state(), *s.flow(), s.maps(T)])
    assert refused == [True, True, True]
    for a, b in zip(*res):
        assert same(a, b)


# ------------------------------------------------------------------ 6. end to end

def test_inbetween_beats_crossfade_on_a_solved_pair():
    """A shifted blob, 32 x 24 x 6, solved with the stop rules on: at three interior times the
    in-between is closer (RMS) to the analytically shifted frame than the cross-fade a caller can
    make today, and the restatement on the same phi orders them the same way."""
    Nx, Ny, Nt = 32, 24, 6
    f0, f1, between = R.blob_pair(Ny, Nx, (3.0, 1.5))
    with BBSolver(f0.ravel(), f1.ravel(), Nt, Nx, Ny, r=1.0, reg_epsilon=1e-2, cg_mode=-1) as s:
        s.iterate(300, convergence_tol=0.05, stop_rules=True)
        T = [1.25, 2.5, 3.75]
        got = s.interpolate(f0, f1, T)
        phi = s.phi().reshape(Nt, Ny, Nx)
        print(f"{len(s.crit)} outer iterations, crit {s.crit[-1]:.4f}")
    for k, t in enumerate(T):
        w = t / (Nt - 1)
        rms = lambda x: 255.0 * float(np.sqrt(np.mean((x - between(w)) ** 2)))   # noqa: E731
        e_i, e_f, e_r = rms(got[k]), rms((1 - w) * f0 + w * f1), rms(R.interp(phi, f0, f1, t, 6))
        print(f"s = {t}: in-between RMS {e_i:.2f} grey levels, restatement {e_r:.2f}, cross-fade {e_f:.2f}")
        assert e_i < e_f and e_r < e_f


# ------------------------------------------------------------------ 7. stream order with torch

_TORCH_CHILD = r"""
import sys
sys.path[:0] = [{repo!r}, {pkg!r}, {tests!r}]
import torch                      # first: libfoto then binds to torch's HIP runtime
import numpy as np
import interp_ref as R
from foto import device
from foto.bb import BBSolver
from foto.synthetic import textured_pair

w, h, Nt = 37, 29, 5
f0, f1 = (np.round(f.reshape(h, w) * 255).astype(np.uint8) for f in textured_pair(w, h))
c0, c1 = R.u8_frames(h, w, 3)
t0, t1 = torch.from_numpy(f0).cuda(), torch.from_numpy(f1).cuda()
s0, s1 = torch.from_numpy(c0).cuda(), torch.from_numpy(c1).cuda()
side = torch.cuda.Stream()
big = torch.ones(1 << 24, device="cuda")
torch.cuda.synchronize()
T = [0.0, 1.25, 2.5, 4.0]
with BBSolver.from_device(t0, t1, Nt, cg_mode=-1) as s:
    s.iterate(3, stop_rules=False)
    want = s.interpolate(255 - c0, c1, T)      # what the stream below computes, from host frames
    wmaps = s.maps(T)
    with torch.cuda.stream(side):
        a = torch.zeros_like(s0)
        out = torch.full((len(T), h, w, 3), 9, dtype=torch.uint8, device="cuda")
        rec = torch.full((len(T), 4, h, w), -1.0, dtype=torch.float64, device="cuda")
        for _ in range(4):
            big = big * 1.0000001 + 0.0        # keeps the stream busy ahead of the producer
        a.copy_(255 - s0)                      # frame 0 is produced by a kernel on this stream
        out.fill_(7)
        assert s.interpolate(a, s1, T, out=out, stream=side) is out
        assert s.maps_device(T, out=rec, dtype="float64", stream=side) is rec
        a.fill_(0)                             # the input may be overwritten as soon as the call returns
        got = (out + 1).cpu().numpy()          # a consumer on the same stream, no host sync between
        gmaps = (rec + 1.0).cpu().numpy()
assert np.array_equal(got, want + 1)
assert np.array_equal(gmaps.view(np.uint64), (wmaps + 1.0).view(np.uint64))

# the one-shot on the cached context: the ends are the caller's frames
kw = dict(r=1.0, convergence_tol=0.0, reg_epsilon=1e-3, max_it=4)
mid = torch.as_tensor(device.bb_interpolate(t0, t1, Nt, 5, colour0=s0, colour1=s1, **kw), device="cuda").cpu().numpy()
assert mid.shape == (5, h, w, 3) and mid.dtype == np.uint8
assert np.array_equal(mid[0], c0) and np.array_equal(mid[-1], c1)
grey = torch.as_tensor(device.bb_interpolate(t0, t1, Nt, [0.0, 2.0, 4.0], dtype="float32", **kw), device="cuda").cpu().numpy()
assert grey.shape == (3, h, w) and np.array_equal(grey[0], (f0 / 255.0).astype(np.float32))
torch.cuda.synchronize()
print("TORCH CHILD OK")
"""


def test_torch_stream_order():
    if importlib.util.find_spec("torch") is None:
        pytest.skip("torch is not installed")
    code = _TORCH_CHILD.format(repo=REPO, pkg=PKG, tests=os.path.join(REPO, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, env=dict(os.environ))
    assert r.returncode == 0 and "TORCH CHILD OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
