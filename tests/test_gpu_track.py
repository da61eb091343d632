"""Point tracking on the GPU (include/foto.h: foto_bb_track / _dev, foto_track_from_phi;
BBSolver.track / track_device, ops.track_from_phi, foto.device.bb_track).

Checker.  The drop-in's host utils.reconstructTrajectory, which reproduces tests/golden/flow.npz
at pixel centres with == (test_dropin.test_reconstruct_trajectory_matches_flow), fed un, vn =
oracle.grad2_central(phi_n, Nx, Ny, "N"), truncated to the first n + 1 planes for record n - 1.
Bar: the project's own for this operator, rtol 1e-13 / atol 1e-12 (test_path_from_phi_golden);
the measured maximum relative difference is printed and expected to be 0.

One stated deviation (foto.h): Python's int(nan) / int(inf) raise, so the checker has no value
for a record whose point arrived at a non-finite position in an earlier step -- the hand-written
start (1e300, -1e300) does after its first step (its weights overflow; the record of that step
itself is nan in the checker and here alike).  For those records the library must return a
non-finite record; every record the checker does produce is compared at the bar above.

Everything else compares entries of this build with each other, bit for bit (np.array_equal on
the integer view): k_track and k_traj call one step function (traj_step, foto_devutil.h), so
these comparisons hold by construction and guard against the two being separated again.
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

import utils as U  # noqa: E402  (the drop-in: the host reconstructTrajectory)
from foto import _lib, ops  # noqa: E402
from foto.bb import BBSolver  # noqa: E402
from foto.device import DeviceArray  # noqa: E402
from foto.synthetic import textured_pair  # noqa: E402
from oracle import foto_oracle as O  # noqa: E402

ITS = 3

# test_gpu_path.py's four: the stencil CG, the pipelined loop, two shards, uneven slabs of 3 and 2
CONFIGS = {
    "stencil-37x29x5": (37, 29, 5, dict(cg_mode=-1)),
    "pipelined-40x30x6": (40, 30, 6, dict(cg_mode=3)),
    "sharded-40x30x6": (40, 30, 6, dict(cg_mode=3, virtual_ranks=2)),
    "uneven-7x6x5": (7, 6, 5, dict(cg_mode=0, virtual_ranks=2)),
}


def ibits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(ibits(a), ibits(b))


def pair(w, h, seed=0):
    a, b = textured_pair(w, h, seed=seed)
    return a.reshape(h, w), b.reshape(h, w)


def hand_points(Nx, Ny):
    return [(0, 0), (Nx - 1, Ny - 1), (Nx - 1 - 1e-12, 0.5), (-0.0, -0.0), (-0.999, 2), (Nx - 2, Ny - 2),
            (1e300, -1e300)]


def points(Nx, Ny, M, seed):
    """M random starts in [-3, Nx + 2] x [-3, Ny + 2] followed by the hand-written list."""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(-3, Nx + 2, M), rng.uniform(-3, Ny + 2, M)], axis=1)
    return np.concatenate([p, np.array(hand_points(Nx, Ny), dtype=np.float64)])


def pixel_centres(Nx, Ny):
    jj, ii = np.meshgrid(np.arange(Ny), np.arange(Nx), indexing="ij")
    return np.stack([ii.ravel(), jj.ravel()], axis=1).astype(np.float64)     # row j * Nx + i = (i, j)


def checker(phi, Nt, Nx, Ny, pts):
    """(records [Nt-1][M][2], raised [Nt-1][M]): reconstructTrajectory per point and record;
    raised marks the records for which int() of a non-finite position raised."""
    nxy = Nx * Ny
    un, vn = np.zeros((Nt, nxy)), np.zeros((Nt, nxy))
    for n in range(Nt):
        g = O.grad2_central(phi[n * nxy:(n + 1) * nxy], Nx, Ny, "N")
        un[n], vn[n] = g[:nxy], g[nxy:]
    out = np.full((Nt - 1, len(pts), 2), np.nan)
    raised = np.zeros((Nt - 1, len(pts)), dtype=bool)
    with np.errstate(all="ignore"):
        for n in range(1, Nt):
            for k, (x, y) in enumerate(pts):
                try:
                    out[n - 1, k] = U.reconstructTrajectory(x, y, un[:n + 1], vn[:n + 1], Nx, Ny, n + 1)
                except (ValueError, OverflowError):
                    raised[n - 1, k] = True
    return out, raised


# ------------------------------------------------------------------ 1. the reference's fixture

@pytest.mark.parametrize("f", range(4))
def test_track_from_phi_golden(gold, f):
    d = gold("flow.npz")
    Nt, Ny, Nx = (int(s) for s in d[f"f{f}_shape"])
    phi = d[f"f{f}_phi"]
    P = points(Nx, Ny, 300, seed=100 + f)
    got = ops.track_from_phi(phi, Nt, Nx, Ny, P)
    assert got.shape == (Nt - 1, len(P), 2) and got.dtype == np.float64
    want, raised = checker(phi, Nt, Nx, Ny, P)
    # only the (1e300, -1e300) start may leave the checker without a value, and only after step 1
    assert not raised[:, :-1].any() and not raised[0].any()
    assert np.isfinite(want[:, :-1]).all()
    ok = ~raised
    with np.errstate(all="ignore"):
        diff = np.abs(got[ok] - want[ok])
        rel = diff / np.maximum(np.abs(want[ok]), 1e-300)
    fin = np.isfinite(want[ok])
    print(f"case {f} ({Nt}x{Ny}x{Nx}): {int(ok.sum())} records x points compared, largest |displacement| "
          f"{np.abs(want[ok][fin]).max():.3e}, max relative difference {rel[fin].max():.3e}")
    np.testing.assert_allclose(got[ok], want[ok], rtol=1e-13, atol=1e-12)
    assert not np.isfinite(got[raised]).all(axis=-1).any()        # the stated deviation
    last = ops.track_from_phi(phi, Nt, Nx, Ny, P, all_steps=False)
    assert last.shape == (1, len(P), 2) and same(last[0], got[-1])


# ------------------------------------------------------------------ 2. pixel centres

def _centres_equal_flow_path(phi, Nt, Nx, Ny):
    got = ops.track_from_phi(phi, Nt, Nx, Ny, pixel_centres(Nx, Ny))
    u, v, _ = ops.flow_path_from_phi(phi, Nt, Nx, Ny)
    assert same(got[..., 0], u) and same(got[..., 1], v)
    fu, fv, _ = ops.flow_from_phi(phi, Nt, Nx, Ny)
    assert same(got[-1, :, 0], fu) and same(got[-1, :, 1], fv)


def test_pixel_centres_equal_flow_path(gold):
    d = gold("flow.npz")
    for f in range(4):
        Nt, Ny, Nx = (int(s) for s in d[f"f{f}_shape"])
        _centres_equal_flow_path(d[f"f{f}_phi"], Nt, Nx, Ny)
    # 2 x 2 x 2: tx and ty clamp to 0, every un / vn is an edge zero
    _centres_equal_flow_path(np.random.default_rng(5).standard_normal(8), 2, 2, 2)


# test_gpu_path.NARROW: both edge selections on adjacent taps, both extra loads clamped
@pytest.mark.parametrize("Nt,Nx,Ny", [(3, 2, 5), (3, 5, 2), (4, 3, 2)])
def test_pixel_centres_equal_flow_path_narrow(Nt, Nx, Ny):
    phi = np.random.default_rng(1000 * Nt + 10 * Nx + Ny).standard_normal(Nt * Nx * Ny)
    _centres_equal_flow_path(phi, Nt, Nx, Ny)


# ------------------------------------------------------------------ 3. block edges

def test_block_edges():
    Nx, Ny, Nt = 37, 29, 5
    phi = np.random.default_rng(7).standard_normal(Nt * Nx * Ny)
    P = points(Nx, Ny, 1000 - 7, seed=8)
    assert len(P) == 1000
    full = ops.track_from_phi(phi, Nt, Nx, Ny, P)
    last = ops.track_from_phi(phi, Nt, Nx, Ny, P, all_steps=False)
    assert same(last[0], full[-1])
    for M in (1, 255, 256, 257):
        assert same(ops.track_from_phi(phi, Nt, Nx, Ny, P[:M]), full[:, :M]), M
        assert same(ops.track_from_phi(phi, Nt, Nx, Ny, P[:M], all_steps=False), last[:, :M]), M


# ------------------------------------------------------------------ 4. the context

_solved = {}


def solved(name):
    """One solve per configuration (3 iterations, no stop rules) and everything the tests compare,
    computed once and left unchanged."""
    if name in _solved:
        return _solved[name]
    Nx, Ny, Nt, opts = CONFIGS[name]
    f0, f1 = pair(Nx, Ny)
    # two blocks; without the (1e300, -1e300) start, which float32 cannot hold (non-finite rows:
    # test_non_finite_points_touch_only_their_rows)
    P = points(Nx, Ny, 500, seed=11)[:-1]
    P32 = P.astype(np.float32)
    r = dict(Nx=Nx, Ny=Ny, Nt=Nt, P=P, P32=P32)
    with BBSolver(f0.ravel(), f1.ravel(), Nt, Nx, Ny, **opts) as s:
        s.iterate(ITS, stop_rules=False)
        r["phi"], r["flow"], r["path"] = s.phi(), s.flow(), s.flow_path()
        r["host"] = s.track(P)
        r["host_last"] = s.track(P, all_steps=False)
        r["one"] = s.track(P[3])
        r["centres"] = s.track(pixel_centres(Nx, Ny))
        dP, dP32 = DeviceArray.from_numpy(P), DeviceArray.from_numpy(P32)
        r["dev64"] = s.track_device(dP, dtype="float64").to_numpy()
        r["dev32"] = s.track_device(dP).to_numpy()
        r["dev64_last"] = s.track_device(dP, dtype="float64", all_steps=False).to_numpy()
        r["dev32_last"] = s.track_device(dP, all_steps=False).to_numpy()
        r["in32_dev64"] = s.track_device(dP32, dtype="float64").to_numpy()
        r["in32_dev32"] = s.track_device(dP32, dtype="float32").to_numpy()
        r["in32_host"] = s.track(np.float64(P32))
        mine = DeviceArray((Nt - 1, len(P), 2), np.float64)          # a caller-owned target
        assert s.track_device(dP, out=mine, dtype="float64") is mine
        r["mine"] = mine.to_numpy()
        r["flow_after"] = s.flow()
    _solved[name] = r
    return r


@pytest.mark.parametrize("name", list(CONFIGS))
def test_track_context(name):
    r = solved(name)
    Nx, Ny, Nt, P = r["Nx"], r["Ny"], r["Nt"], r["P"]
    host = r["host"]
    assert host.shape == (Nt - 1, len(P), 2) and host.dtype == np.float64
    # the context's records (virtual ranks: one launch per shard, the positions carried between
    # them) == the single-grid test entry on the gathered phi
    assert same(host, ops.track_from_phi(r["phi"], Nt, Nx, Ny, P))
    assert same(r["host_last"], host[-1:])
    assert r["one"].shape == (Nt - 1, 1, 2) and same(r["one"], host[:, 3:4])
    assert same(r["dev64"], host) and same(r["mine"], host)
    assert same(r["dev32"], host.astype(np.float32))
    assert same(r["dev64_last"], host[-1:]) and same(r["dev32_last"], host[-1:].astype(np.float32))
    assert same(r["in32_dev64"], r["in32_host"])
    assert same(r["in32_dev32"], r["in32_host"].astype(np.float32))
    # pixel centres: the bits of flow_path()'s (u, v); the last record those of flow()
    u, v, _ = r["path"]
    assert same(r["centres"][..., 0], u) and same(r["centres"][..., 1], v)
    assert same(r["centres"][-1, :, 0], r["flow"][0]) and same(r["centres"][-1, :, 1], r["flow"][1])
    for a, b in zip(r["flow"], r["flow_after"]):       # flow() has the same bits after track
        assert same(a, b)
    assert np.isfinite(host).all()


# ------------------------------------------------------------------ 5. no side effect

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


@pytest.mark.parametrize("name,straight", [("pipelined-40x30x6", True), ("sharded-40x30x6", False)])
def test_track_has_no_side_effect(name, straight, monkeypatch):
    """Iterate 3, track (host and device), iterate 3 more: everything is bit-identical to 6
    iterations straight (the default loop) / to the same two calls without the tracking in
    between (virtual ranks, where the scratch of the running positions is used as well)."""
    monkeypatch.delenv("FOTO_PIPE", raising=False)
    Nx, Ny, Nt, opts = CONFIGS[name]
    f0, f1 = pair(Nx, Ny)
    P = points(Nx, Ny, 300, seed=13)
    mk = lambda: BBSolver(f0.ravel(), f1.ravel(), Nt, Nx, Ny, **opts)   # noqa: E731
    with mk() as s:
        s.iterate(3, stop_rules=False)
        before = s.flow()
        a = s.track(P)
        b = s.track_device(DeviceArray.from_numpy(P), dtype="float64").to_numpy()
        assert same(a, b)
        for x, y in zip(before, s.flow()):
            assert same(x, y)
        s.iterate(3, stop_rules=False)
        touched = _final(s)
    with mk() as s:
        for n in ((6,) if straight else (3, 3)):
            s.iterate(n, stop_rules=False)
        plain = _final(s)
    assert len(plain["crit"]) == 6
    _assert_same_tree(touched, plain)


# ------------------------------------------------------------------ 6. rules

def _raw(L, s, P, out, all_steps=1):
    return L.foto_bb_track(s._ctx, _lib.dptr(P), len(P), all_steps, _lib.dptr(out))


def _raw_dev(L, s, pts, pcode, M, all_steps, out, dcode):
    return L.foto_bb_track_dev(s._ctx, ctypes.c_void_p(pts), pcode, M, all_steps, ctypes.c_void_p(out), dcode, None)


def test_rules_and_argument_errors():
    Nx, Ny, Nt = 37, 29, 5
    f0, f1 = pair(Nx, Ny)
    L = _lib.lib()
    E, S = _lib.FOTO_ERR_ARG, _lib.FOTO_ERR_STATE
    F32, F64 = _lib.FOTO_F32, _lib.FOTO_F64
    P = points(Nx, Ny, 20, seed=17)
    M = len(P)
    fill = np.full((Nt - 1, M, 2), 7.25)
    with BBSolver(f0.ravel(), f1.ravel(), Nt, Nx, Ny, cg_mode=-1) as s:
        dP = DeviceArray.from_numpy(P)
        out = DeviceArray.from_numpy(fill)
        host = np.array(fill)
        # before any iteration
        assert _raw(L, s, P, host) == S
        assert _raw_dev(L, s, dP.ptr, F64, M, 1, out.ptr, F64) == S
        with pytest.raises(_lib.FotoError):
            s.track(P)
        s.iterate(2, stop_rules=False)
        # argument errors leave `out` untouched
        assert _raw_dev(L, s, dP.ptr, F64, M, 1, host.ctypes.data, F64) == E      # a host pointer as out
        assert _raw_dev(L, s, P.ctypes.data, F64, M, 1, out.ptr, F64) == E        # a host pointer as pts
        assert _raw_dev(L, s, 0, F64, M, 1, out.ptr, F64) == E
        assert _raw_dev(L, s, dP.ptr, F64, M, 1, 0, F64) == E
        assert _raw_dev(L, s, dP.ptr, F64, 0, 1, out.ptr, F64) == E
        assert _raw_dev(L, s, dP.ptr, F64, -5, 1, out.ptr, F64) == E
        assert _raw_dev(L, s, dP.ptr, F64, 2 ** 31, 1, out.ptr, F64) == E
        assert _raw_dev(L, s, dP.ptr, F64, M, 2, out.ptr, F64) == E
        assert _raw_dev(L, s, dP.ptr, F64, M, -1, out.ptr, F64) == E
        assert _raw_dev(L, s, dP.ptr, _lib.FOTO_U8, M, 1, out.ptr, F64) == E
        assert _raw_dev(L, s, dP.ptr, F64, M, 1, out.ptr, _lib.FOTO_U8) == E
        assert _raw_dev(L, s, dP.ptr, F64, M, 1, out.ptr, 3) == E
        assert _raw_dev(L, s, dP.ptr + 8, F64, M - 1, 1, out.ptr, F64) == E       # not on an (x, y) pair
        assert _raw_dev(L, s, dP.ptr, F64, M, 1, out.ptr + 8, F64) == E
        assert _raw_dev(L, s, dP.ptr, F32, M, 1, out.ptr + 4, F32) == E
        assert _raw_dev(L, s, dP.ptr, F64, M + 1, 1, out.ptr, F64) == E           # one point past both allocations
        assert _raw(L, s, P, host, all_steps=2) == E
        assert L.foto_bb_track(s._ctx, _lib._D(), M, 1, _lib.dptr(host)) == E
        assert L.foto_bb_track(s._ctx, _lib.dptr(P), 0, 1, _lib.dptr(host)) == E
        assert same(out.to_numpy(), fill) and same(host, fill)
        # the context is as it was, and the same target now receives the records
        want = ops.track_from_phi(s.phi(), Nt, Nx, Ny, P)
        assert s.track_device(dP, out=out, dtype="float64") is out
        assert same(out.to_numpy(), want) and same(s.track(P), want)


def test_non_finite_points_touch_only_their_rows():
    Nx, Ny, Nt = 37, 29, 5
    f0, f1 = pair(Nx, Ny)
    P = points(Nx, Ny, 293, seed=19)[:-1]          # (without the 1e300 start)
    bad = {5: (np.nan, 3.0), 64: (2.0, np.inf), 255: (-np.inf, np.nan), 256: (np.inf, -np.inf), 298: (np.nan, np.nan)}
    Q = P.copy()
    for k, p in bad.items():
        Q[k] = p
    rows = sorted(bad)
    keep = np.setdiff1d(np.arange(len(P)), rows)
    with BBSolver(f0.ravel(), f1.ravel(), Nt, Nx, Ny, cg_mode=-1) as s:
        s.iterate(2, stop_rules=False)
        clean = s.track(P)
        out = np.empty_like(clean)
        assert _raw(_lib.lib(), s, Q, out) == 0                     # never an error
        dev32 = s.track_device(DeviceArray.from_numpy(Q.astype(np.float32))).to_numpy()
        clean32 = s.track_device(DeviceArray.from_numpy(P.astype(np.float32))).to_numpy()
        last = s.track(Q, all_steps=False)
    assert np.isfinite(clean).all()
    assert same(out[:, keep], clean[:, keep]) and same(dev32[:, keep], clean32[:, keep])
    assert not np.isfinite(out[:, rows]).all(axis=-1).any()
    assert not np.isfinite(dev32[:, rows]).all(axis=-1).any()
    assert same(last[:, keep], clean[-1:, keep]) and not np.isfinite(last[:, rows]).all(axis=-1).any()


def test_callback_of_the_default_loop_sees_the_reported_iteration(monkeypatch):
    monkeypatch.delenv("FOTO_PIPE", raising=False)
    Nx, Ny, Nt = 40, 30, 6
    f0, f1 = pair(Nx, Ny)
    P = points(Nx, Ny, 100, seed=23)
    seen = {}
    with BBSolver(f0.ravel(), f1.ravel(), Nt, Nx, Ny, cg_mode=3) as s:
        dP = DeviceArray.from_numpy(P)

        def cb(i, crit, its, info):
            if i == 2:                      # the 3rd iteration; the 4th is already on the stream
                seen["host"] = s.track(P)
                seen["dev"] = s.track_device(dP, dtype="float64").to_numpy()
                seen["phi"] = s.phi()
        s.iterate(5, stop_rules=False, callback=cb)
        final = s.phi()
    with BBSolver(f0.ravel(), f1.ravel(), Nt, Nx, Ny, cg_mode=3) as s:
        s.iterate(3, stop_rules=False)
        phi3 = s.phi()
        s.iterate(2, stop_rules=False)
        assert same(s.phi(), final)         # the calls from the callback changed nothing
    assert same(seen["phi"], phi3)
    want = ops.track_from_phi(phi3, Nt, Nx, Ny, P)
    assert same(seen["host"], want) and same(seen["dev"], want)


def test_callback_of_the_one_in_flight_loop_is_refused(monkeypatch):
    """FOTO_PIPE=0 (read when the context is made): the next solve overwrites phi, so both calls
    raise FotoError from the callback, and the solve finishes as one that made no call."""
    monkeypatch.setenv("FOTO_PIPE", "0")
    Nx, Ny, Nt = 40, 30, 6
    f0, f1 = pair(Nx, Ny)
    P = points(Nx, Ny, 100, seed=29)
    res, refused = [], []
    for call in (True, False):
        with BBSolver(f0.ravel(), f1.ravel(), Nt, Nx, Ny, cg_mode=3) as s:
            dP = DeviceArray.from_numpy(P)

            def cb(i, crit, its, info):
                if not call or i != 2:
                    return
                for fn in (lambda: s.track(P), lambda: s.track_device(dP)):
                    try:
                        fn()
                        refused.append(False)
                    except _lib.FotoError:
                        refused.append(True)
            s.iterate(5, stop_rules=False, callback=cb)
            res.append([np.array(s.crit), s.phi(), *s.state(), *s.flow(), s.track(P)])
    assert refused == [True, True]
    for a, b in zip(*res):
        assert same(a, b)


# ------------------------------------------------------------------ 7. stream order with torch

_TORCH_CHILD = r"""
import sys
sys.path[:0] = [{repo!r}, {pkg!r}]
import torch                      # first: libfoto then binds to torch's HIP runtime
import numpy as np
from foto import device
from foto.bb import BBSolver
from foto.synthetic import textured_pair

w, h, Nt, M = 37, 29, 5, 1000
f0, f1 = (np.round(f.reshape(h, w) * 255).astype(np.uint8) for f in textured_pair(w, h))
t0, t1 = torch.from_numpy(f0).cuda(), torch.from_numpy(f1).cuda()
rng = np.random.default_rng(3)
base = np.stack([rng.uniform(0, w - 1, M), rng.uniform(0, h - 1, M)], axis=1).astype(np.float32)
side = torch.cuda.Stream()
big = torch.ones(1 << 24, device="cuda")
tb = torch.from_numpy(base).cuda()
torch.cuda.synchronize()
with BBSolver.from_device(t0, t1, Nt, cg_mode=-1) as s:
    s.iterate(3, stop_rules=False)
    P32 = base * np.float32(0.5) + np.float32(1.25)        # what the stream below computes
    want = s.track(np.float64(P32))
    with torch.cuda.stream(side):
        pts = torch.full((M, 2), -1.0, dtype=torch.float32, device="cuda")
        rec = torch.full((Nt - 1, M, 2), -1.0, dtype=torch.float64, device="cuda")
        for _ in range(4):
            big = big * 1.0000001 + 0.0        # keeps the stream busy ahead of the producer
        pts.copy_(tb * 0.5 + 1.25)             # the points are produced by a kernel on this stream
        rec.fill_(-2.0)
        assert s.track_device(pts, out=rec, dtype="float64", stream=side) is rec
        pts.fill_(0.0)                         # the input may be overwritten as soon as the call returns
        rec2 = rec + 1.0                       # a consumer on the same stream, no host sync between
        got = rec2.cpu().numpy()               # (.cpu() waits on the side stream)
assert np.array_equal(got.view(np.uint64), (want + 1.0).view(np.uint64))

# the one-shot on the cached context: the last record is where bb_flow moves each point
kw = dict(r=1.0, convergence_tol=0.0, reg_epsilon=1e-3, max_it=4)
pts = torch.from_numpy(P32).cuda()
path = torch.as_tensor(device.bb_track(t0, t1, Nt, pts, dtype="float64", **kw), device="cuda").cpu().numpy()
end = torch.as_tensor(device.bb_track(t0, t1, Nt, pts, dtype="float64", all_steps=False, **kw), device="cuda").cpu().numpy()
assert path.shape == (Nt - 1, M, 2) and end.shape == (1, M, 2)
assert np.array_equal(path[-1].view(np.uint64), end[0].view(np.uint64))
f32 = torch.as_tensor(device.bb_track(t0, t1, Nt, pts, **kw), device="cuda").cpu().numpy()
assert f32.dtype == np.float32 and np.array_equal(f32.view(np.uint32), path.astype(np.float32).view(np.uint32))
torch.cuda.synchronize()
print("TORCH CHILD OK")
"""


def test_torch_stream_order():
    if importlib.util.find_spec("torch") is None:
        pytest.skip("torch is not installed")
    code = _TORCH_CHILD.format(repo=REPO, pkg=PKG)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, env=dict(os.environ))
    assert r.returncode == 0 and "TORCH CHILD OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
