"""The transport path on the GPU (include/foto.h: foto_bb_frames / _dev, foto_bb_flow_path / _dev,
foto_flow_path_from_phi; BBSolver.frames / frames_device / flow_path / flow_path_device).

Bars.  Against the reference (the CPU oracle's flow_from_phi on the first n + 1 planes of the
golden phi): test_flow's rtol 1e-13 / atol 1e-12.  Everything else compares entries of this build
with each other and is bit for bit (np.array_equal on the integer view): the path runs k_traj one
step at a time from the stored positions and finishes each record with k_flow_record, the kernel
that finishes foto_bb_flow's, so its last record has foto_bb_flow's bits by construction; an
integer frame position with scale 1 copies the plane.  A fractional position is one rounding of 1 - w, two
products and one sum, at most 4 half-ulps of the largest term with or without FMA contraction:
|got - ((1 - w) a + w b)| <= 2^-50 max(|a|, |b|).

"Sharded equals unsharded" is checked on the same data: a virtual_ranks = 2 context's exports,
whose planes and steps come from two shards, against the single-grid entries
(ops.flow_path_from_phi, the planes of state()) fed that context's gathered phi and mu.  Two
separate solves, one sharded and one not, differ at the CG's rtol (per-rank partial sums change
the reduction order: test_gpu_parity.test_bb_virtual_ranks_match_single), so their paths can
agree only to that bar.
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

from foto import _lib, ops  # noqa: E402
from foto.bb import BBSolver  # noqa: E402
from foto.device import DeviceArray  # noqa: E402
from foto.synthetic import textured_pair  # noqa: E402
from oracle import foto_oracle as O  # noqa: E402

ITS = 3

# (Nx, Ny, Nt, options): the stencil CG, the pipelined loop, two shards, uneven slabs of 3 and 2
CONFIGS = {
    "stencil-37x29x5": (37, 29, 5, dict(cg_mode=-1)),
    "pipelined-40x30x6": (40, 30, 6, dict(cg_mode=3)),
    "sharded-40x30x6": (40, 30, 6, dict(cg_mode=3, virtual_ranks=2)),
    "uneven-7x6x5": (7, 6, 5, dict(cg_mode=0, virtual_ranks=2)),
}
# frames only: 33 x 5, odd, and a uint8 frame (165 bytes) ends off every 16-byte boundary
FRAME_CONFIGS = dict(CONFIGS, **{"narrow-33x5x4": (33, 5, 4, dict(cg_mode=-1))})


def ibits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(ibits(a), ibits(b))


def pair(w, h, seed=0):
    a, b = textured_pair(w, h, seed=seed)
    return a.reshape(h, w), b.reshape(h, w)


def frac_positions(Nt):
    return [0.25, 1.5, Nt - 1 - 1e-9]


_solved = {}


def solved(name):
    """One solve per configuration (3 iterations, no stop rules) and everything the tests compare,
    computed once and left unchanged."""
    if name in _solved:
        return _solved[name]
    Nx, Ny, Nt, opts = FRAME_CONFIGS[name]
    f0, f1 = pair(Nx, Ny)
    r = dict(Nx=Nx, Ny=Ny, Nt=Nt)
    with BBSolver(f0.ravel(), f1.ravel(), Nt, Nx, Ny, **opts) as s:
        r["frames0"] = s.frames(Nt)                        # before any iteration
        s.iterate(ITS, stop_rules=False)
        r["phi"], r["mu"], r["flow"] = s.phi(), s.state()[0], s.flow()
        r["path"] = s.flow_path()
        r["path64"] = s.flow_path_device(dtype="float64").to_numpy()
        r["path32"] = s.flow_path_device(dtype="float32", layout="planar").to_numpy()
        r["pathi64"] = s.flow_path_device(dtype="float64", layout="interleaved").to_numpy()
        r["pathi32"] = s.flow_path_device(layout="interleaved").to_numpy()
        mine = DeviceArray((Nt - 1, 3, Ny, Nx), np.float64)   # a caller-owned target
        assert s.flow_path_device(out=mine, dtype="float64") is mine
        r["path_mine"] = mine.to_numpy()
        r["flow_after"] = s.flow()
        pos = list(range(Nt)) + frac_positions(Nt)
        r["pos"] = np.array(pos, dtype=np.float64)
        r["fr"] = s.frames(pos)
        r["fr64"] = s.frames_device(pos, dtype="float64").to_numpy()
        r["fr32"] = s.frames_device(pos).to_numpy()
        r["fr8"] = s.frames_device(pos, scale=1.7, dtype="uint8").to_numpy()
        r["fr_scaled"] = s.frames(pos, scale=1.7)
        r["fr_k"] = s.frames(4)
        r["fr_lin"] = s.frames(np.linspace(0, Nt - 1, 4))
    _solved[name] = r
    return r


# ------------------------------------------------------------------ 1. the reference's fixture

def _records_match_oracle(phi, Nt, Nx, Ny, label):
    """Record n - 1 of foto_flow_path_from_phi against the oracle's flow of the first n + 1
    planes; the last record has foto_flow_from_phi's bits.  Returns the records."""
    u, v, m = ops.flow_path_from_phi(phi, Nt, Nx, Ny)
    assert u.shape == v.shape == m.shape == (Nt - 1, Nx * Ny)
    for n in range(1, Nt):
        ref = O.flow_from_phi(phi[:(n + 1) * Nx * Ny], n + 1, Nx, Ny)
        for got, want, name in zip((u, v, m), ref, "uvm"):
            assert np.isfinite(want).all()
            err = np.abs(got[n - 1] - want).max()
            print(f"{label} ({Nt}x{Ny}x{Nx}) record {n - 1} {name}: max |diff| {err:.3e}")
            np.testing.assert_allclose(got[n - 1], want, rtol=1e-13, atol=1e-12)
    for got, want in zip((u, v, m), ops.flow_from_phi(phi, Nt, Nx, Ny)):
        assert same(got[-1], want)
    return u, v, m


def test_path_from_phi_golden(gold):
    """Every intermediate step of the four cases has positions outside the frame: truncation,
    clamp and extrapolation.  Case 2 has one record."""
    d = gold("flow.npz")
    for f in range(4):
        Nt, Ny, Nx = (int(s) for s in d[f"f{f}_shape"])
        uvm = _records_match_oracle(d[f"f{f}_phi"], Nt, Nx, Ny, f"case {f}")
        for got, key in zip(uvm, "uvm"):
            np.testing.assert_allclose(got[-1], d[f"f{f}_{key}"], rtol=1e-13, atol=1e-12)


# (Nt, Nx, Ny): two columns / two rows -- every un / vn tap is an edge zero on that axis, both
# edge selections fall on adjacent taps and both extra loads of the step are clamped
NARROW = [(3, 2, 5), (3, 5, 2), (4, 3, 2)]


@pytest.mark.parametrize("Nt,Nx,Ny", NARROW)
def test_path_from_phi_narrow(Nt, Nx, Ny):
    """The trajectory step on the narrowest grids, anchored to the reference (random-normal phi:
    positions leave the frame at once)."""
    phi = np.random.default_rng(1000 * Nt + 10 * Nx + Ny).standard_normal(Nt * Nx * Ny)
    _records_match_oracle(phi, Nt, Nx, Ny, "narrow")


# ------------------------------------------------------------------ 2. the path on a context

@pytest.mark.parametrize("name", list(CONFIGS))
def test_flow_path_context(name):
    r = solved(name)
    Nx, Ny, Nt = r["Nx"], r["Ny"], r["Nt"]
    u, v, m = r["path"]
    assert u.shape == (Nt - 1, Nx * Ny)
    # the context's path (steps from whichever shard owns the plane) == the single-grid entry on
    # the gathered phi; its last record == flow(), and flow() is what it was before
    for got, want in zip((u, v, m), ops.flow_path_from_phi(r["phi"], Nt, Nx, Ny)):
        assert same(got, want)
    for got, want, again in zip((u, v, m), r["flow"], r["flow_after"]):
        assert same(got[-1], want) and same(again, want)
    host = np.stack([u, v, m], axis=1).reshape(Nt - 1, 3, Ny, Nx)
    assert same(r["path64"], host) and same(r["path_mine"], host)
    assert same(r["path32"], host.astype(np.float32))
    inter = np.stack([u, v], axis=-1).reshape(Nt - 1, Ny, Nx, 2)
    assert same(r["pathi64"], inter)
    assert same(r["pathi32"], inter.astype(np.float32))


def test_sharded_and_unsharded_solves_agree_to_cg_rtol():
    """Two separate solves (see the module docstring): the bar of
    test_bb_virtual_ranks_match_single's flow comparison, atol 1e-6."""
    a, b = solved("pipelined-40x30x6"), solved("sharded-40x30x6")
    for x, y, name in zip(a["path"], b["path"], "uvm"):
        print(f"{name}: max |sharded - unsharded| {np.abs(x - y).max():.3e}")
        np.testing.assert_allclose(y, x, rtol=0, atol=1e-6)


# ------------------------------------------------------------------ 3. frames

@pytest.mark.parametrize("name", list(FRAME_CONFIGS))
def test_frames_context(name):
    r = solved(name)
    Nx, Ny, Nt = r["Nx"], r["Ny"], r["Nt"]
    nxy = Nx * Ny
    planes = r["mu"][:Nt * nxy].reshape(Nt, Ny, Nx)
    fr = r["fr"]
    assert fr.shape == (Nt + 3, Ny, Nx)
    assert same(fr[:Nt], planes)                      # integer positions, scale 1: the planes
    for k, s in enumerate(frac_positions(Nt)):
        n = min(int(s), Nt - 2)
        w = s - n
        a, b = planes[n], planes[n + 1]
        err = np.abs(fr[Nt + k] - ((1 - w) * a + w * b))
        bound = 2.0 ** -50 * np.maximum(np.abs(a), np.abs(b))
        print(f"s = {s!r}: max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert np.all(err <= bound)
    assert same(r["fr64"], fr)
    assert same(r["fr32"], fr.astype(np.float32))
    sc = r["fr_scaled"]
    assert same(sc[:Nt], 1.7 * planes)                # the multiply by scale comes last
    assert same(r["fr8"], np.uint8(255 * np.clip(sc, 0, 1) + 0.5))
    assert r["fr8"].max() == 255                      # (the clip is exercised)
    assert same(r["fr_k"], r["fr_lin"]) and r["fr_k"].shape == (4, Ny, Nx)
    # before any iteration: the linear initial path of benamou_brenier.py:193-194
    f0, f1 = pair(Nx, Ny)
    init = np.stack([(1 - n / (Nt - 1)) * f0 + (n / (Nt - 1)) * f1 for n in range(Nt)])
    assert same(r["frames0"], init)


@pytest.mark.parametrize("name", ["stencil-37x29x5", "sharded-40x30x6", "narrow-33x5x4"])
def test_frames_uint8_round_trip(name):
    """Before any iteration planes 0 and Nt - 1 are the two frames: u8 pixels ingested with
    divisor 255 come back exactly, also through normalize = 1 with the frame-0 sum as scale."""
    Nx, Ny, Nt, opts = FRAME_CONFIGS[name]
    i0, i1 = (np.round(f * 255).astype(np.uint8) for f in pair(Nx, Ny))
    i0[0, :4] = (0, 49, 254, 255)
    d0, d1 = DeviceArray.from_numpy(i0), DeviceArray.from_numpy(i1)
    with BBSolver.from_device(d0, d1, Nt, **opts) as s:
        got = s.frames_device([0, Nt - 1], dtype="uint8").to_numpy()
    assert same(got, np.stack([i0, i1]))
    with BBSolver.from_device(d0, d1, Nt, normalize=True, **opts) as s:
        got = s.frames_device([0], scale=s.sums[0], dtype="uint8").to_numpy()
        f64 = s.frames([0], scale=s.sums[0])
    assert same(got[0], i0)
    np.testing.assert_allclose(f64[0], i0 / 255.0, rtol=4 * 2.0 ** -53, atol=0)


# ------------------------------------------------------------------ 4. no side effect

def _exports(s):
    Nt = s.Nt
    return dict(fr=s.frames(Nt), fr32=s.frames_device([0.5, Nt - 1.0]).to_numpy(), path=s.flow_path(),
                path32=s.flow_path_device().to_numpy())


def _final(s):
    return dict(crit=np.array(s.crit), cg=np.array(s.cg_its), phi=s.phi(), state=s.state(), flow=s.flow())


def _assert_same_tree(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        xs = a[k] if isinstance(a[k], tuple) else (a[k],)
        ys = b[k] if isinstance(b[k], tuple) else (b[k],)
        for x, y in zip(xs, ys):
            assert same(x, y), k


def test_exports_have_no_side_effect(monkeypatch):
    monkeypatch.delenv("FOTO_PIPE", raising=False)
    Nx, Ny, Nt = 40, 30, 6
    f0, f1 = pair(Nx, Ny)
    mk = lambda: BBSolver(f0.ravel(), f1.ravel(), Nt, Nx, Ny, cg_mode=3)   # noqa: E731
    seen = {}
    with mk() as s:
        s.iterate(2, stop_rules=False)
        seen[2] = _exports(s)

        def cb(i, crit, its, info):
            if i == 3:                      # the 4th iteration; the 5th is already on the stream
                seen[4] = _exports(s)
        s.iterate(4, stop_rules=False, callback=cb)
        touched = _final(s)
    with mk() as s:
        s.iterate(6, stop_rules=False)
        plain = _final(s)
    assert len(plain["crit"]) == 6 and sorted(seen) == [2, 4]
    _assert_same_tree(touched, plain)
    for n in (2, 4):                        # the data is that of the reported iteration
        with mk() as s:
            s.iterate(n, stop_rules=False)
            _assert_same_tree(seen[n], _exports(s))


_PIPE0_CHILD = r"""
import sys
sys.path[:0] = [{repo!r}, {pkg!r}]
import numpy as np
from foto import FotoError
from foto.bb import BBSolver
from foto.synthetic import textured_pair

Nx, Ny, Nt = 40, 30, 6
f0, f1 = textured_pair(Nx, Ny, seed=0)
res, refused = [], []
for call in (True, False):
    with BBSolver(f0, f1, Nt, Nx, Ny, cg_mode=3) as s:
        def cb(i, crit, its, info):
            if not call or i != 2:
                return
            for fn in (lambda: s.frames(Nt), lambda: s.frames_device([0.5]), s.flow_path, s.flow_path_device):
                try:
                    fn()
                    refused.append(False)
                except FotoError:
                    refused.append(True)
        s.iterate(5, stop_rules=False, callback=cb)
        res.append([np.array(s.crit), np.array(s.cg_its, dtype=np.float64), s.phi(), *s.state(), *s.flow(),
                    *s.flow_path()])
assert refused == [True] * 4, refused
for a, b in zip(*res):
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
print("PIPE0 CHILD OK")
"""


def test_one_in_flight_callback_is_refused():
    """FOTO_PIPE=0: the next solve overwrites phi, so the four calls raise FotoError from the
    callback, and the solve finishes as one that made no call."""
    env = dict(os.environ, FOTO_PIPE="0")
    r = subprocess.run([sys.executable, "-c", _PIPE0_CHILD.format(repo=REPO, pkg=PKG)], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 0 and "PIPE0 CHILD OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------ 5. errors

def test_errors():
    Nx, Ny, Nt = 37, 29, 5
    f0, f1 = pair(Nx, Ny)
    L = _lib.lib()
    P = ctypes.c_void_p
    fill = np.full((2, Ny, Nx), 7.25)

    def frames_dev(s, pos, scale, out, dtype, count=None):
        pos = np.array(pos, dtype=np.float64)
        return L.foto_bb_frames_dev(s._ctx, _lib.dptr(pos), len(pos) if count is None else count, scale, P(out),
                                    dtype, None)

    with BBSolver(f0.ravel(), f1.ravel(), Nt, Nx, Ny, cg_mode=-1) as s:
        rec = DeviceArray((Nt - 1, 3, Ny, Nx), np.float64)
        hu = np.empty((3, Nt - 1, Nx * Ny))
        assert L.foto_bb_flow_path_dev(s._ctx, P(rec.ptr), _lib.FOTO_F64, 0, None) == _lib.FOTO_ERR_STATE
        assert L.foto_bb_flow_path(s._ctx, _lib.dptr(hu[0]), _lib.dptr(hu[1]), _lib.dptr(hu[2])) == _lib.FOTO_ERR_STATE
        with pytest.raises(_lib.FotoError):
            s.flow_path()
        # frames before any iteration succeed: the linear initial path
        init = np.stack([(1 - n / (Nt - 1)) * f0 + (n / (Nt - 1)) * f1 for n in range(Nt)])
        assert same(s.frames_device(Nt, dtype="float64").to_numpy(), init)
        s.iterate(2, stop_rules=False)
        out = DeviceArray.from_numpy(fill)
        host = np.array(fill)
        E = _lib.FOTO_ERR_ARG
        F64 = _lib.FOTO_F64
        assert frames_dev(s, [0.0, -0.1], 1.0, out.ptr, F64) == E
        assert frames_dev(s, [Nt - 1 + 1e-9, 0.0], 1.0, out.ptr, F64) == E
        assert frames_dev(s, [0.0, float("nan")], 1.0, out.ptr, F64) == E
        assert frames_dev(s, [0.0, float("inf")], 1.0, out.ptr, F64) == E
        assert frames_dev(s, [0.0, 1.0], 1.0, out.ptr, F64, count=0) == E
        assert frames_dev(s, [0.0, 1.0], 0.0, out.ptr, F64) == E
        assert frames_dev(s, [0.0, 1.0], -1.0, out.ptr, F64) == E
        assert frames_dev(s, [0.0, 1.0], float("nan"), out.ptr, F64) == E
        assert frames_dev(s, [0.0, 1.0], float("inf"), out.ptr, F64) == E
        assert frames_dev(s, [0.0, 1.0], 1.0, out.ptr, 3) == E
        assert frames_dev(s, [0.0, 1.0], 1.0, out.ptr, -1) == E
        assert frames_dev(s, [0.0, 1.0], 1.0, host.ctypes.data, F64) == E       # a host pointer
        assert frames_dev(s, [0.0, 1.0], 1.0, 0, F64) == E
        three = [0.0, 1.0, 2.0]                                                  # one frame past the allocation
        assert frames_dev(s, three, 1.0, out.ptr, F64) == E
        assert L.foto_bb_frames_dev(s._ctx, None, 2, 1.0, P(out.ptr), F64, None) == E
        pos = np.array([0.0, -0.1])
        assert L.foto_bb_frames(s._ctx, _lib.dptr(pos), 2, 1.0, _lib.dptr(host)) == E
        assert same(out.to_numpy(), fill) and same(host, fill)                  # `out` untouched
        # the flow path: uint8, a bad layout, a host pointer
        assert L.foto_bb_flow_path_dev(s._ctx, P(rec.ptr), _lib.FOTO_U8, 0, None) == E
        assert L.foto_bb_flow_path_dev(s._ctx, P(rec.ptr), F64, 2, None) == E
        assert L.foto_bb_flow_path_dev(s._ctx, P(hu.ctypes.data), F64, 0, None) == E
        small = DeviceArray((Nt - 2, 3, Ny, Nx), np.float64)                    # one record short
        assert L.foto_bb_flow_path_dev(s._ctx, P(small.ptr), F64, 0, None) == E
        # the context is as it was
        want = s.flow_path()
        assert same(s.flow_path_device(out=rec, dtype="float64").to_numpy(),
                    np.stack(want, axis=1).reshape(Nt - 1, 3, Ny, Nx))
        assert same(s.frames_device([0.0, 1.0], out=out, dtype="float64").to_numpy(), s.frames([0, 1]))


def test_frames_more_than_one_launch():
    """More frames than one launch's argument block holds (128): the second launch starts at the
    right frame."""
    Nx, Ny, Nt = 7, 6, 5
    f0, f1 = pair(Nx, Ny)
    with BBSolver(f0.ravel(), f1.ravel(), Nt, Nx, Ny, cg_mode=0) as s:
        s.iterate(1, stop_rules=False)
        got = s.frames_device(131, dtype="float64").to_numpy()
        assert same(got, s.frames(131))
        planes = s.state()[0][:Nt * Nx * Ny].reshape(Nt, Ny, Nx)
    assert same(got[0], planes[0]) and same(got[130], planes[Nt - 1])


# ------------------------------------------------------------------ 6. stream order with torch

_TORCH_CHILD = r"""
import sys
sys.path[:0] = [{repo!r}, {pkg!r}]
import torch                      # first: libfoto then binds to torch's HIP runtime
import numpy as np
from foto import device
from foto.bb import BBSolver
from foto.synthetic import textured_pair

w, h, Nt = 37, 29, 5
f0, f1 = (np.round(f.reshape(h, w) * 255).astype(np.uint8) for f in textured_pair(w, h))
t0, t1 = torch.from_numpy(f0).cuda(), torch.from_numpy(f1).cuda()
side = torch.cuda.Stream()
big = torch.ones(1 << 24, device="cuda")
torch.cuda.synchronize()
with BBSolver.from_device(t0, t1, Nt, cg_mode=-1) as s:
    s.iterate(3, stop_rules=False)
    fr_ref = s.frames(7)
    u, v, m = s.flow_path()
    with torch.cuda.stream(side):
        fr = torch.full((7, h, w), -1.0, dtype=torch.float32, device="cuda")
        rec = torch.full((Nt - 1, 3, h, w), -1.0, dtype=torch.float64, device="cuda")
        for _ in range(4):
            big = big * 1.0000001 + 0.0        # keeps the stream busy ahead of the targets' fills
        fr.fill_(-2.0)
        rec.fill_(-2.0)
        assert s.frames_device(7, out=fr, stream=side) is fr
        assert s.flow_path_device(out=rec, dtype="float64", stream=side) is rec
        fr2 = fr * 2.0                         # consumers on the same stream, no host sync between
        rec2 = rec + 1.0
        got_fr, got_rec = fr2.cpu().numpy(), rec2.cpu().numpy()     # (.cpu() waits on the side stream)
want = np.stack([u, v, m], axis=1).reshape(Nt - 1, 3, h, w)
assert np.array_equal(got_fr.view(np.uint32), (fr_ref.astype(np.float32) * np.float32(2.0)).view(np.uint32))
assert np.array_equal(got_rec.view(np.uint64), (want + 1.0).view(np.uint64))

# the one-shot: bb_flow plus the two exports on the cached context
kw = dict(r=1.0, convergence_tol=0.0, reg_epsilon=1e-3, max_it=4)
flow = torch.as_tensor(device.bb_flow(t0, t1, Nt, dtype="float64", **kw), device="cuda").cpu().numpy()
frames, path = device.bb_path(t0, t1, Nt, frames=5, dtype="float64", normalize=False, **kw)
path = torch.as_tensor(path, device="cuda").cpu().numpy()
assert torch.as_tensor(frames, device="cuda").shape == (5, h, w) and path.shape == (Nt - 1, 3, h, w)
assert np.array_equal(path[-1].view(np.uint64), flow.view(np.uint64))
fr8, _ = device.bb_path(t0, t1, Nt, frames=[0, Nt - 1], frame_dtype="uint8", normalize=True, max_it=1)
fr8 = torch.as_tensor(fr8, device="cuda").cpu().numpy()
assert fr8.dtype == np.uint8 and fr8.shape == (2, h, w)
# (normalize: the planes are about 1 / (w h) and would all export as 0; the frame-0 sum as scale
# brings them back to f0's range)
assert fr8.max() > 0
torch.cuda.synchronize()
print("TORCH CHILD OK")
"""


def test_torch_stream_order():
    if importlib.util.find_spec("torch") is None:
        pytest.skip("torch is not installed")
    code = _TORCH_CHILD.format(repo=REPO, pkg=PKG)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, env=dict(os.environ))
    assert r.returncode == 0 and "TORCH CHILD OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
