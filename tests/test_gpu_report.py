"""The transport report on the GPU (include/foto.h: foto_bb_report / _dev, foto_report_from_state;
BBSolver.report / report_device, ops.report_from_state, foto.device.bb_report).

Bars.  Every per-voxel term of the report is bit-identical to its numpy restatement (the library is
built without FMA contraction; g and c come from ops.grad_st and ops.bb_rhs(mu, 0, ...), which run
the kernel's own device functions), so only the order of a plane's sum differs.  Against the
correctly rounded sum math.fsum(terms) any float64 summation order of n terms errs by at most
(n - 1) u sum|terms| to first order, u = 2^-53; doubled for the higher-order part the bar is
|got - ref| <= 2 Nx Ny 2^-53 sum|terms| per plane and column.  It is derived, not measured.  The
criterion: a quotient of two such sums of non-negative terms on each side and a square root,
relative bar 4 N 2^-53 with N = Nt Nx Ny.  Everything else compares entries of this build with
each other and is bit for bit (integer views).
"""
import ctypes
import importlib.util
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import PKG, REPO  # noqa: E402  (puts the package on sys.path)

from foto import _lib, bb, device, ops  # noqa: E402
from foto import report as R  # noqa: E402
from foto.bb import BBSolver  # noqa: E402
from foto.device import DeviceArray  # noqa: E402
from foto.synthetic import textured_pair  # noqa: E402

ITS = 3
U = 2.0 ** -53
COLS = ["MASS", "KINETIC", "VACUUM", "CONT", "HJ_NUM", "HJ_DEN", "DUAL", "DIST_T"]

# (Nx, Ny, Nt, options): the smallest grids at which each path can go wrong
CONFIGS = {
    "stencil-37x29x5": (37, 29, 5, dict(cg_mode=-1)),
    "pipelined-40x30x6": (40, 30, 6, dict(cg_mode=3)),
    "sharded-40x30x6": (40, 30, 6, dict(cg_mode=3, virtual_ranks=2)),
    "uneven-7x6x5": (7, 6, 5, dict(cg_mode=0, virtual_ranks=2)),           # slabs of 3 and 2 planes
    "narrow-33x5x4": (33, 5, 4, dict(cg_mode=-1)),
    "tiny-2x2x2": (2, 2, 2, dict(cg_mode=-1)),       # every voxel on every boundary, both DUAL planes
    "pieces-130x67x3": (130, 67, 3, dict(cg_mode=-1)),   # 8710 voxels per plane: 5 pieces, the last ragged
}


def ibits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(ibits(a), ibits(b))


def terms(mu, phi, rho0, rhoT, Nt, Nx, Ny):
    """The eight per-voxel terms of include/foto.h in numpy, [8][Nt][Nx*Ny], in the header's
    operation order; g and c from the library's own per-voxel entries."""
    nxy, N = Nx * Ny, Nt * Nx * Ny
    rho, m1, m2 = (mu[k * N:(k + 1) * N].reshape(Nt, nxy) for k in range(3))
    gt, gx, gy = ops.grad_st(phi, Nt, Nx, Ny).reshape(3, Nt, nxy)
    c = ops.bb_rhs(mu, np.zeros(3 * N), rho0, rhoT, 1.0, Nt, Nx, Ny).reshape(Nt, nxy)
    ph = phi.reshape(Nt, nxy)
    mm, gg, pos = m1 * m1 + m2 * m2, gx * gx + gy * gy, rho > 0
    T = np.zeros((8, Nt, nxy))
    T[R.MASS] = rho
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        T[R.KINETIC] = np.where(pos, mm / (rho + rho), 0.0)
    T[R.VACUUM] = np.where(pos, 0.0, mm)
    T[R.CONT] = c * c
    T[R.HJ_NUM] = rho * np.abs(gt + 0.5 * gg)
    T[R.HJ_DEN] = rho * gg
    T[R.DUAL][0] = -(ph[0] * rho0)
    T[R.DUAL][Nt - 1] = ph[Nt - 1] * rhoT
    T[R.DIST_T] = (rho - rhoT) * (rho - rhoT)
    return T


def assert_within_bar(table, T, Nx, Ny, label, cols=range(8)):
    """|got - fsum(terms)| <= 2 Nx Ny 2^-53 sum|terms| for every plane and column of `cols`; prints
    the largest error / bar ratio per column before asserting."""
    Nt = table.shape[0]
    worst, bad = {}, []
    for k in cols:
        worst[k] = 0.0
        for n in range(Nt):
            ref = math.fsum(T[k, n])
            bar = 2.0 * Nx * Ny * U * math.fsum(np.abs(T[k, n]))
            err = abs(table[n, k] - ref)
            if bar > 0:
                worst[k] = max(worst[k], err / bar)
            if not err <= bar:
                bad.append((COLS[k], n, table[n, k], ref, err, bar))
    print(f"{label}: max error / bar " + ", ".join(f"{COLS[k]} {worst[k]:.2e}" for k in cols))
    assert not bad, bad


_solved = {}


def solved(name):
    """One solve per configuration (3 iterations, no stop rules) and everything the tests compare,
    computed once and left unchanged."""
    if name in _solved:
        return _solved[name]
    Nx, Ny, Nt, opts = CONFIGS[name]
    f0, f1 = textured_pair(Nx, Ny, seed=0)
    r = dict(Nx=Nx, Ny=Ny, Nt=Nt, f0=f0, f1=f1, cb=[])
    with BBSolver(f0, f1, Nt, Nx, Ny, **opts) as s:
        s.iterate(ITS, stop_rules=False, callback=lambda i, crit, its, info: r["cb"].append(crit))
        r["mu"], r["phi"] = s.state()[0], s.phi()
        r["rep"] = s.report()
        r["rep2"] = s.report()
        r["dev"] = s.report_device().to_numpy()
        mine = DeviceArray((Nt, 8), np.float64)           # a caller-owned target
        assert s.report_device(out=mine) is mine
        r["mine"] = mine.to_numpy()
        r["mu_after"], r["phi_after"] = s.state()[0], s.phi()
    r["from_state"] = ops.report_from_state(r["mu"], r["phi"], f0, f1, Nt, Nx, Ny)
    _solved[name] = r
    return r


# ------------------------------------------------------------------ 1. against numpy, term by term

@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_against_numpy(name):
    r = solved(name)
    Nx, Ny, Nt = r["Nx"], r["Ny"], r["Nt"]
    rep = r["rep"]
    assert rep.table.shape == (Nt, 8) and (rep.Nt, rep.Nx, rep.Ny) == (Nt, Nx, Ny)
    assert np.isfinite(rep.table).all()
    T = terms(r["mu"], r["phi"], r["f0"], r["f1"], Nt, Nx, Ny)
    assert_within_bar(rep.table, T, Nx, Ny, name)
    # interior planes carry no DUAL term, exactly
    assert not rep.dual[1:Nt - 1].any()
    assert rep.dual[0] != 0 and rep.dual[Nt - 1] != 0


# ------------------------------------------------------------------ 2. the criterion

def crit_bar(Nt, Nx, Ny):
    return 4.0 * Nt * Nx * Ny * U


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_crit_matches_callback(name):
    """The fused k_prox_rhs path (the default)."""
    r = solved(name)
    crit, got = r["cb"][-1], r["rep"].crit
    print(f"{name}: crit {crit!r}, report {got!r}, rel diff {abs(got - crit) / crit:.2e}, bar "
          f"{crit_bar(r['Nt'], r['Nx'], r['Ny']):.2e}")
    assert len(r["cb"]) == ITS and crit > 0
    assert abs(got - crit) <= crit_bar(r["Nt"], r["Nx"], r["Ny"]) * crit


@pytest.mark.parametrize("name", ["stencil-37x29x5", "pipelined-40x30x6", "sharded-40x30x6"])
def test_crit_matches_callback_separate_prox(name, monkeypatch):
    """FOTO_FUSE_PR=0: k_prox and k_rhs as separate launches."""
    monkeypatch.setenv("FOTO_FUSE_PR", "0")
    Nx, Ny, Nt, opts = CONFIGS[name]
    f0, f1 = textured_pair(Nx, Ny, seed=0)
    with BBSolver(f0, f1, Nt, Nx, Ny, **opts) as s:
        s.iterate(ITS, stop_rules=False)
        rep, crit = s.report(), s.crit[-1]
        assert same(rep.table, ops.report_from_state(s.state()[0], s.phi(), f0, f1, Nt, Nx, Ny))
    print(f"{name}: crit {crit!r}, report {rep.crit!r}, rel diff {abs(rep.crit - crit) / crit:.2e}")
    assert abs(rep.crit - crit) <= crit_bar(Nt, Nx, Ny) * crit


def test_report_from_pipelined_callback(monkeypatch):
    """From the callback of the pipelined loop the report is that of the iteration the callback
    reports, not of the one in flight."""
    monkeypatch.delenv("FOTO_PIPE", raising=False)
    Nx, Ny, Nt, opts = CONFIGS["pipelined-40x30x6"]
    f0, f1 = textured_pair(Nx, Ny, seed=0)
    seen = {}
    with BBSolver(f0, f1, Nt, Nx, Ny, **opts) as s:
        def cb(i, crit, its, info):
            if i in (1, 2):                 # iteration i + 1 is already on the stream
                seen[i] = (crit, s.report())
        s.iterate(5, stop_rules=False, callback=cb)
        crits = list(s.crit)
    assert sorted(seen) == [1, 2] and len(crits) == 5
    for i, (crit, rep) in seen.items():
        print(f"callback {i}: crit {crit!r}, report {rep.crit!r}; next iteration's {crits[i + 1]!r}")
        assert abs(rep.crit - crit) <= crit_bar(Nt, Nx, Ny) * crit
        assert abs(rep.crit - crits[i + 1]) > 100 * crit_bar(Nt, Nx, Ny) * crit   # (the test can tell them apart)
    # ... and is the table a stopped solve gives
    with BBSolver(f0, f1, Nt, Nx, Ny, **opts) as s:
        s.iterate(2, stop_rules=False)
        assert same(s.report().table, seen[1][1].table)


# ------------------------------------------------------------------ 3. bit for bit

@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_entries_agree_bitwise(name):
    """Host entry, device entry, caller's target, the context-free entry on the gathered state
    (for the two virtual_ranks = 2 configurations: sharded equals unsharded on the same data), and
    a second call."""
    r = solved(name)
    t = r["rep"].table
    assert t.dtype == np.float64 and r["dev"].shape == (r["Nt"], 8)
    assert same(t, r["dev"])
    assert same(t, r["mine"])
    assert same(t, r["from_state"])
    assert same(t, r["rep2"].table)
    # the calls left the state alone
    assert same(r["mu"], r["mu_after"]) and same(r["phi"], r["phi_after"])


# ------------------------------------------------------------------ 4. no perturbation

@pytest.mark.parametrize("name", ["pipelined-40x30x6", "sharded-40x30x6", "stencil-37x29x5"])
def test_report_does_not_perturb_the_solve(name):
    Nx, Ny, Nt, opts = CONFIGS[name]
    f0, f1 = textured_pair(Nx, Ny, seed=0)
    res = []
    for with_report in (True, False):
        with BBSolver(f0, f1, Nt, Nx, Ny, **opts) as s:
            for _ in range(3):
                s.iterate(1, stop_rules=False)
                if with_report:
                    s.report()
                    s.report_device()
            s.iterate(1, stop_rules=False)
            st0 = s.stats()
            res.append([s.phi(), *s.state(), *s.flow(), np.array(s.crit)])
            assert st0["outer_iters"] == 4
    for a, b in zip(*res):
        assert same(a, b)


# ------------------------------------------------------------------ 5. empty density

def blob(Nx, Ny, cx, cy, sigma=2.0, mass=100.0):
    x = np.arange(Nx, dtype=np.float64)[None, :]
    y = np.arange(Ny, dtype=np.float64)[:, None]
    g = np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * sigma * sigma))
    return (mass * g / g.sum()).ravel()


def test_empty_density_after_many_iterations():
    Nx, Ny, Nt = 20, 16, 6
    f0, f1 = blob(Nx, Ny, 7, 8), blob(Nx, Ny, 11, 8)
    with BBSolver(f0, f1, Nt, Nx, Ny, cg_mode=-1) as s:
        s.iterate(100, stop_rules=False)
        mu, phi, rep = s.state()[0], s.phi(), s.report()
    rho = mu[:Nt * Nx * Ny]
    share = np.count_nonzero(rho == 0) / rho.size
    print(f"voxels with rho = 0 after 100 iterations: {100 * share:.1f} %; {rep!r}")
    assert share >= 0.05
    T = terms(mu, phi, f0, f1, Nt, Nx, Ny)
    assert T[R.VACUUM].any()                       # the select has both outcomes to take
    assert_within_bar(rep.table, T, Nx, Ny, "blobs-20x16x6")


def test_vacuum_split_on_a_hand_made_state():
    """rho = +0.0, -0.0 and 1e-300 next to non-zero momentum: the first two are VACUUM, the third
    is KINETIC."""
    Nx, Ny, Nt = 9, 8, 4
    nxy, N = Nx * Ny, Nt * Nx * Ny
    rng = np.random.default_rng(5)
    mu = rng.standard_normal(3 * N)
    mu[:N] = np.abs(mu[:N]) + 0.1
    phi, rho0, rhoT = rng.standard_normal(N), rng.random(nxy), rng.random(nxy)
    rho, m1, m2 = (mu[k * N:(k + 1) * N].reshape(Nt, nxy) for k in range(3))
    # plane 0: the three special densities among ordinary voxels
    rho[0, 10], rho[0, 11], rho[0, 12] = 0.0, -0.0, 1e-300
    m1[0, 10:13] = 1.0, -2.0, 0.5
    # planes 1-3: one special voxel each, the only one of its plane that carries momentum
    m1[1:], m2[1:] = 0.0, 0.0
    v = 3 * Nx + 4
    for n, d in ((1, 0.0), (2, -0.0), (3, 1e-300)):
        rho[n, v], m1[n, v], m2[n, v] = d, 0.75, -1.5
    mm = 0.75 * 0.75 + 1.5 * 1.5
    got = ops.report_from_state(mu, phi, rho0, rhoT, Nt, Nx, Ny)
    assert got[1, R.VACUUM] == mm and got[1, R.KINETIC] == 0.0
    assert got[2, R.VACUUM] == mm and got[2, R.KINETIC] == 0.0
    assert got[3, R.VACUUM] == 0.0 and got[3, R.KINETIC] == mm / (1e-300 + 1e-300)
    T = terms(mu, phi, rho0, rhoT, Nt, Nx, Ny)
    assert T[R.VACUUM][0, 10] > 0 and T[R.VACUUM][0, 11] > 0 and T[R.VACUUM][0, 12] == 0
    assert T[R.KINETIC][0, 10] == 0 and T[R.KINETIC][0, 11] == 0 and T[R.KINETIC][0, 12] > 1e298
    assert_within_bar(got, T, Nx, Ny, "hand-made 9x8x4", cols=(R.KINETIC, R.VACUUM))


# ------------------------------------------------------------------ 6. plane independence

def test_plane_independence():
    """A plane's sums are a function of that plane's data and its t-neighbours alone: a NaN in one
    voxel reaches exactly the entries whose terms read it, every other entry keeps its bits."""
    Nx, Ny, Nt = 9, 8, 4
    nxy, N = Nx * Ny, Nt * Nx * Ny
    rng = np.random.default_rng(7)
    mu = rng.standard_normal(3 * N)
    mu[:N] = np.abs(mu[:N]) + 0.1
    v, w = 2 * nxy + 3 * Nx + 4, 2 * nxy + 5 * Nx + 2      # two voxels of plane 2
    mu[w] = 0.0                                           # (w: an emptied voxel)
    phi, rho0, rhoT = rng.standard_normal(N), rng.random(nxy), rng.random(nxy)
    base = ops.report_from_state(mu, phi, rho0, rhoT, Nt, Nx, Ny)
    assert np.isfinite(base).all()

    def run(index, value=float("nan")):
        m = mu.copy()
        m[index] = value
        got = ops.report_from_state(m, phi, rho0, rhoT, Nt, Nx, Ny)
        changed = {(int(n), COLS[k]) for n, k in zip(*np.nonzero(ibits(got) != ibits(base)))}
        nonfinite = {(int(n), COLS[k]) for n, k in zip(*np.nonzero(~np.isfinite(got)))}
        return changed, nonfinite

    # m1 (the x-stencil does not cross planes): where rho > 0 the term is KINETIC's, else VACUUM's
    changed, nonfinite = run(N + v)
    assert changed == nonfinite == {(2, "KINETIC"), (2, "CONT")}
    changed, nonfinite = run(N + w)
    assert changed == nonfinite == {(2, "VACUUM"), (2, "CONT")}
    # m2 likewise (the y-stencil)
    changed, nonfinite = run(2 * N + v)
    assert changed == nonfinite == {(2, "KINETIC"), (2, "CONT")}
    # rho: the t-stencil of planes 1 and 3 reads plane 2.  Plane 2 is interior, where the central
    # difference 0.5 (rho[3] - rho[1]) of div_st's row does not read the plane's own density, so
    # within planes 1-3 it is CONT of 1 and 3 that the NaN reaches
    changed, nonfinite = run(v)
    assert nonfinite == {(1, "CONT"), (3, "CONT"), (2, "MASS"), (2, "HJ_NUM"), (2, "HJ_DEN"), (2, "DIST_T")}
    # (the NaN density counts as emptied: its KINETIC term goes, its momentum lands in VACUUM)
    assert changed == nonfinite | {(2, "KINETIC"), (2, "VACUUM")}
    # rho of plane 3, the last one: its own row (rho[3] - rho[2], and the rhoT term) and plane 2's
    changed, nonfinite = run(v + nxy)
    assert nonfinite == {(2, "CONT"), (3, "CONT"), (3, "MASS"), (3, "HJ_NUM"), (3, "HJ_DEN"), (3, "DIST_T")}
    assert changed == nonfinite | {(3, "KINETIC"), (3, "VACUUM")}
    # phi of plane 2: g_t of planes 1 and 3, g_x / g_y of plane 2; DUAL's planes are 0 and 3
    p = phi.copy()
    p[v] = float("nan")
    got = ops.report_from_state(mu, p, rho0, rhoT, Nt, Nx, Ny)
    changed = {(int(n), COLS[k]) for n, k in zip(*np.nonzero(ibits(got) != ibits(base)))}
    assert changed == {(1, "HJ_NUM"), (2, "HJ_NUM"), (2, "HJ_DEN"), (3, "HJ_NUM")}


# ------------------------------------------------------------------ 7. state and argument rules

def test_state_and_argument_rules():
    Nx, Ny, Nt = 37, 29, 5
    f0, f1 = textured_pair(Nx, Ny, seed=0)
    L = _lib.lib()
    P = ctypes.c_void_p
    fill = np.full((Nt, 8), 7.25)
    with BBSolver(f0, f1, Nt, Nx, Ny, cg_mode=-1) as s:
        out = DeviceArray.from_numpy(fill)
        host = np.array(fill)
        # before any outer iteration
        assert L.foto_bb_report(s._ctx, _lib.dptr(host)) == _lib.FOTO_ERR_STATE
        assert L.foto_bb_report_dev(s._ctx, P(out.ptr), None) == _lib.FOTO_ERR_STATE
        with pytest.raises(_lib.FotoError):
            s.report()
        with pytest.raises(_lib.FotoError):
            s.report_device()
        s.iterate(2, stop_rules=False)
        E = _lib.FOTO_ERR_ARG
        assert L.foto_bb_report(s._ctx, None) == E
        assert L.foto_bb_report_dev(s._ctx, None, None) == E
        assert L.foto_bb_report_dev(s._ctx, P(host.ctypes.data), None) == E          # a host pointer
        assert L.foto_bb_report_dev(s._ctx, P(out.ptr + 4), None) == E               # misaligned
        short = DeviceArray.from_numpy(fill[:Nt - 1])                                # one plane short
        assert L.foto_bb_report_dev(s._ctx, P(short.ptr), None) == E
        assert L.foto_bb_report_dev(s._ctx, P(out.ptr + 64), None) == E              # runs past its allocation
        assert same(out.to_numpy(), fill) and same(short.to_numpy(), fill[:Nt - 1]) and same(host, fill)
        for bad in (DeviceArray((Nt, 8), np.float32), DeviceArray((Nt + 1, 8), np.float64),
                    DeviceArray((8, Nt), np.float64).T, DeviceArray((Nt, 10), np.float64)[:, :8]):
            with pytest.raises(ValueError):
                s.report_device(out=bad)
        # the context is as it was
        want = s.report().table
        assert s.report_device(out=out) is out and same(out.to_numpy(), want)
        assert same(want, ops.report_from_state(s.state()[0], s.phi(), f0, f1, Nt, Nx, Ny))


def test_one_in_flight_callback_is_refused():
    """virtual_ranks = 2 runs the one-in-flight loop, whose next solve overwrites phi: both entries
    return FOTO_ERR_STATE from its callback, and the solve finishes as one that made no call."""
    Nx, Ny, Nt, opts = CONFIGS["sharded-40x30x6"]
    f0, f1 = textured_pair(Nx, Ny, seed=0)
    L = _lib.lib()
    rcs, res = [], []
    for call in (True, False):
        with BBSolver(f0, f1, Nt, Nx, Ny, **opts) as s:
            host = np.full((Nt, 8), 7.25)
            out = DeviceArray.from_numpy(host)

            def cb(i, crit, its, info):
                if call and i == 1:
                    rcs.append(L.foto_bb_report(s._ctx, _lib.dptr(host)))
                    rcs.append(L.foto_bb_report_dev(s._ctx, ctypes.c_void_p(out.ptr), None))
            s.iterate(3, stop_rules=False, callback=cb)
            assert (host == 7.25).all() and (out.to_numpy() == 7.25).all()
            res.append([s.phi(), *s.state(), s.report().table])
    assert rcs == [_lib.FOTO_ERR_STATE] * 2
    for a, b in zip(*res):
        assert same(a, b)


_TORCH_CHILD = r"""
import sys
sys.path[:0] = [{repo!r}, {pkg!r}]
import torch                      # first: libfoto then binds to torch's HIP runtime
import numpy as np
from foto.bb import BBSolver
from foto.synthetic import textured_pair

w, h, Nt = 37, 29, 5
f0, f1 = textured_pair(w, h)
side = torch.cuda.Stream()
big = torch.ones(1 << 24, device="cuda")
torch.cuda.synchronize()
with BBSolver(f0, f1, Nt, w, h, cg_mode=-1) as s:
    s.iterate(3, stop_rules=False)
    want = s.report().table
    with torch.cuda.stream(side):
        out = torch.full((Nt, 8), -1.0, dtype=torch.float64, device="cuda")
        for _ in range(4):
            big = big * 1.0000001 + 0.0        # keeps the stream busy ahead of the target's fill
        out.fill_(-2.0)
        assert s.report_device(out=out, stream=side) is out
        copy = out.clone()                     # the consumer: a copy on the same stream, no host sync between
        got = copy.cpu().numpy()               # (.cpu() waits on the side stream)
assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
torch.cuda.synchronize()
print("TORCH CHILD OK")
"""


def test_report_device_on_a_callers_stream():
    if importlib.util.find_spec("torch") is None:
        pytest.skip("torch is not installed")
    code = _TORCH_CHILD.format(repo=REPO, pkg=PKG)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, env=dict(os.environ))
    assert r.returncode == 0 and "TORCH CHILD OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------ 8. the one-shot

def test_one_shot_on_device_frames():
    w, h, Nt = 37, 29, 5
    f0, f1 = (np.round(f.reshape(h, w) * 255).astype(np.uint8) for f in textured_pair(w, h))
    d0, d1 = DeviceArray.from_numpy(f0), DeviceArray.from_numpy(f1)
    kw = dict(r=1.0, convergence_tol=0.0, reg_epsilon=1e-3, max_it=3)
    try:
        got = device.bb_report(d0, d1, Nt, cg_mode=-1, **kw)
        again = device.bb_report(d0, d1, Nt, cg_mode=-1, **kw)      # the cached context, reset
    finally:
        bb.clear_context_cache()
    with BBSolver.from_device(d0, d1, Nt, r=1.0, reg_epsilon=1e-3, cg_mode=-1) as s:
        s.iterate(3, convergence_tol=0.0, stop_rules=True)
        want = s.report()
    assert isinstance(got, R.TransportReport) and (got.Nt, got.Nx, got.Ny) == (Nt, w, h)
    assert same(got.table, want.table) and same(again.table, want.table)
    assert np.isfinite(got.table).all() and got.mass[0] > 0
