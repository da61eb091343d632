"""TV-L1 flow with an illumination channel on the device (csrc/foto_tvl1.hip) against the numpy
restatement of the scheme (tests/tvl1_ref.py): the coefficient kernel and the inner iteration one by
one, the whole solve through the host and the device entries, its quality on the three pairs the
method is there for, and the CLI.

Sizes.  The iteration kernel works on TW x TH = foto.tvl1.TILE_W x TILE_H tiles (64 x 4), one thread
per pixel.  Beside the project's (2, 2), (3, 5), (33, 17), (71, 77): one pixel more than a tile in
each direction, and two tiles plus one."""
import contextlib
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import PKG  # noqa: E402,F401  (puts the package on sys.path)

import gn_pyr_ref as G  # noqa: E402
import tvl1_ref as T  # noqa: E402
from foto import tvl1  # noqa: E402
from foto import device as D  # noqa: E402
from foto.device import DeviceArray  # noqa: E402

TW, TH = tvl1.TILE_W, tvl1.TILE_H
SIZES = [(2, 2), (3, 5), (33, 17), (71, 77), (TW + 1, TH + 1), (2 * TW + 1, 2 * TH + 1)]
OP_TOL = 1e-13   # the project's operator tolerance, times max(1, max|ref|)
LAM, THETA, TAU = 38.0, 0.3, 0.25


def close(got, ref, tol, what):
    got, ref = np.asarray(got), np.asarray(ref)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what
    bound = tol * max(1.0, np.abs(ref[~nan]).max())
    err = np.abs(got[~nan] - ref[~nan]).max()
    print(f"{what}: max abs diff {err:.3e} (bound {bound:.3e})")
    assert err <= bound, what


# ------------------------------------------------------------------ the kernels

@pytest.mark.parametrize("w,h", SIZES)
def test_coeffs(w, h):
    """Sub-pixel displacements everywhere, then exact integers, far out of frame on all four sides
    and one NaN at chosen pixels (2 x 2 has four pixels: the NaN, two far ones that cover the four
    sides between them, and one with an integer x and a sub-pixel y).  The NaN displacement gives
    NaN in all five fields there and nowhere else."""
    n = w * h
    rng = np.random.default_rng(w * 100 + h)
    f1, f2 = rng.random(n), rng.random(n)
    u, v = rng.uniform(-3, 3, n), rng.uniform(-3, 3, n)
    special = [(np.nan, 0.25), (-1e6, 1e6), (1e6, -1e6), (-1.0, -0.5)]
    if n > 4:
        special += [(1.0, 1.0), (-2.0, 0.0), (0.0, 3.0), (-1e6, 0.3), (1e6, 0.3), (0.3, -1e6), (0.3, 1e6),
                    (float(w), float(h)), (0.5, 0.5)]
    for k, (du, dv) in enumerate(special):
        i = (k * n) // len(special)
        u[i], v[i] = du, dv
    for gamma in (0.1, 0.0):
        ref = T.coeffs(f1, f2, u, v, w, h, gamma)
        got = tvl1.coeffs(f1, f2, u, v, w, h, gamma)
        for g, r, name in zip(got, ref, ("a1", "a2", "a3", "n2", "rc")):
            assert np.isnan(r).sum() == 1 and np.isnan(r[0])
            close(g, r, OP_TOL, f"coeffs {name} {w}x{h} gamma {gamma}")


def iterate_inputs(w, h):
    """Random U, random dual vectors of norm <= 1 and random coefficients with |a_d| in [0.1, 1]
    (so that the -rho / n2 branch amplifies a rounding error by 1 / |a| <= 10 at the most), rc
    spread over all three branches; then pixels with n2 = 0 and pixels placed exactly on both
    thresholds (U = 0 there, so rho is rc exactly and rc = +-lambda theta n2 as the kernel forms it)."""
    n = w * h
    rng = np.random.default_rng(w * 1000 + h)
    a = [rng.choice([-1.0, 1.0], n) * rng.uniform(0.1, 1.0, n) for _ in range(3)]
    rc = rng.uniform(-25.0, 25.0, n)
    U = [rng.uniform(-2, 2, n) for _ in range(3)]
    P = [rng.uniform(-0.7, 0.7, n) for _ in range(6)]
    lt = LAM * THETA
    kinds = ["zero-", "upper", "lower"] + (["zero0", "zero+", "upper", "lower"] if n > 4 else [])
    for k, kind in enumerate(kinds):
        i = (k * n) // len(kinds)
        if kind.startswith("zero"):
            for d in range(3):
                a[d][i] = 0.0
            rc[i] = {"-": -1.0, "0": 0.0, "+": 1.0}[kind[-1]]
        else:
            for d in range(3):
                U[d][i] = 0.0
            n2 = (a[0][i] * a[0][i] + a[1][i] * a[1][i]) + a[2][i] * a[2][i]
            rc[i] = lt * n2 if kind == "upper" else -lt * n2
    n2 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    return (a[0], a[1], a[2], n2, rc), U, P


@pytest.mark.parametrize("n_it", [1, 2, 7])
@pytest.mark.parametrize("w,h", SIZES)
def test_iterate(w, h, n_it):
    co, U, P = iterate_inputs(w, h)
    rU, rP = T.iterate(co, U, P, w, h, LAM, THETA, TAU, n_it)
    gU, gP = tvl1.iterate(co, U, P, w, h, LAM, THETA, TAU, n_it)
    for d in range(3):
        close(gU[d], rU[d], OP_TOL, f"iterate x{n_it} U[{d}] {w}x{h}")
    for d in range(6):
        close(gP[d], rP[d], OP_TOL, f"iterate x{n_it} P[{d}] {w}x{h}")
        assert np.abs(gP[d]).max() <= 1.0


def tile(k):
    """The tile a block stores with k iterations per launch."""
    return tvl1.REGION_W - 2 * k, tvl1.REGION_H - 2 * k


# for 7, 4 and 3 iterations in a launch: one pixel more than a tile each way, and two tiles plus one
TILED_SIZES = SIZES + [s for k in (7, 4, 3) for s in ((tile(k)[0] + 1, tile(k)[1] + 1),
                                                      (2 * tile(k)[0] + 1, 2 * tile(k)[1] + 1))]


@pytest.mark.parametrize("w,h", TILED_SIZES)
def test_iterate_does_not_depend_on_the_launch_structure(w, h):
    """7 iterations, one per launch, in one call: 6 launches that run the dual and the primal step
    together between a primal-only and a dual-only one.  7 calls of 1, and 4 + 3, cut that chain at
    other places; with several iterations per launch the same 7 run as one launch of 7 on LDS tiles,
    as 4 + 3 and as 3 + 3 + 1 (per_launch = 3).  Every value is computed by one expression wherever
    it is computed: equal bits."""
    co, U, P = iterate_inputs(w, h)
    whole = tvl1.iterate(co, U, P, w, h, LAM, THETA, TAU, 7)
    want = list(whole[0]) + list(whole[1])
    for split, per in (([1] * 7, 1), ([4, 3], 1), ([7], 7), ([4, 3], 4), ([7], 4), ([7], 3), ([2, 5], 8)):
        u, p = U, P
        for k in split:
            u, p = tvl1.iterate(co, u, p, w, h, LAM, THETA, TAU, k, per_launch=per)
        for a, b in zip(list(u) + list(p), want):
            assert np.array_equal(a, b), (split, per)


# ------------------------------------------------------------------ the whole solve

CASES = ["96x80", "71x77", "45x37"]
_gpu = {}


def gpu_flow(case, gamma):
    """The device solver's (u, v, m) of a case through the host entry, once per process (read-only)."""
    key = (case, gamma)
    if key not in _gpu:
        w, h = G.CASES[case][:2]
        with tvl1.TVL1(w, h, gamma=gamma) as p:
            assert p.sizes == G.sizes(w, h, 4)
            u, v, m, st = p.solve(*G.frames(case))
        L = len(p.sizes)
        assert st["levels"] == L and st["sizes"] == p.sizes
        per_warp = 1 + -(-30 // p.opts["per_launch"])   # the coefficients, then ceil(iters / per_launch) launches
        assert st["launches"] == [5 * per_warp + (l < L - 1) for l in range(L)]
        assert st["launches_total"] == sum(st["launches"])
        print(f"{case} gamma {gamma}: launches {st['launches']}, ms per level {['%.2f' % t for t in st['ms_level']]}, "
              f"total {st['ms_total']:.2f} ms")
        for a in (u, v, m):
            a.setflags(write=False)
        _gpu[key] = (u, v, m)
    return _gpu[key]


@pytest.mark.parametrize("gamma", T.GAMMAS)
@pytest.mark.parametrize("case", CASES)
def test_solve_matches_restatement(case, gamma):
    """atol = 1e-6 max(1, max|ref|), the pyramid test's bound, justified the same way: perturbing
    every inner iteration of the restatement by +-1e-13 (the operator tolerance; the kernels run the
    restatement's operations in its order) moved its final flow by at most 8.7e-8 on these cases
    (71x77 at gamma 0, where the -rho / n2 branch amplifies in flat regions;
    tests/test_tvl1_host.py measures and prints it), so the scheme does not carry a per-iteration
    error beyond the bound.  The test prints what it sees."""
    ref = T.reference(case, gamma)
    got = gpu_flow(case, gamma)
    for a, b, name in zip(got, ref, "uvm"):
        print(f"{case} gamma {gamma} {name}: max abs diff {np.abs(a - b).max():.3e} (max|ref| {np.abs(b).max():.3f})")
    for a, b in zip(got, ref):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-6 * max(1.0, np.abs(b).max()))
    if gamma == 0.0:
        assert not got[2].any()


@pytest.mark.parametrize("per_launch", [1, 4, 5, 8])
@pytest.mark.parametrize("case", CASES)
def test_solve_does_not_depend_on_the_launch_structure(case, per_launch):
    """The whole solve with 1, 4, 5 and 8 inner iterations per launch (30 per warp: 30 launches, 7 of
    4 and one of 2, 6 of 5, 3 of 8 and one of 6): equal bits, and the launches the report counts."""
    w, h = G.CASES[case][:2]
    with tvl1.TVL1(w, h, per_launch=per_launch) as p:
        u, v, m, st = p.solve(*G.frames(case))
    L = len(p.sizes)
    assert st["launches"] == [5 * (1 + -(-30 // per_launch)) + (l < L - 1) for l in range(L)]
    for a, b in zip((u, v, m), gpu_flow(case, 0.1)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("gamma", T.GAMMAS)
@pytest.mark.parametrize("case", CASES)
def test_solve_device(case, gamma):
    """The device entry on device frames: float64 planar is the host entry's flow bit for bit,
    float32 its rounding, interleaved its (u, v); into a new array and into the caller's."""
    w, h = G.CASES[case][:2]
    f1, f2 = G.frames(case)
    d1, d2 = DeviceArray.from_numpy(f1.reshape(h, w)), DeviceArray.from_numpy(f2.reshape(h, w))
    want = np.stack(gpu_flow(case, gamma)).reshape(3, h, w)
    with tvl1.TVL1(w, h, gamma=gamma) as p:
        out, st = p.solve_device(d1, d2, dtype="float64", layout="planar", stats=True)
        assert st["levels"] == len(p.sizes) and out.shape == (3, h, w)
        assert np.array_equal(out.to_numpy(), want)
        out, st = p.solve_device(d1, d2, dtype="float32", layout="planar")
        assert st is None and np.array_equal(out.to_numpy(), np.float32(want))
        mine = DeviceArray((h, w, 2), np.float64)
        got, _ = p.solve_device(d1, d2, out=mine, dtype="float64", layout="interleaved")
        assert got is mine and np.array_equal(mine.to_numpy(), np.moveaxis(want[:2], 0, 2))
        out, _ = p.solve_device(d1, d2, dtype="float32", layout="interleaved")
        assert np.array_equal(out.to_numpy(), np.float32(np.moveaxis(want[:2], 0, 2)))
    # the cached solver behind foto.device.tvl1_flow; its buffer is what the flow tools take
    flow = D.tvl1_flow(d1, d2, gamma=gamma)
    assert np.array_equal(flow.to_numpy(), np.float32(want))
    if case == "45x37":
        from foto import chain, evaluate, render
        assert render.reconstruct(d1, flow).shape == (h, w)
        assert chain.invert(flow).shape == (3, h, w)
        gt = DeviceArray.from_numpy(np.ascontiguousarray(np.broadcast_to(np.float32(G.CASES[case][2]), (h, w, 2))))
        ee = float(evaluate.score_flow(flow, gt).ee_R[0])   # (the share of pixels more than 0.5 px off)
        print(f"{case} gamma {gamma}: EE-R0.5 {ee:.4f}")
        assert 0.0 <= ee <= 1.0
    tvl1.clear_cache()


def test_reused_solver_equals_fresh():
    """A second pair on the same solver (its buffers hold the first pair's fields) equals a fresh
    solver's result bit for bit, and identical frames give exactly zero."""
    w, h = 71, 77
    from foto.synthetic import textured_pair
    a = textured_pair(w, h, seed=1, dx=3.0, dy=1.0, smooth=5)
    b = G.frames("71x77")
    with tvl1.TVL1(w, h) as p:
        p.solve(*a)
        second = p.solve(*b)
        zero = p.solve(b[0], b[0])
    for x, y in zip(second[:3], gpu_flow("71x77", 0.1)):
        assert np.array_equal(x, y)
    for x in zero[:3]:
        assert not x.any()


# ------------------------------------------------------------------ quality, as a condition

def device_epe(f1, f2, tu, tv, **opts):
    w, h = 96, 80
    with tvl1.TVL1(w, h, **opts) as p:
        u, v, m, _ = p.solve(f1, f2)
    return T.interior_epe(u, v, w, h, tu, tv)


def test_quality_layered():
    """Two layers moving (2, 0) and (-2, 1): interior EPE <= 0.25 x the GN pyramid restatement's
    (levels 3, warps 3).  The restatement of TV-L1 gives 0.147 px against 0.888 px, ratio 0.165."""
    w, h = 96, 80
    f1, f2, tu, tv = T.layered_pair()
    e = device_epe(f1, f2, tu, tv)
    gu, gv, _ = G.pyramid(f1, f2, w, h, G.ALPHA, G.LAM, 3, 3)
    eg = T.interior_epe(gu, gv, w, h, tu, tv)
    print(f"layered: TV-L1 on the device {e:.4f} px, GN pyramid {eg:.4f} px, ratio {e / eg:.3f} (bound 0.25)")
    assert e <= 0.25 * eg


def test_quality_shift_and_brightness():
    """(5, 3) px shift: EPE <= 0.02 px at both gammas.  With a smooth 30 % brightness bump on frame
    1: gamma = 0.1 gives <= 0.03 px, gamma = 0 at least ten times that.  The restatement gives
    0.0028 / 0.0057 and 0.0110 / 0.452."""
    e = {}
    for bright in (False, True):
        f1, f2 = T.shift_pair(bright)
        for gamma in T.GAMMAS:
            e[bright, gamma] = device_epe(f1, f2, 5.0, 3.0, gamma=gamma)
            print(f"shift, bump {bright}, gamma {gamma}: interior EPE on the device {e[bright, gamma]:.4f} px")
    assert e[False, 0.0] <= 0.02 and e[False, 0.1] <= 0.02
    assert e[True, 0.1] <= 0.03
    assert e[True, 0.0] >= 10 * e[True, 0.1]


# ------------------------------------------------------------------ the CLI

def test_cli_writes_the_flow_and_its_median(tmp_path):
    """main.py --algo=TVL1 on a 45x37 PNG pair writes the .flo that foto.device.tvl1_flow gives on
    the same uint8 frames, and with --median 2 the one foto.filter.median gives of it (main.py's
    guide and tables; rounding to float32 is monotone, so it commutes with the median)."""
    import main as M
    import utils as U
    from PIL import Image
    from foto import filter as F
    w, h = 45, 37
    paths, frames = [], []
    for k, fr in enumerate(G.frames("45x37")):
        frames.append(np.round(fr.reshape(h, w) * 255).astype(np.uint8))
        paths.append(str(tmp_path / f"f{k}.png"))
        Image.fromarray(frames[-1], "L").save(paths[-1])
    plain, filt = str(tmp_path / "plain.flo"), str(tmp_path / "median.flo")
    outs = []
    for extra in ([f"--out={plain}"], [f"--out={filt}", "--median", "2", "--tv-gamma", "0.1"]):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            M.main(paths + ["--algo=TVL1"] + extra)
        outs.append(buf.getvalue())
    for line in (" - algorithm: TVL1", "\t - lambda=38.0", "\t - theta=0.3", "\t - tau=0.25", "\t - gamma=0.1",
                 "\t - levels=4", "\t - warps=5", "\t - iters=30"):
        assert line in outs[0].splitlines()
    assert " - median filter: radius 2, 1 round(s), guided by f0" in outs[1]
    flow = D.tvl1_flow(DeviceArray.from_numpy(frames[0]), DeviceArray.from_numpy(frames[1]), dtype="float32",
                       layout="interleaved")
    want = flow.to_numpy()

    def flo(path):
        ww, hh, u, v = U.openFlo(path)
        assert (ww, hh) == (w, h)
        return np.ascontiguousarray(np.stack([u, v], axis=-1).reshape(h, w, 2), dtype=np.float32)

    assert np.array_equal(flo(plain).view(np.uint32), want.view(np.uint32))
    guide = U.openGrayscaleImage(paths[0])[0].reshape(h, w)
    sp, rg = M.median_tables(2)
    med, _, _ = F.median(want, in_layout="interleaved", guide=guide, radius=2, spatial=sp, range=rg)
    assert np.array_equal(flo(filt).view(np.uint32), med.view(np.uint32))
    assert not np.array_equal(med, want)   # the filter did something
    tvl1.clear_cache()
