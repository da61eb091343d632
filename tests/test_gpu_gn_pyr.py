"""Coarse-to-fine GN on the device (csrc/foto_gn_pyr.hip) against the numpy restatement of the
scheme (tests/gn_pyr_ref.py: the oracle's gn_assemble and gn_neg_lap, scipy's spsolve): the four
kernels one by one, the increment solve, the whole pyramid, its quality on displacements the
single solve cannot follow, and the device-buffer path."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import PKG  # noqa: E402,F401  (puts the package on sys.path)

import gn_pyr_ref as R  # noqa: E402
from foto import gn, render  # noqa: E402
from foto import device as D  # noqa: E402
from foto.device import DeviceArray  # noqa: E402
from foto.synthetic import textured_pair  # noqa: E402
from oracle import foto_oracle as O  # noqa: E402

SIZES = [(2, 2), (3, 5), (33, 17), (71, 77)]
OP_TOL = 1e-13   # the project's operator tolerance, times max(1, max|ref|)


def close(got, ref, tol, what):
    ref = np.asarray(ref)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what
    bound = tol * max(1.0, np.abs(ref[~nan]).max())
    err = np.abs(np.asarray(got)[~nan] - ref[~nan]).max()
    print(f"{what}: max abs diff {err:.3e} (bound {bound:.3e})")
    assert err <= bound, what


def smooth_field(rng, w, h, amp):
    jj, ii = np.meshgrid(np.arange(h) / max(h - 1, 1), np.arange(w) / max(w - 1, 1), indexing="ij")
    a, b, c, d = rng.uniform(-1, 1, 4)
    return (amp * (a * np.sin(3.0 * ii + b) + c * np.cos(2.0 * jj + d)) / 2).ravel()


# ------------------------------------------------------------------ the kernels

@pytest.mark.parametrize("w,h", SIZES)
def test_pyr_down_bits(w, h):
    rng = np.random.default_rng(w * 100 + h)
    f1, f2 = rng.random(w * h), rng.random(w * h)
    c1, c2 = gn.pyr_down(f1, f2, w, h)
    assert np.array_equal(c1, R.down(f1, w, h)) and np.array_equal(c2, R.down(f2, w, h))


@pytest.mark.parametrize("odd", [0, 1])
@pytest.mark.parametrize("wc,hc", SIZES)
def test_pyr_up(wc, hc, odd):
    w, h = 2 * wc - odd, 2 * hc - odd
    rng = np.random.default_rng(wc * 100 + hc)
    c = [rng.uniform(-4, 4, wc * hc) for _ in range(3)]
    got = gn.pyr_up(*c, wc, hc, w, h)
    for g, r, name in zip(got, R.up(*c, wc, hc, w, h), "uvm"):
        close(g, r, OP_TOL, f"up {name} {wc}x{hc} -> {w}x{h}")


@pytest.mark.parametrize("w,h", SIZES)
def test_pyr_warp(w, h):
    """Sub-pixel displacements everywhere, then exact integers, far out of frame on all four sides
    and one NaN at chosen pixels (2 x 2 has four pixels: the NaN, two far ones that cover the four
    sides between them, and one with an integer x and a sub-pixel y)."""
    n = w * h
    rng = np.random.default_rng(w * 100 + h)
    f2 = rng.random(n)
    u, v, m = rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(-0.3, 0.3, n)
    special = [(np.nan, 0.25), (-1e6, 1e6), (1e6, -1e6), (-1.0, -0.5)]
    if n > 4:
        special += [(1.0, 1.0), (-2.0, 0.0), (0.0, 3.0), (-1e6, 0.3), (1e6, 0.3), (0.3, -1e6), (0.3, 1e6),
                    (float(w), float(h)), (0.5, 0.5)]
    for k, (du, dv) in enumerate(special):
        i = (k * n) // len(special)
        u[i], v[i] = du, dv
    ref = R.warp(f2, u, v, m, w, h)
    assert np.isnan(ref).sum() == 1
    close(gn.warp_prior(f2, u, v, m, w, h), ref, OP_TOL, f"warp {w}x{h}")


# ------------------------------------------------------------------ the increment solve

@pytest.mark.parametrize("w,h", [(33, 17), (71, 77)])
def test_solve_prior(w, h):
    """One increment solve with a random smooth prior against spsolve of the modified system, at
    the goldens' 1e-7; a zero prior is Plan.solve bit for bit."""
    f1, f2 = textured_pair(w, h, seed=5, dx=1.2, dy=-0.7, smooth=3)
    rng = np.random.default_rng(w)
    prior = (smooth_field(rng, w, h, 0.8), smooth_field(rng, w, h, 0.8), smooth_field(rng, w, h, 0.05))
    g = R.warp(f2, *prior, w, h)
    ref = R.solve_inc(f1, g, w, h, R.ALPHA, R.LAM, prior)
    u, v, m, info, its = gn.solve_prior(f1, g, w, h, R.ALPHA, R.LAM, prior)
    assert info == 0 and its > 0
    for a, b, name in zip((u, v, m), ref, "uvm"):
        print(f"solve_prior {w}x{h} {name}: max abs diff {np.abs(a - b).max():.3e}, {its} PCG its")
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-7)
    with gn.Plan(w, h, R.ALPHA, R.LAM) as p:
        want = p.solve(f1, f2)
    zero = (np.zeros(w * h),) * 3
    for pr in (zero, None):
        got = gn.solve_prior(f1, f2, w, h, R.ALPHA, R.LAM, pr)
        assert got[3] == want[3] and got[4] == want[4]
        for a, b in zip(got[:3], want[:3]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("w,h", [(40, 30), (71, 77)])
def test_one_level_one_warp_is_plan_solve(w, h):
    f1, f2 = textured_pair(w, h)
    with gn.Plan(w, h, R.ALPHA, R.LAM) as p:
        want = p.solve(f1, f2)
    with gn.Pyramid(w, h, R.ALPHA, R.LAM, levels=1, warps=1) as q:
        assert q.sizes == [(w, h)]
        u, v, m, info, st = q.solve(f1, f2)
    assert info == want[3] == 0 and st["iterations"] == [want[4]] and st["levels"] == 1 and st["solves"] == 1
    for a, b in zip((u, v, m), want[:3]):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------ the whole pyramid

_gpu = {}


def gpu_flow(case):
    """The device pyramid's flow of a case, solved once per process and shared (read-only)."""
    if case not in _gpu:
        w, h, _, _, levels, warps = R.CASES[case]
        f1, f2 = R.frames(case)
        with gn.Pyramid(w, h, R.ALPHA, R.LAM, levels=levels, warps=warps) as p:
            assert p.sizes == R.sizes(w, h, levels)
            u, v, m, info, st = p.solve(f1, f2)
        assert info == 0 and st["info"] == [0] * (len(p.sizes) * warps) and st["solves"] == len(p.sizes) * warps
        print(f"{case}: PCG its {st['iterations']}, ms per level {['%.2f' % t for t in st['ms_level']]}, "
              f"own steps {st['ms_new']:.2f} ms, total {st['ms_total']:.2f} ms")
        for a in (u, v, m):
            a.setflags(write=False)
        _gpu[case] = (u, v, m)
    return _gpu[case]


@pytest.mark.parametrize("case", ["96x80", "71x77", "45x37"])
def test_pyramid_matches_restatement(case):
    """atol = 1e-6 max(1, max|ref|), test_gn_solve_multilevel's: perturbing every solve of the
    restatement by +-1e-7 moved its final flow by at most 2.2e-7 on these cases, so the scheme does
    not amplify the per-solve PCG error.  Measured on an MI355X: 3.4e-11, 1.3e-11
    and 1.8e-11; the test prints what it sees."""
    ref = R.reference(case)
    worst = 0.0
    for a, b, name in zip(gpu_flow(case), ref, "uvm"):
        d = np.abs(a - b).max()
        worst = max(worst, d / max(1.0, np.abs(b).max()))
        print(f"{case} {name}: max abs diff {d:.3e} (max|ref| {np.abs(b).max():.3f})")
    print(f"{case}: worst diff / max(1, max|ref|) = {worst:.3e} (bound 1e-6)")
    for a, b in zip(gpu_flow(case), ref):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-6 * max(1.0, np.abs(b).max()))


@pytest.mark.parametrize("case", ["96x80", "71x77"])
def test_pyramid_quality(case):
    """Displacements of 5 to 6 px: the single solve is > 2 px short, the pyramid within 0.1 px
    (mean endpoint error, 10 px border off), and the clipped reconstruction's intensity error
    falls below a quarter."""
    w, h, (dx, dy), _, _, _ = R.CASES[case]
    f1, f2 = R.frames(case)
    u0, v0, m0, info, _ = gn.solve(f1, f2, w, h, R.ALPHA, R.LAM)
    assert info == 0
    u, v, m = gpu_flow(case)
    e0, e = R.interior_epe(u0, v0, w, h, dx, dy), R.interior_epe(u, v, w, h, dx, dy)
    src = DeviceArray.from_numpy(f1.reshape(h, w))

    def ie(flow):
        fl = DeviceArray.from_numpy(np.stack([np.asarray(a).reshape(h, w) for a in flow]))
        rec = render.reconstruct(src, fl, dtype="float64").to_numpy()
        return O.IE(w, h, rec.ravel(), f2)

    ie0, ie1 = ie((u0, v0, m0)), ie((u, v, m))
    print(f"{case}: EPE single {e0:.3f} px, pyramid {e:.4f} px; IE single {ie0:.2f}, pyramid {ie1:.2f}")
    assert e0 > 2.0 and e < 0.1
    assert ie1 < 0.25 * ie0


# ------------------------------------------------------------------ the device path

def strided_u8(f, w, h):
    """One channel of an interleaved [h][w][3] uint8 frame (stride_x = 3) and its float64 values."""
    q = np.round(255 * f.reshape(h, w)).astype(np.uint8)
    hwc = np.zeros((h, w, 3), np.uint8)
    hwc[:, :, 1] = q
    return DeviceArray.from_numpy(hwc)[:, :, 1], (np.float64(q) / 255).ravel()


def strided_f32(f, w, h):
    """A row-padded float32 frame (stride_y = w + 5) and its float64 values."""
    q = np.float32(f.reshape(h, w))
    pad = np.zeros((h, w + 5), np.float32)
    pad[:, :w] = q
    return DeviceArray.from_numpy(pad)[:, :w], np.float64(q).ravel()


@pytest.mark.parametrize("frames", ["uint8", "float32"])
def test_solve_device(frames):
    case = "45x37"
    w, h, _, _, levels, warps = R.CASES[case]
    make = strided_u8 if frames == "uint8" else strided_f32
    (d1, h1), (d2, h2) = (make(f, w, h) for f in R.frames(case))
    with gn.Pyramid(w, h, R.ALPHA, R.LAM, levels=levels, warps=warps) as p:
        u, v, m, info, _ = p.solve(h1, h2)
        assert info == 0
        want = np.float32(np.stack([u, v, m]).reshape(3, h, w))
        out, info, st = p.solve_device(d1, d2, dtype="float32", layout="planar", stats=True)
        assert info == 0 and st["solves"] == levels * warps and out.shape == (3, h, w)
        assert np.array_equal(out.to_numpy(), want)
        mine = DeviceArray((h, w, 2), np.float32)
        got, info, st = p.solve_device(d1, d2, out=mine, dtype="float32", layout="interleaved")
        assert got is mine and info == 0 and st is None
        assert np.array_equal(mine.to_numpy(), np.moveaxis(want[:2], 0, 2))
        # both are flow buffers foto.render takes as they are
        src = DeviceArray.from_numpy(h1.reshape(h, w))
        assert render.reconstruct(src, out).shape == (h, w)
        assert render.reconstruct(src, mine, layout="interleaved", use_m=False).shape == (h, w)
    # the cached pyramid behind foto.device.gn_flow, and the drop-in's extension
    flow = D.gn_flow(d1, d2, R.ALPHA, R.LAM, levels=levels, warps=warps)
    assert np.array_equal(flow.to_numpy(), want)
    import classical
    g = classical.GLLOpticalFlow(w, h)
    g.setAlpha(R.ALPHA)
    g.setLambda(R.LAM)
    g.setPyramid(levels, warps)
    for a, b in zip(g.assemble(h1, h2).process(), (u, v, m)):
        assert np.array_equal(a, b)
    gn.clear_plan_cache()


def test_reused_pyramid_equals_fresh():
    """A second pair on the same Pyramid (its plans carry the first pair's iteration predictions
    and buffers) equals a fresh Pyramid's result bit for bit."""
    w, h, levels, warps = 71, 77, 3, 2
    a = textured_pair(w, h, seed=1, dx=3.0, dy=1.0, smooth=5)
    b = R.frames("71x77")
    with gn.Pyramid(w, h, R.ALPHA, R.LAM, levels=levels, warps=warps) as p:
        p.solve(*a)
        second = p.solve(*b)
    assert second[3] == 0
    for x, y in zip(second[:3], gpu_flow("71x77")):
        assert np.array_equal(x, y)


def test_identical_frames_give_zero():
    w, h = 71, 77
    f1, _ = R.frames("71x77")
    d1 = DeviceArray.from_numpy(f1.reshape(h, w))
    with gn.Pyramid(w, h, R.ALPHA, R.LAM, levels=3, warps=2) as p:
        u, v, m, info, st = p.solve(f1, f1)
        assert info == 0 and st["solves"] == 6 and st["iterations"] == [0] * 6 and st["info"] == [0] * 6
        for a in (u, v, m):
            assert not a.any()
        out, info, st = p.solve_device(d1, d1, dtype="float64", stats=True)
        assert info == 0 and st["iterations"] == [0] * 6 and st["info"] == [0] * 6
        assert not out.to_numpy().any()
