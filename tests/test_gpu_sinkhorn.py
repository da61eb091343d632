"""Entropic transport on the device (csrc/foto_sinkhorn.hip) against its numpy restatement
(tests/sinkhorn_ref.py), bit for bit: the scalings a and b, the forward and backward flows in the
four output forms, `valid`, `bad` and `unreachable`; the record's four float sums within w h 2^-53
sum |terms| of their exactly rounded values, the bound of any summation order.

Sizes.  The fused kernel works on tiles of TX x TY = 64 x 32 pixels (a wave is one row of a tile,
a thread eight consecutive rows of a column) with a halo of R on every side in LDS; the two-pass
form and the sums on flat blocks of 256 pixels.  (2, 2) and (5, 3) are smaller than the window on
both sides for every R > 2; (TX - 1, TY + 1) = (63, 33) has an incomplete tile in x and a second
tile row of one line; (64, 32) is exactly one tile; (65, 31) has a second tile of one column and
an incomplete tile in y; (2 TX + 1, 2 TY + 1) = (129, 65) is a 3 x 3 grid with interior seams on
both axes, whose halos read across two neighbours at R = 32.  R = 0 (the kernel is the identity),
1, 7 and the largest, 32, whose LDS image is the 144 KiB the kernel is sized for.  eps = 1, 2, 8;
0, 1, 3 and 25 iterations, run as 0 + 1 + 2 + 22 on one context.  Both forms of the half-iteration
(FOTO_SK_FUSED = 0, the default, and 1) run every one of these cases."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import PKG  # noqa: E402,F401  (puts the package on sys.path)

import sinkhorn_ref as R  # noqa: E402
from foto import _lib  # noqa: E402
from foto import device as D  # noqa: E402
from foto import evaluate, render, sinkhorn  # noqa: E402
from foto.device import DeviceArray  # noqa: E402
from foto.synthetic import textured_pair, translating_gaussian  # noqa: E402

F32, F64 = np.float32, np.float64
TX, TY = sinkhorn.TILE_W, sinkhorn.TILE_H
SIZES = [(2, 2), (5, 3), (TX - 1, TY + 1), (TX, TY), (TX + 1, TY - 1), (2 * TX + 1, 2 * TY + 1)]
FORMS = [(F32, "planar"), (F64, "planar"), (F32, "interleaved"), (F64, "interleaved")]


def dev(a, dtype=F64):
    return DeviceArray.from_numpy(np.ascontiguousarray(a, dtype=dtype))


def same(got, ref, what):
    assert R.same(got, ref), what


def frames(w, h, seed):
    """Seeded random frames, each with a block of exact zeros (elsewhere in the other frame; one
    pixel in the frames that are smaller than a block)."""
    rng = np.random.default_rng(seed)
    f0, f1 = rng.random((h, w)) + 0.05, rng.random((h, w)) + 0.05
    bh, bw = (5, 6) if min(w, h) >= 16 else (1, 1)
    f0[h // 4:h // 4 + bh, w // 3:w // 3 + bw] = 0.0
    f1[h // 2:h // 2 + bw, w // 2:w // 2 + bh] = 0.0
    return f0, f1


def record(u, v, dtype, layout):
    if layout == "planar":
        return np.stack([u, v, np.zeros_like(u)]).astype(dtype)
    return np.stack([u, v], axis=-1).astype(dtype)


def check_state(s, ref, what, forms=FORMS):
    """Everything the context can give against the restatement."""
    a, b = s.scalings()
    same(a.to_numpy(), ref.a, "a " + what)
    same(b.to_numpy(), ref.b, "b " + what)
    for direction in ("forward", "backward"):
        u, v, ok = ref.flow(direction)
        for dtype, layout in forms:
            fl, valid = s.flow(direction, dtype=dtype, layout=layout, valid=True)
            same(fl.to_numpy(), record(u, v, dtype, layout), f"{direction} flow {dtype.__name__} {layout} {what}")
            same(valid.to_numpy(), ok, f"{direction} valid {what}")
    check_info(s.info(), ref, what)


def check_info(got, ref, what):
    want, bounds = ref.info(), ref.sum_bounds()
    assert (got.bad, got.unreachable, got.iterations) == (want["bad"], want["unreachable"], want["iterations"]), what
    for name, bound in zip(("mass0", "mass1", "marginal_error", "cost"), bounds):
        g, w_ = getattr(got, name), want[name]
        print(f"{what} {name}: {g!r} against {w_!r}, bound {bound:.3e}")
        assert abs(g - w_) <= bound, f"{name} {what}"
    assert got.w2 == np.sqrt(2.0 * got.cost)


# ------------------------------------------------------------------ sizes, radii, eps, iteration counts

@pytest.mark.parametrize("fused", ["0", "1"], ids=["two-pass", "fused"])
@pytest.mark.parametrize("eps", [1.0, 2.0, 8.0])
@pytest.mark.parametrize("radius", [0, 1, 7, 32])
@pytest.mark.parametrize("w,h", SIZES)
def test_bits(w, h, radius, eps, fused, monkeypatch):
    monkeypatch.setenv("FOTO_SK_FUSED", fused)   # (read once, when the context is made)
    f0, f1 = frames(w, h, 1000 * w + 10 * radius + int(eps))
    ref = R.Ref(w, h, eps, radius).set_frames(f0, f1)
    case = SIZES.index((w, h)) + radius + int(eps)
    with sinkhorn.Sinkhorn(w, h, eps, radius) as s:
        s.set_frames(dev(f0), dev(f1))
        for k, more in enumerate((0, 1, 2, 22)):   # 0, 1, 3, 25 iterations
            s.iterate(more)
            ref.iterate(more)
            # (every form at the ends, one form -- a different one per case -- in between)
            forms = FORMS if k in (0, 3) else [FORMS[(case + k) % 4]]
            check_state(s, ref, f"{w}x{h} R={radius} eps={eps} it={ref.iterations}", forms)


# ------------------------------------------------------------------ inputs

def test_zero_band_wider_than_the_window_is_unreachable():
    """R = 1: a pixel of frame 0 with mass whose whole 3 x 3 window lies in a zero block of frame 1
    sees b = 0 there, s = 0: unreachable, valid = 0, flow 0."""
    w, h = TX + 1, TY + 1
    f0, f1 = frames(w, h, 3)
    f0[:] = np.maximum(f0, 0.05)
    f1[10:15, 60:65] = 0.0   # 5 x 5, across the tile seam in x: its inner 3 x 3 is out of reach
    ref = R.Ref(w, h, 2.0, 1).set_frames(f0, f1).iterate(3)
    with sinkhorn.Sinkhorn(w, h, 2.0, 1) as s:
        s.set_frames(dev(f0), dev(f1)).iterate(3)
        check_state(s, ref, "zero band")
        i = s.info()
        fl, valid = s.flow(dtype=F64, valid=True)
    valid, fl = valid.to_numpy(), fl.to_numpy()
    assert i.unreachable >= 9 and not valid[11:14, 61:64].any() and valid[9, 59] == 1
    assert not fl[:2, 11:14, 61:64].any()


def test_bad_pixels_count_as_zero():
    w, h = TX + 3, 9
    f0, f1 = frames(w, h, 4)
    f0[0, 0], f0[3, TX], f0[8, w - 1], f0[2, 2] = -0.25, np.nan, np.inf, -np.inf
    f1[1, 1], f1[4, TX - 1] = np.nan, -1e-300
    ref = R.Ref(w, h, 2.0, 7).set_frames(f0, f1).iterate(3)
    assert ref.bad == 6
    for dtype in (F32, F64):
        g0, g1 = f0.astype(dtype), f1.astype(dtype)
        ref = R.Ref(w, h, 2.0, 7).set_frames(g0.astype(F64), g1.astype(F64)).iterate(3)
        with sinkhorn.Sinkhorn(w, h, 2.0, 7) as s:
            s.set_frames(dev(g0, dtype), dev(g1, dtype)).iterate(3)
            check_state(s, ref, f"bad pixels {dtype.__name__}", FORMS[1:2])
            assert s.info().bad == ref.bad >= 5


def test_constant_frame_and_equal_frames():
    w, h = TX + 1, TY + 1
    c = np.full((h, w), 0.5)
    f0, _ = frames(w, h, 5)
    for x, y, what in ((c, c, "constant"), (f0, f0, "mu = nu"), (c, f0, "constant against random")):
        ref = R.Ref(w, h, 2.0, 7).set_frames(x, y).iterate(3)
        with sinkhorn.Sinkhorn(w, h, 2.0, 7) as s:
            s.set_frames(dev(x), dev(y)).iterate(3)
            check_state(s, ref, what, FORMS[1:3])


def test_strided_uint8_float32_float64_frames():
    """A row stride larger than w, in the three frame dtypes; uint8 frames are pixel / 255."""
    w, h, pad = TX + 1, TY + 1, 7
    rng = np.random.default_rng(6)
    for dtype in (np.uint8, F32, F64):
        if dtype == np.uint8:
            big = [rng.integers(0, 256, (h, w + pad), dtype=np.uint8) for _ in range(2)]
            vals = [b[:, :w].astype(F64) / 255.0 for b in big]
        else:
            big = [(rng.random((h, w + pad)) + 0.05).astype(dtype) for _ in range(2)]
            vals = [b[:, :w].astype(F64) for b in big]
        d0, d1 = (dev(b, dtype)[:, :w] for b in big)
        assert not d0.contiguous
        ref = R.Ref(w, h, 2.0, 7).set_frames(*vals).iterate(3)
        with sinkhorn.Sinkhorn(w, h, 2.0, 7) as s:
            s.set_frames(d0, d1).iterate(3)
            check_state(s, ref, f"strided {np.dtype(dtype).name}", FORMS[:1])


# ------------------------------------------------------------------ continuing, resetting, the two forms

def test_iterate_in_parts_and_set_frames_resets():
    w, h = 2 * TX + 1, TY + 1
    f0, f1 = frames(w, h, 7)
    with sinkhorn.Sinkhorn(w, h, 2.0, 7) as s, sinkhorn.Sinkhorn(w, h, 2.0, 7) as t:
        s.set_frames(dev(f0), dev(f1)).iterate(3).iterate(3).iterate(3)
        t.set_frames(dev(f1), dev(f0)).iterate(4)          # another pair first: set_frames starts again
        t.set_frames(dev(f0), dev(f1))
        assert t.info().iterations == 0
        same(t.scalings()[1].to_numpy(), np.ones((h, w)), "b = 1 after set_frames")
        t.iterate(9)
        for x, y in zip(s.scalings(), t.scalings()):
            same(x.to_numpy(), y.to_numpy(), "3 + 3 + 3 against 9")
        assert s.info() == t.info() and s.info().iterations == 9
        same(s.flow(dtype=F64).to_numpy(), t.flow(dtype=F64).to_numpy(), "flows")


def test_contexts_of_different_radii_side_by_side():
    """A context with the largest LDS image keeps working after one with the smallest is made."""
    w, h = TX + 1, TY + 1
    f0, f1 = frames(w, h, 11)
    with sinkhorn.Sinkhorn(w, h, 2.0, 32) as big:
        big.set_frames(dev(f0), dev(f1)).iterate(1)
        with sinkhorn.Sinkhorn(w, h, 2.0, 0) as small:
            small.set_frames(dev(f0), dev(f1)).iterate(2)
            big.iterate(1)
            check_state(small, R.Ref(w, h, 2.0, 0).set_frames(f0, f1).iterate(2), "R = 0 beside R = 32", FORMS[1:2])
            check_state(big, R.Ref(w, h, 2.0, 32).set_frames(f0, f1).iterate(2), "R = 32 beside R = 0", FORMS[1:2])


@pytest.mark.parametrize("radius", [0, 7, 32])
def test_two_pass_form_equals_the_fused_form(radius, monkeypatch):
    """FOTO_SK_FUSED, read once when the context is made: 0 (the default) runs a half-iteration as a
    row kernel and a column + divide kernel through a scratch image, 1 as one LDS-tiled launch.  The
    same bits, and the restatement's."""
    w, h = 2 * TX + 1, 2 * TY + 1
    f0, f1 = frames(w, h, 8 + radius)
    ref = R.Ref(w, h, 2.0, radius).set_frames(f0, f1).iterate(3)
    monkeypatch.setenv("FOTO_SK_FUSED", "0")
    with sinkhorn.Sinkhorn(w, h, 2.0, radius) as two:
        monkeypatch.setenv("FOTO_SK_FUSED", "1")
        with sinkhorn.Sinkhorn(w, h, 2.0, radius) as fused:
            for s in (two, fused):
                s.set_frames(dev(f0), dev(f1)).iterate(3)
            for x, y, z in zip(two.scalings(), fused.scalings(), (ref.a, ref.b)):
                same(x.to_numpy(), y.to_numpy(), "two-pass against fused")
                same(x.to_numpy(), z, "two-pass against the restatement")
            check_state(two, ref, f"two-pass R={radius}", FORMS[1:2])


# ------------------------------------------------------------------ hand-offs

def gaussians(w=40, h=24):
    f0, f1 = translating_gaussian(w, h)
    return f0.reshape(h, w), f1.reshape(h, w)


def test_flow_feeds_score_and_reconstruct():
    w, h = 40, 24
    f0, f1 = gaussians()
    with sinkhorn.Sinkhorn(w, h, 2.0, 12) as s:
        fl, valid = s.set_frames(dev(f0), dev(f1)).iterate(40).flow(valid=True)
        gt = np.zeros((3, h, w), F32)
        gt[0] = 4.0
        sc = evaluate.score_flow(fl, dev(gt, F32), gt_layout="planar", mask=valid)
        assert sc is not None
        rec = render.reconstruct(dev(f1), fl, dtype=F64).to_numpy()
    assert rec.shape == (h, w) and np.isfinite(rec).all()


def test_device_one_shot_matches_the_context():
    w, h = TX + 1, TY + 1
    f0, f1 = frames(w, h, 9)
    d0, d1 = dev(f0), dev(f1)
    ref = R.Ref(w, h, 8.0, 7).set_frames(f0, f1).iterate(5)
    u, v, _ = ref.flow()
    for dtype, layout in FORMS:
        got = D.sinkhorn_flow(d0, d1, eps=8.0, radius=7, iters=5, dtype=dtype, layout=layout)
        same(got.to_numpy(), record(u, v, dtype, layout), f"sinkhorn_flow {dtype.__name__} {layout}")
    with sinkhorn.Sinkhorn(w, h, 8.0, 7) as s:
        same(s.set_frames(d0, d1).iterate(5).flow(dtype=F64).to_numpy(), record(u, v, F64, "planar"), "context")
        hu, hv, hm = s.solve(f0.ravel(), f1.ravel(), 5)
        same(hu.reshape(h, w), u, "host solve u")
        same(hv.reshape(h, w), v, "host solve v")
        assert not hm.any()
    sinkhorn.clear_cache()


def test_on_the_callers_stream():
    """Every call is enqueued on a caller's non-blocking stream with no synchronisation in between;
    the results are read after that stream alone."""
    w, h = 2 * TX + 1, TY + 1
    f0, f1 = frames(w, h, 10)
    ref = R.Ref(w, h, 2.0, 7).set_frames(f0, f1).iterate(6)
    u, v, ok = ref.flow()
    _lib.lib()
    hip = ctypes.CDLL(D.mapped_hip_runtimes()[0])   # the runtime libfoto is bound to
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(stream), 1) == 0   # hipStreamNonBlocking
    try:
        a, b = dev(f0), dev(f1)
        assert hip.hipDeviceSynchronize() == 0   # (the uploads went through the null stream)
        with sinkhorn.Sinkhorn(w, h, 2.0, 7) as s:
            st = stream.value
            s.set_frames(a, b, stream=st).iterate(2, stream=st).iterate(4, stream=st)
            fl, valid = s.flow(dtype=F64, valid=True, stream=st)
            rec = s.info_device(stream=st)
            sa, sb = s.scalings(stream=st)
            one = s.solve_device(a, b, 6, dtype=F64, stream=st)
            assert hip.hipStreamSynchronize(stream) == 0
            same(fl.to_numpy(), record(u, v, F64, "planar"), "flow on the caller's stream")
            same(valid.to_numpy(), ok, "valid on the caller's stream")
            same(sa.to_numpy(), ref.a, "a on the caller's stream")
            same(sb.to_numpy(), ref.b, "b on the caller's stream")
            same(one.to_numpy(), record(u, v, F64, "planar"), "one shot on the caller's stream")
            r = rec.to_numpy()
            assert r[6] == 6 and r[7] == 0 and abs(r[3] - ref.info()["cost"]) <= ref.sum_bounds()[3]
    finally:
        assert hip.hipStreamDestroy(stream) == 0


def test_divergence_on_the_translating_gaussian():
    """The three costs within the sum bound of the restatement's, and with them the condition the
    host test shows the restatement to meet: w2_debiased / sqrt(mass) within 1e-3 of the 4 px shift."""
    w, h = 40, 24
    f0, f1 = gaussians()
    (c01, c00, c11), refs = R.costs(f0, f1, w, h, 2.0, 12, 60)
    d = sinkhorn.divergence(f0, f1, eps=2.0, radius=12, iters=60)
    for got, want, ref, what in ((d.cost01, c01, refs[0], "cost01"), (d.cost00, c00, refs[1], "cost00"),
                                 (d.cost11, c11, refs[2], "cost11")):
        print(f"{what}: {got!r} against {want!r}, bound {ref.sum_bounds()[3]:.3e}")
        assert abs(got - want) <= ref.sum_bounds()[3], what
    assert d.divergence == d.cost01 - 0.5 * d.cost00 - 0.5 * d.cost11
    assert d.w2_debiased == np.sqrt(2.0 * max(d.divergence, 0.0))
    print("w2_debiased / sqrt(mass) =", d.w2_debiased / np.sqrt(d.mass0))
    assert abs(d.w2_debiased / np.sqrt(d.mass0) - 4.0) <= 1e-3 * 4.0
    # device frames give the same record
    assert sinkhorn.divergence(dev(f0), dev(f1), eps=2.0, radius=12, iters=60) == d


# ------------------------------------------------------------------ errors that need the device

def test_state_and_device_argument_errors():
    w, h = 8, 6
    with sinkhorn.Sinkhorn(w, h, 2.0, 2) as s:
        for call in (lambda: s.iterate(1), lambda: s.flow(), lambda: s.info(), lambda: s.scalings()):
            with pytest.raises(_lib.FotoError, match="no frames"):
                call()
        with pytest.raises(ValueError):
            s.set_frames(dev(np.ones((h, w + 1))), dev(np.ones((h, w + 1))))
        s.set_frames(dev(np.ones((h, w))), dev(np.ones((h, w))))
        with pytest.raises(ValueError):
            s.iterate(-1)
        with pytest.raises(ValueError):
            s.flow("sideways")
        L = _lib.lib()
        host = np.zeros(3 * w * h)
        assert L.foto_sinkhorn_flow_dev(s._p, 0, ctypes.c_void_p(host.ctypes.data), _lib.FOTO_F64, 0, None,
                                        None) == _lib.FOTO_ERR_ARG
        assert L.foto_sinkhorn_info_dev(s._p, ctypes.c_void_p(host.ctypes.data), None) == _lib.FOTO_ERR_ARG
        assert L.foto_sinkhorn_iterate_dev(s._p, -1, None) == _lib.FOTO_ERR_ARG
        out = DeviceArray((3, h, w), F64)
        assert L.foto_sinkhorn_flow_dev(s._p, 2, ctypes.c_void_p(out.ptr), _lib.FOTO_F64, 0, None, None) == _lib.FOTO_ERR_ARG
        assert s.iterate(1).info().iterations == 1   # (the context is untouched by the errors)


# ------------------------------------------------------------------ the command line

def _quiet_main(argv):
    import main as M
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = M.main(argv)
    return res, buf.getvalue()


def test_cli_writes_the_restatements_flow(tmp_path):
    import utils
    from PIL import Image
    w, h = 48, 40
    paths = []
    for k, f in enumerate(textured_pair(w, h, seed=5, dx=2, dy=1, smooth=3)):
        paths.append(str(tmp_path / f"f{k}.png"))
        Image.fromarray(np.uint8(np.round(255 * f.reshape(h, w))), "L").save(paths[-1])
    flo = str(tmp_path / "sk.flo")
    (u, v, m), out = _quiet_main(paths + ["--algo=sinkhorn", "--sk-eps=2", "--sk-radius=5", "--sk-iters=7", f"--out={flo}"])
    assert " - algorithm: sinkhorn" in out and "\t - radius=5" in out
    g0, g1 = (utils.openGrayscaleImage(p)[0] for p in paths)
    ru, rv, _ = R.Ref(w, h, 2.0, 5).set_frames(g0, g1).iterate(7).flow()
    same(np.asarray(u).reshape(h, w), ru, "u of the run")
    same(np.asarray(v).reshape(h, w), rv, "v of the run")
    assert not np.asarray(m).any()
    fw, fh, fu, fv = utils.openFlo(flo)
    assert (fw, fh) == (w, h)
    same(np.asarray(fu, F32).ravel(), ru.astype(F32).ravel(), "u in the file")
    same(np.asarray(fv, F32).ravel(), rv.astype(F32).ravel(), "v in the file")
    sinkhorn.clear_cache()
