"""Global motion on the device (csrc/foto_motion.hip) against its numpy restatement
(tests/motion_ref.py), bit for bit: the fit on correspondences and on a dense flow, the model
field, the residual flow, the hand-offs from the tracker and to the renderer and the scorer, the
caller's stream and the CLI.

Sizes.  A wavefront is 64 correspondences, a block 256; the scoring kernel works on 512 entries x 32
hypotheses per block and the sums on tiles of FOTO_MOTION_TILE = 1024: M = 63 .. 65 and 257 cross the
first two seams, 1025 is three scoring tiles and one entry more than a summing tile, 1 .. 5 run from
below the minimal sample of every model to above the largest; H = 1 and 7 are less than a chunk of
hypotheses, 256 is eight chunks, 8232 more chunks than the grid holds."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import PKG  # noqa: E402,F401  (puts the package on sys.path)

import motion_ref as R  # noqa: E402
import sparse_ref as S  # noqa: E402
from foto import _lib  # noqa: E402
from foto import device as D  # noqa: E402
from foto import evaluate, motion, render, sparse  # noqa: E402
from foto.device import DeviceArray  # noqa: E402
from foto.synthetic import textured_pair  # noqa: E402

F32, F64 = np.float32, np.float64
W, H = 96, 80
_tables = {}


def table(Hn):
    if Hn not in _tables:
        _tables[Hn] = R.samples(Hn, 11)
        _tables[Hn].setflags(write=False)
    return _tables[Hn]


def dev(a, dtype=F64):
    return DeviceArray.from_numpy(np.ascontiguousarray(a, dtype=dtype))


def same(got, ref, what):
    assert R.same(got, ref), what


def check_fit(fit, ref, what):
    m, mask, info, rms = ref
    same(fit.model.to_numpy().ravel(), m, "model " + what)
    same(fit.inliers.to_numpy(), mask, "mask " + what)
    assert fit.counts() == tuple(int(v) for v in info), "info " + what
    same(np.float64(fit.rms()), np.float64(rms), "rms " + what)


# ------------------------------------------------------------------ fit: sizes, tables, dtypes, status

@pytest.mark.parametrize("model", list(R.MODELS))
@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 63, 64, 65, 257, 1025])
def test_fit_bits(M, model):
    p, d, bad, shift, _ = R.synthetic(model, W, H, M, 0.3, seed=7 * M + R.MODELS[model])
    st = np.zeros(M, dtype=np.uint8)
    st[::3] = [1, 2, 8, 255][R.MODELS[model]]   # a third is unusable: any non-zero byte
    q = p.copy()
    if M >= 5:   # NaN and Inf among the flagged and among the unflagged ones
        q[0, 0], q[3, 1], q[1, 0], q[4, 1] = np.nan, np.inf, np.nan, -np.inf
    e = d.copy()
    if M >= 64:
        e[7, 1], e[9, 0] = np.nan, np.inf
    nones = 0
    for dtype in (F32, F64):
        P, E = q.astype(dtype), e.astype(dtype)
        dP, dE, dS = dev(P, dtype), dev(E, dtype), dev(st, np.uint8)
        for Hn in (1, 7, 256):
            for status in (None, st):
                what = f"{model} M={M} H={Hn} {dtype.__name__} status={status is not None}"
                ref = R.fit(P, E, W, H, model, status=status, table=table(Hn))
                fit = motion.fit(dP, dE, W, H, model, status=None if status is None else dS, samples=table(Hn))
                check_fit(fit, ref, what)
                nones += int(ref[2][3] & R.NONE)
                if M >= 63 and Hn == 256 and status is None:   # the cases find their model
                    assert ref[2][0] >= 0.5 * M and not (ref[2][3] & R.NONE), what
    k = R.k_of(R.MODELS[model])
    if M < k:   # below the minimal sample everything is NONE
        assert nones == 12


def test_fit_mixed_dtypes_rounds_and_options():
    p, d, _, _, _ = R.synthetic("similarity", W, H, 300, 0.4, seed=3)
    dP, dE = dev(p.astype(F32), F32), dev(d)
    for kw in (dict(rounds=0), dict(rounds=1), dict(rounds=6), dict(threshold=0.25), dict(threshold=3.0),
               dict(min_inliers=150), dict(min_inliers=299)):
        ref = R.fit(p.astype(F32), d, W, H, "similarity", table=table(7), **kw)
        check_fit(motion.fit(dP, dE, W, H, "similarity", samples=table(7), **kw), ref, str(kw))
    assert ref[2][3] == R.NONE   # (299 of 300 with 40 % displaced cannot be reached)
    # a frame that is taller than wide, and the default table
    ref = R.fit(p.astype(F32), d, 80, 130, "affine")
    check_fit(motion.fit(dP, dE, 80, 130, "affine"), ref, "80 x 130, default table")


def test_more_hypotheses_than_the_scoring_grid_holds():
    """The scoring grid holds 256 chunks of 32 hypotheses; beyond 8192 a block walks further chunks.
    The last chunk is partial, and the best row stands in the walked part alone."""
    p, d, _, _, _ = R.synthetic("affine", W, H, 70, 0.4, seed=8)
    x, y, X, Y = R.normalise(p[:, 0], p[:, 1], d[:, 0], d[:, 1], W, H)
    t = R.samples(8192 + 40, 5)
    scores = R.fit_list("affine", x, y, X, Y, 70, W, H, t)[4]
    best = t[int(np.argmax(scores))].copy()
    t[scores == scores.max()] = np.repeat(t[:1, :1], 4, axis=1)   # (degenerate rows in their place)
    t[8192 + 37] = best
    ref = R.fit(p, d, W, H, "affine", table=t)
    assert ref[2][2] == 8192 + 37
    check_fit(motion.fit(dev(p), dev(d), W, H, "affine", samples=t), ref, "H = 8232")


# ------------------------------------------------------------------ ties and degeneracy

def test_equal_counts_go_to_the_lower_hypothesis():
    p, d, _, _, _ = R.synthetic("affine", W, H, 120, 0.3, seed=5)
    x, y, X, Y = R.normalise(p[:, 0], p[:, 1], d[:, 0], d[:, 1], W, H)
    t = R.samples(8, 2)
    best = t[int(np.argmax(R.fit_list("affine", x, y, X, Y, 120, W, H, t)[4]))].copy()
    t = np.repeat(t[:, :1], 4, axis=1)           # every row degenerate ...
    t[[3, 5]] = best                             # ... but the best row, twice
    scores = R.fit_list("affine", x, y, X, Y, 120, W, H, t)[4]
    assert list(scores) == [-1, -1, -1, scores[3], -1, scores[3], -1, -1] and scores[3] >= 60
    ref = R.fit(p, d, W, H, "affine", table=t, rounds=0)
    fit = motion.fit(dev(p), dev(d), W, H, "affine", samples=t, rounds=0)
    check_fit(fit, ref, "tie")
    assert fit.counts()[2] == 3
    # every hypothesis the same: the winner is 0
    t[:] = t[3]
    assert motion.fit(dev(p), dev(d), W, H, "affine", samples=t).counts()[2] == 0


@pytest.mark.parametrize("model", ["similarity", "affine", "homography"])
def test_repeated_points_give_none(model):
    p, d, _, _, _ = R.synthetic(model, W, H, 70, 0.0, seed=6)
    t = np.repeat(R.samples(9, 4)[:, :1], 4, axis=1)
    ref = R.fit(p, d, W, H, model, table=t)
    assert list(ref[2]) == [0, 70, -1, R.NONE]
    fit = motion.fit(dev(p), dev(d), W, H, model, samples=t)
    check_fit(fit, ref, "repeated points " + model)
    same(fit.matrix(), np.eye(3), "identity")
    assert not fit.inliers.to_numpy().any() and np.isnan(fit.rms())


def test_all_invalid_gives_none():
    p, d, _, _, _ = R.synthetic("affine", W, H, 70, 0.0, seed=6)
    st = np.full(70, 4, dtype=np.uint8)
    fit = motion.fit(dev(p), dev(d), W, H, "affine", status=dev(st, np.uint8))
    check_fit(fit, R.fit(p, d, W, H, "affine", status=st), "all invalid")
    assert fit.counts() == (0, 0, -1, R.NONE)


def test_residual_exactly_on_the_threshold():
    """64 x 64: s = 32, so threshold / s is exact.  A translation from correspondence 0; the
    residual of correspondence 1, read from the restatement's own numbers, is the threshold: an
    inlier at it, none one ulp below."""
    w = h = 64
    p = np.array([[10.0, 12.0], [40.0, 30.0], [20.0, 50.0]])
    d = np.array([[2.0, 0.0], [2.71828, 0.0], [9.0, 0.0]])
    x, y, X, Y = R.normalise(p[:, 0], p[:, 1], d[:, 0], d[:, 1], w, h)
    tx = X[0] - x[0]
    e = abs((x[1] + tx) - X[1])
    thr = e * 32.0
    assert thr / 32.0 == e and 0.7 < thr < 0.72
    t = np.zeros((1, 4), dtype=np.uint32)        # sample number 0: list entry 0
    for threshold, want in ((thr, [1, 1, 0]), (np.nextafter(thr, 0.0), [1, 0, 0])):
        ref = R.fit(p, d, w, h, "translation", table=t, threshold=threshold, rounds=0)
        assert list(ref[1]) == want
        check_fit(motion.fit(dev(p), dev(d), w, h, "translation", samples=t, threshold=threshold, rounds=0), ref,
                  f"threshold {threshold!r}")


def test_homography_with_a_denominator_that_changes_sign():
    """A true homography whose wv is negative on one side of the points: the exact hypothesis fits
    every correspondence, and only those with wv > 0 are inliers."""
    rng = np.random.default_rng(12)
    mt = np.array([1.0, 0.02, 1.0, -0.01, 1.0, 0.5, -1.0 / 40.0, 0.0, 1.0])
    px = np.concatenate([rng.uniform(2, 30, 30), rng.uniform(50, 94, 30)])
    p = np.column_stack([px, rng.uniform(0, H - 1, 60)])
    ex, ey = R.apply(mt, p[:, 0], p[:, 1])
    d = np.column_stack([ex - p[:, 0], ey - p[:, 1]])
    for rounds in (0, 2):
        ref = R.fit(p, d, W, H, "homography", table=table(7), rounds=rounds)
        assert 20 <= ref[2][0] <= 40 and not (ref[2][3] & R.NONE)
        left, right = ref[1][:30], ref[1][30:]
        assert (left.all() and not right.any()) or (right.all() and not left.any())
        check_fit(motion.fit(dev(p), dev(d), W, H, "homography", samples=table(7), rounds=rounds), ref, "wv sign")


# ------------------------------------------------------------------ fit_flow

def model_flow(w, h, model, seed, dtype, layout, records=1):
    """Flow records of a true model's field with noise, a displaced block and NaN pixels."""
    rng = np.random.default_rng(seed)
    recs = []
    for _ in range(records):
        mt = R.true_matrix(model, w, h, rng)
        u, v = R.field_uv(mt, w, h)
        u, v = u + rng.normal(0, 0.05, u.shape), v + rng.normal(0, 0.05, v.shape)
        u[: h // 3, : w // 3] += 6.0
        v[12, ::5] = np.nan     # (row 12 and column 0 are on the lattice of strides 1, 3 and 4)
        u[12, 12] = np.inf
        m = rng.standard_normal((h, w))
        recs.append(np.stack([u, v, m]) if layout == "planar" else np.stack([u, v], -1))
    return np.stack(recs).astype(dtype)


@pytest.mark.parametrize("w,h,stride", [(33, 17, 1), (33, 17, 3), (96, 80, 4)])
@pytest.mark.parametrize("dtype,layout", [(F32, "planar"), (F64, "interleaved")])
def test_fit_flow_bits(w, h, stride, dtype, layout):
    f = model_flow(w, h, "affine", 20 + stride, dtype, layout, records=2)
    mask = (np.random.default_rng(3).random((h, w)) < 0.8).astype(np.uint8) * 255
    df, dm = dev(f, dtype), dev(mask, np.uint8)
    for model in ("translation", "homography"):
        for record in (0, 1):
            for use_mask in (False, True):
                what = f"{w}x{h} stride {stride} {layout} {model} record {record} mask {use_mask}"
                ref = R.fit_flow(f[record], w, h, model, layout=layout, stride=stride, mask=mask if use_mask else None,
                                 table=table(7))
                fit = motion.fit_flow(df, w, h, record=record, stride=stride, mask=dm if use_mask else None,
                                      model=model, samples=table(7), layout=layout)
                check_fit(fit, ref, what)
                assert ref[1].shape == ((h - 1) // stride + 1, (w - 1) // stride + 1)
                assert ref[2][1] < (ref[1].size if not use_mask else 0.9 * ref[1].size), what   # NaN, Inf, masked: left out
                assert model == "translation" or ref[2][0] > 0.6 * ref[2][1], what      # the homography holds the affine field
    # a single record without a record axis
    check_fit(motion.fit_flow(dev(f[1], dtype), stride=stride, model="affine", samples=table(7), layout=layout),
              R.fit_flow(f[1], w, h, "affine", layout=layout, stride=stride, table=table(7)), "no record axis")


# ------------------------------------------------------------------ field and residual

NEG = np.array([1.0, 0, 0, 0, 1.0, 0, -1.0 / 20.0, 0.002, 1.0])   # wv changes sign at x ~ 20


@pytest.mark.parametrize("w,h", [(33, 17), (96, 80)])
@pytest.mark.parametrize("dtype,layout", [(F32, "planar"), (F64, "planar"), (F32, "interleaved"), (F64, "interleaved")])
def test_field_and_residual_bits(w, h, dtype, layout):
    rng = np.random.default_rng(w)
    ms = np.stack([R.true_matrix("homography", w, h, rng), NEG, R.true_matrix("similarity", w, h, rng)])
    # field: one model, and three records
    one = motion.field(dev(ms[0].reshape(3, 3)), w, h, dtype=dtype, layout=layout).to_numpy()
    same(one, R.field(ms[0], w, h, dtype, layout), "field, one model")
    three = motion.field(dev(ms.reshape(3, 3, 3)), w, h, dtype=dtype, layout=layout).to_numpy()
    ref = R.field(ms, w, h, dtype, layout)
    same(three, ref, "field, three models")
    u = ref[1, 0] if layout == "planar" else ref[1, ..., 0]
    assert np.isnan(u[:, 25:]).all() and np.isfinite(u[:, :19]).all()   # (wv = 0 at x = 20 + 0.04 y)
    # residual: one model for every record, one per record, and a flow without a record axis
    f = model_flow(w, h, "affine", 9, dtype, layout, records=3)
    df = dev(f, dtype)
    same(motion.residual(df, dev(ms[0]), layout=layout).to_numpy(), R.residual(f, ms[0], layout), "residual, count 1")
    got = motion.residual(df, dev(ms), layout=layout).to_numpy()
    want = R.residual(f, ms, layout)
    same(got, want, "residual, a model per record")
    if layout == "planar":
        same(got[:, 2], f[:, 2], "m copied")
    same(motion.residual(dev(f[2], dtype), dev(ms[2]), layout=layout).to_numpy(), R.residual(f[2], ms[2], layout),
         "residual, no record axis")
    with pytest.raises(ValueError):
        motion.residual(df, dev(ms[:2]), layout=layout)


def test_device_argument_errors():
    from foto._lib import FotoError
    p, d, _, _, _ = R.synthetic("affine", W, H, 16, 0.0, seed=1)
    dp, dd = dev(p), dev(d)
    with pytest.raises(FotoError, match="not"):   # a host pointer where device memory is required
        L = _lib.lib()
        o = _lib.MotionOpts(2, 3, 0, 0, 1.0)
        t = R.samples(4, 0)
        host = np.zeros(64)
        _lib.check(L.foto_motion_fit_dev(ctypes.c_void_p(dp.ptr), 2, ctypes.c_void_p(dd.ptr), 2, None, 16, W, H,
                                         ctypes.byref(o), t.ctypes.data_as(ctypes.c_void_p), 4,
                                         ctypes.c_void_p(host.ctypes.data), ctypes.c_void_p(host.ctypes.data + 128),
                                         ctypes.c_void_p(host.ctypes.data + 256), ctypes.c_void_p(host.ctypes.data + 320),
                                         None))
    assert not host.any()
    with pytest.raises(FotoError, match="overlap"):   # the mask over the displacements
        L = _lib.lib()
        out = DeviceArray((3, 3), F64)
        info = DeviceArray((40,), np.uint8)
        _lib.check(L.foto_motion_fit_dev(ctypes.c_void_p(dp.ptr), 2, ctypes.c_void_p(dd.ptr), 2, None, 16, W, H,
                                         ctypes.byref(o), t.ctypes.data_as(ctypes.c_void_p), 4, ctypes.c_void_p(out.ptr),
                                         ctypes.c_void_p(dd.ptr), ctypes.c_void_p(info.ptr),
                                         ctypes.c_void_p(info.ptr + 32), None))
    same(dd.to_numpy(), d, "the displacements are untouched")
    with pytest.raises(ValueError):
        motion.fit(dp, dev(d[:5]), W, H)


# ------------------------------------------------------------------ hand-offs

AFF = np.array([1.012, 0.009, -1.4, -0.007, 0.991, 1.1, 0.0, 0.0, 1.0])   # about the origin, pixels
_pair = {}


def affine_pair():
    """A 96 x 80 texture and the same texture moved by AFF (bilinear, clamped), computed once."""
    if not _pair:
        f0 = textured_pair(W, H, seed=5, dx=0, dy=0, smooth=3)[0].reshape(H, W)
        A = AFF.reshape(3, 3)
        det = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
        yy, xx = np.meshgrid(np.arange(H, dtype=F64), np.arange(W, dtype=F64), indexing="ij")
        bx, by = xx - A[0, 2], yy - A[1, 2]
        sx = np.clip((A[1, 1] * bx - A[0, 1] * by) / det, 0, W - 1)
        sy = np.clip((-A[1, 0] * bx + A[0, 0] * by) / det, 0, H - 1)
        x0, y0 = np.minimum(sx.astype(int), W - 2), np.minimum(sy.astype(int), H - 2)
        ax, ay = sx - x0, sy - y0
        f1 = ((1 - ay) * ((1 - ax) * f0[y0, x0] + ax * f0[y0, x0 + 1])
              + ay * ((1 - ax) * f0[y0 + 1, x0] + ax * f0[y0 + 1, x0 + 1]))
        for a in (f0, f1):
            a.setflags(write=False)
        _pair["f"] = (f0, f1)
    return _pair["f"]


def ref_chain(f0, f1, K, model):
    pts, n, _ = S.corners(f0.ravel(), W, H, K)
    d, st, _, _ = S.track_checked(f0.ravel(), f1.ravel(), W, H, pts.astype(F32), dtype=F32)
    return pts.astype(F32), d, st, R.fit(pts.astype(F32), d, W, H, model, status=st)


def test_corners_lk_fit_chain():
    """corners -> LK with the forward-backward check -> fit, nothing downloaded in between (the
    corner count stays on the device: the NaN rows beyond it reach the fit as unusable)."""
    f0, f1 = affine_pair()
    pts, d, st, ref = ref_chain(f0, f1, 64, "affine")
    a, b = dev(f0), dev(f1)
    fit, gp, gd, gst = D.global_motion(a, b, "affine", 64)
    same(gp.to_numpy(), pts, "chain corners")
    same(gd.to_numpy(), d, "chain d")
    same(gst.to_numpy(), st, "chain status")
    check_fit(fit, ref, "chain fit")
    n_in, n_valid, _, status = fit.counts()
    assert n_valid >= 12 and n_in >= 0.7 * n_valid and status == 0 and n_valid < 64
    # the known affine map is found: its field to a few hundredths of a pixel over the frame
    ut, vt = R.field_uv(AFF, W, H)
    u, v = R.field_uv(fit.matrix().ravel(), W, H)
    err = max(np.abs(u - ut).max(), np.abs(v - vt).max())
    print(f"chain: {n_in} of {n_valid} inliers, rms {fit.rms():.4f}, field error {err:.4f} px")
    assert err < 0.25
    # the stages called one by one give the same bits
    p1, _ = sparse.corners(a, 64, dtype=F32, wait=False)
    with sparse.LK(W, H) as lk:
        lk.set_frames(a, b)
        d1, s1, _, _ = lk.track(p1, check=True, dtype=F32)
        check_fit(motion.fit(p1, d1, W, H, "affine", status=s1), ref, "stages")


def test_field_feeds_reconstruct_and_residual_feeds_score():
    f0, f1 = affine_pair()
    ref = ref_chain(f0, f1, 64, "affine")[3]
    fit = D.global_motion(dev(f0), dev(f1), "affine", 64)[0]
    fld = motion.field(fit, W, H, dtype=F64)
    same(fld.to_numpy(), R.field(ref[0], W, H, F64), "field of the fit")
    got = render.reconstruct(dev(f1), fld, dtype=F64).to_numpy()
    want = render.reconstruct(dev(f1), dev(R.field(ref[0], W, H, F64)), dtype=F64).to_numpy()
    same(got, want, "stabilised frame")
    # a dense flow fitted on the lattice; its residual scored against zero over the inliers' pixels
    flow = model_flow(W, H, "affine", 31, F32, "planar")[0]
    df = dev(flow, F32)
    ff = motion.fit_flow(df, stride=1, model="affine")
    res = motion.residual(df, ff)
    same(res.to_numpy(), R.residual(flow, R.fit_flow(flow, W, H, "affine", stride=1)[0]), "residual of the fit")
    sc = evaluate.score_flow(res, dev(np.zeros((3, H, W), F32), F32), gt_layout="planar", mask=ff.inliers)
    assert sc is not None


def test_fit_on_the_callers_stream():
    """The fit is enqueued on a caller's non-blocking stream right after the LK calls that make its
    inputs, with no synchronisation in between; the results are read after that stream alone."""
    f0, f1 = affine_pair()
    ref = ref_chain(f0, f1, 64, "homography")[3]
    _lib.lib()
    hip = ctypes.CDLL(D.mapped_hip_runtimes()[0])   # the runtime libfoto is bound to
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(stream), 1) == 0   # hipStreamNonBlocking
    try:
        a, b = dev(f0), dev(f1)
        assert hip.hipDeviceSynchronize() == 0   # (the uploads went through the null stream)
        fit = D.global_motion(a, b, "homography", 64, stream=stream.value)[0]
        again = D.global_motion(a, b, "homography", 64, stream=stream.value, samples=R.samples(256, 0))[0]
        assert hip.hipStreamSynchronize(stream) == 0
        check_fit(fit, ref, "caller's stream")
        check_fit(again, ref, "caller's stream, second call")
    finally:
        assert hip.hipStreamDestroy(stream) == 0


# ------------------------------------------------------------------ the command line

def _quiet_main(argv):
    import main as M
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = M.main(argv)
    return res, buf.getvalue()


def test_cli_global_motion_and_residual(tmp_path):
    import utils
    from PIL import Image
    w, h = 64, 48
    paths = []
    for k, f in enumerate(textured_pair(w, h, seed=5, dx=2, dy=1, smooth=3)):
        paths.append(str(tmp_path / f"f{k}.png"))
        Image.fromarray(np.uint8(np.round(255 * f.reshape(h, w))), "L").save(paths[-1])
    plain, out0 = _quiet_main(paths + ["--algo=TVL1"])
    rf = str(tmp_path / "residual.flo")
    (u, v, m), out1 = _quiet_main(paths + ["--algo=TVL1", "--global-motion", "affine", f"--save-residual-flow={rf}"])
    for a, b in zip(plain, (u, v, m)):
        same(a, b, "the solve is the same")
    # without the flags the run prints what it printed; with them, two lines more
    strip = lambda s: [l for l in s.splitlines() if not l.startswith(" - time:")]
    extra = [l for l in strip(out1) if l not in strip(out0)]
    assert len(extra) == 2 and extra[0].startswith(" - global motion (affine): ") and extra[1] == "saving residual flo file..."
    assert [l for l in strip(out1) if l not in extra] == strip(out0)
    flow = np.stack([u.reshape(h, w), v.reshape(h, w), np.zeros((h, w))])
    fit = motion.fit_flow(dev(flow), stride=4, model="affine")
    want = motion.residual(dev(flow), fit).to_numpy()
    fw, fh, ru, rv = utils.openFlo(rf)
    assert (fw, fh) == (w, h)
    same(np.asarray(ru, F32).ravel(), want[0].astype(F32).ravel(), "residual u in the file")
    same(np.asarray(rv, F32).ravel(), want[1].astype(F32).ravel(), "residual v in the file")
    nums = extra[0].split(": ")[1].split(" / ")[0].split()
    same(np.array([float(x) for x in nums]), fit.matrix().ravel(), "the printed matrix")
    n_in, n_valid, _, _ = fit.counts()
    assert float(extra[0].rsplit(": ", 1)[1]) == n_in / n_valid and n_in > 0.5 * n_valid
    with pytest.raises(SystemExit):
        _quiet_main(paths + ["--algo=TVL1", f"--save-residual-flow={rf}"])
