"""CPU checks of the global-motion stage: the sample table, the C ABI's record, default and argument
errors (no device is touched), and the numpy restatement (tests/motion_ref.py) that the GPU tests
hold the device to bit for bit.  The accuracy facts are checked here, on the restatement: the
device inherits them through bit equality."""
import ctypes

import numpy as np
import pytest

import motion_ref as R

W, H = 96, 80

# The largest difference (px, either component, over the 96 x 80 frame) between the fitted and the
# true model's field, measured with this restatement on the four cases of each model below
# (M in {40, 200} x displaced share in {0.3, 0.5}, seed 1000 + M + 10 share, H = 256, threshold 1,
# noise 0.05 px): the worst case of each model.  The test asserts twice the figure: the fit is
# deterministic, the margin covers a change of fixture seed only.
#   translation 0.0266 (M 40, 50 %)   similarity 0.0402 (M 40, 50 %)
#   affine      0.0857 (M 40, 50 %)   homography 0.0817 (M 40, 50 %)
FIELD_ERR = {"translation": 0.0266, "similarity": 0.0402, "affine": 0.0857, "homography": 0.0817}


# ------------------------------------------------------------------ the sample table

def test_sample_table():
    from foto import motion
    t = motion.samples()
    assert t.dtype == np.uint32 and t.shape == (256, 4) and t.flags.c_contiguous
    assert np.array_equal(t, motion.samples(256, 0)) and np.array_equal(t, R.samples())
    assert not np.array_equal(t, motion.samples(256, 1))
    assert motion.samples(7, 3).shape == (7, 4) and np.array_equal(motion.samples(7, 3), R.samples(7, 3))
    assert len(np.unique(t)) > 1000 and t.max() > 2 ** 31   # the whole uint32 range is drawn from
    with pytest.raises(ValueError):
        motion.samples(0)
    # the lookup is in range for every count, the largest sample number included
    for n in (1, 2, 3, 1025, 2 ** 31 - 1):
        assert (np.uint64(2 ** 32 - 1) * np.uint64(n)) >> np.uint64(32) == n - 1


# ------------------------------------------------------------------ accuracy

@pytest.mark.parametrize("share", [0.3, 0.5])
@pytest.mark.parametrize("M", [40, 200])
@pytest.mark.parametrize("model", list(R.MODELS))
def test_restatement_recovers_the_model(model, M, share):
    p, d, bad, shift, mt = R.synthetic(model, W, H, M, share, seed=1000 + M + int(share * 10))
    m, mask, info, rms = R.fit(p, d, W, H, model)
    ut, vt = R.field_uv(mt, W, H)
    u, v = R.field_uv(m, W, H)
    err = max(np.abs(u - ut).max(), np.abs(v - vt).max())
    found = mask[~bad].mean()
    print(f"{model} M {M} share {share}: info {info}, rms {rms:.4f}, field err {err:.4f}, found {found:.3f}")
    assert not mask[shift > 5.0].any()
    assert found >= 0.9
    assert info[0] == mask.sum() and info[1] == M and info[3] == 0 and 0 <= info[2] < 256
    assert err <= 2 * FIELD_ERR[model]
    assert m[8] == 1.0 and rms < 0.2


# ------------------------------------------------------------------ the restatement's pieces

def test_elimination_order_and_degeneracy():
    rng = np.random.default_rng(5)
    A, b = rng.standard_normal((6, 8, 8)), rng.standard_normal((6, 8))
    p, ok = R.solve(A, b)
    assert ok.all() and np.abs(np.einsum("bij,bj->bi", A, p) - b).max() < 1e-10
    # ties go to the lower row: rows 0 and 1 tie in column 0, no exchange happens
    p, ok = R.solve([[[2.0, 1.0], [-2.0, 3.0]]], [[1.0, 2.0]])
    assert ok[0] and R.same(p[0], np.array([(1.0 - 1.0 * (3.0 / 4.0)) / 2.0, 3.0 / 4.0]))
    # a pivot at the bound is degenerate, just above it is not; NaN is degenerate
    for piv, want in ((1e-12, False), (1.1e-12, True), (np.nan, False), (0.0, False)):
        p, ok = R.solve([[[1.0, 0.0], [0.0, piv]]], [[1.0, 1.0]])
        assert ok[0] == want and np.isnan(p[0]).all() != want


def test_degenerate_samples_repeated_and_collinear():
    rng = np.random.default_rng(6)
    M = 50
    p = np.column_stack([rng.uniform(0, W - 1, M), rng.uniform(0, H - 1, M)])
    d = np.tile([2.0, -1.0], (M, 1))
    x, y, X, Y = R.normalise(p[:, 0], p[:, 1], d[:, 0], d[:, 1], W, H)
    # every hypothesis repeats its first point: similarity, affine and homography are degenerate
    rep = np.repeat(R.samples(16, 1)[:, :1], 4, axis=1)
    for model in ("similarity", "affine", "homography"):
        m, lmask, info, rms, scores, _ = R.fit_list(model, x, y, X, Y, M, W, H, rep)
        assert (scores == -1).all() and list(info) == [0, M, -1, R.NONE]
        assert R.same(m, R.IDENTITY) and not lmask.any() and np.isnan(rms)
    # a translation needs one point: never degenerate
    m, lmask, info, _, scores, _ = R.fit_list("translation", x, y, X, Y, M, W, H, rep)
    assert (scores == M).all() and info[2] == 0 and lmask.all()
    # collinear points: the affine and homography samples are degenerate, the similarity is not
    p[:, 1] = 0.5 * p[:, 0] + 3.0
    x, y, X, Y = R.normalise(p[:, 0], p[:, 1], d[:, 0], d[:, 1], W, H)
    t = R.samples(16, 2)
    for model in ("affine", "homography"):
        scores = R.fit_list(model, x, y, X, Y, M, W, H, t)[4]
        assert (scores == -1).all()
    assert (R.fit_list("similarity", x, y, X, Y, M, W, H, t)[4] >= 0).any()


def test_all_invalid_and_too_few_valid():
    rng = np.random.default_rng(7)
    M = 12
    p = np.column_stack([rng.uniform(0, W - 1, M), rng.uniform(0, H - 1, M)])
    d = np.tile([1.5, 0.5], (M, 1))
    m, mask, info, rms = R.fit(p, d, W, H, "affine", status=np.ones(M, dtype=np.uint8))
    assert R.same(m, R.IDENTITY) and not mask.any() and list(info) == [0, 0, -1, R.NONE] and np.isnan(rms)
    bad = p.copy()
    bad[:, 0] = np.nan
    assert list(R.fit(bad, d, W, H, "translation")[2]) == [0, 0, -1, R.NONE]
    # n_valid < k: two usable correspondences cannot carry an affine map, but carry a similarity
    st = np.ones(M, dtype=np.uint8)
    st[[3, 8]] = 0
    m, mask, info, _ = R.fit(p, d, W, H, "affine", status=st)
    assert list(info) == [0, 2, -1, R.NONE] and not mask.any() and R.same(m, R.IDENTITY)
    m, mask, info, _ = R.fit(p, d, W, H, "similarity", status=st)
    assert info[0] == 2 and info[1] == 2 and list(np.flatnonzero(mask)) == [3, 8]
    assert np.abs(m - [1, 0, 1.5, 0, 1, 0.5, 0, 0, 1]).max() < 1e-9
    # min_inliers above what there is
    assert list(R.fit(p, d, W, H, "translation", min_inliers=M + 1)[2]) == [0, M, -1, R.NONE]
    assert R.fit(p, d, W, H, "translation", min_inliers=M)[2][0] == M


def test_refinement_round_that_loses_its_inliers():
    """Two clusters of a translation 1 px apart, threshold 0.6: the winner holds one cluster; the
    least-squares mean of a start model whose inliers are fewer than k is kept, with the bit."""
    M = 8
    p = np.column_stack([np.linspace(5, 80, M), np.linspace(7, 60, M)])
    d = np.zeros((M, 2))
    d[:, 0] = 3.0
    x, y, X, Y = R.normalise(p[:, 0], p[:, 1], d[:, 0], d[:, 1], W, H)
    far = np.array([1.0, 0, 0.5, 0, 1.0, 0.5, 0, 0, 1.0])   # half a normalised unit off: no inlier
    t2 = (1.0 / 48.0) ** 2
    m, kept = R.refine_round(R.TRANSLATION, far, x, y, X, Y, t2, M)
    assert kept and m is far
    # an affine round on collinear inliers: the normal equations are degenerate, the model is kept
    pc = np.column_stack([np.linspace(5, 80, M), np.full(M, 20.0)])
    x, y, X, Y = R.normalise(pc[:, 0], pc[:, 1], d[:, 0], d[:, 1], W, H)
    start = np.array([1.0, 0, 3.0 / 48.0, 0, 1.0, 0, 0, 0, 1.0])
    assert R.inlier(start, x, y, X, Y, t2).all()
    m, kept = R.refine_round(R.AFFINE, start, x, y, X, Y, t2, M)
    assert kept and m is start
    # a translation of the same points refines without the bit; every affine sample of them is degenerate
    assert R.fit(pc, d, W, H, "translation", rounds=2)[2][3] == 0
    assert list(R.fit_list("affine", x, y, X, Y, M, W, H, R.samples(4, 0))[2]) == [0, M, -1, R.NONE]


def test_sum_order_is_the_tiles():
    rng = np.random.default_rng(8)
    v = rng.standard_normal((3, 2500))
    assert np.abs(R.fsum(v, 2500) - v.sum(axis=1)).max() < 1e-11
    # the padding does not change a bit: the same terms in a longer list
    assert R.same(R.fsum(v[:, :900], 900), R.fsum(v[:, :900], 1024))
    # slots before lanes: entries 0 and 256 meet first, then the wave tree
    t = np.zeros(1024)
    t[0], t[256], t[32] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert R.fsum(t, 1024)[0] == 1.0
    t[256], t[32], t[1], t[33] = 0.0, 0.0, 2.0 ** -53, 2.0 ** -53
    assert R.fsum(t, 1024)[0] == 1.0 + 2.0 ** -52


def test_pixel_matrix_field_and_residual():
    rng = np.random.default_rng(9)
    mt = R.true_matrix("homography", W, H, rng)
    # a model fitted to exact correspondences is the true one to rounding
    p = np.column_stack([rng.uniform(0, W - 1, 30), rng.uniform(0, H - 1, 30)])
    ex, ey = R.apply(mt, p[:, 0], p[:, 1])
    m, mask, info, rms = R.fit(p, np.column_stack([ex - p[:, 0], ey - p[:, 1]]), W, H, "homography")
    assert mask.all() and np.abs(m - mt).max() < 1e-9 and rms < 1e-9
    f = R.field(m, W, H, np.float64)
    assert f.shape == (3, H, W) and not f[2].any()
    assert np.abs(f[0, 10, 20] - (R.apply(m, 20.0, 10.0)[0] - 20.0)) < 1e-12
    fi = R.field(m, W, H, np.float32, "interleaved")
    assert fi.shape == (H, W, 2) and R.same(fi[..., 1], f[1].astype(np.float32))
    # wv changes sign inside the frame: NaN on the far side, and the residual is NaN there too
    neg = np.array([1.0, 0, 0, 0, 1.0, 0, -1.0 / 40.0, 0, 1.0])
    g = R.field(neg, W, H, np.float64)
    assert np.isnan(g[0, :, 40:]).all() and np.isfinite(g[0, :, :40]).all()
    flow = rng.standard_normal((2, 3, H, W))
    r = R.residual(flow, np.stack([m, neg]))
    assert R.same(r[:, 2], flow[:, 2]) and R.same(r[0, 0], flow[0, 0] - f[0]) and np.isnan(r[1, 1, :, 40:]).all()
    assert R.same(R.residual(flow[0], m), r[0])


# ------------------------------------------------------------------ the ABI

def test_abi_record_default_and_exports():
    from foto import _lib, motion
    L = _lib.lib()
    for name in ("foto_motion_opts_default", "foto_motion_fit_dev", "foto_motion_fit_flow_dev",
                 "foto_motion_field_dev", "foto_motion_residual_dev"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert ctypes.sizeof(_lib.MotionOpts) == 24 and _lib.MotionOpts.threshold.offset == 16
    o = _lib.MotionOpts(9, 9, 9, 9, 9.0)
    assert L.foto_motion_opts_default(ctypes.byref(o)) == 0
    assert (o.model, o.rounds, o.min_inliers, o.reserved, o.threshold) == (-1, 3, 0, 0, 1.0)
    assert {k: getattr(o, k) for k in motion.DEFAULTS} == motion.DEFAULTS == R.DEFAULTS
    assert motion.MODELS == R.MODELS == dict(translation=0, similarity=1, affine=2, homography=3)
    assert (motion.NONE, motion.KEPT, _lib.FOTO_MOTION_TILE) == (R.NONE, R.KEPT, R.TILE) == (1, 2, 1024)


def test_argument_errors_without_gpu():
    """Every argument error that needs no device is FOTO_ERR_ARG with a message, found before any
    HIP call: the outputs (host memory here) stay as they were."""
    from foto import _lib
    L = _lib.lib()
    E = _lib.FOTO_ERR_ARG
    f32, f64 = _lib.FOTO_F32, _lib.FOTO_F64
    assert L.foto_motion_opts_default(None) == E
    buf = np.zeros(4096)
    outs = np.full(64, 7.0)
    ptr = ctypes.c_void_p(buf.ctypes.data)
    optr = ctypes.c_void_p(outs.ctypes.data)
    table = R.samples(8, 0)
    tptr = table.ctypes.data_as(ctypes.c_void_p)

    def opts(**kw):
        o = _lib.MotionOpts()
        L.foto_motion_opts_default(ctypes.byref(o))
        o.model = _lib.FOTO_MOTION_AFFINE
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def fit(pts=ptr, pd=f64, disp=ptr, dd=f64, M=16, w=96, h=80, o=True, t=tptr, Hn=8, model=optr, inl=optr, info=optr,
            rms=optr, **kw):
        oo = opts(**kw)
        rc = L.foto_motion_fit_dev(pts, pd, disp, dd, None, M, w, h, ctypes.byref(oo) if o else None, t, Hn, model, inl,
                                   info, rms, None)
        assert rc >= 0 or L.foto_last_error()
        return rc

    for kw in (dict(pts=None), dict(disp=None), dict(o=False), dict(t=None), dict(model=None), dict(inl=None),
               dict(info=None), dict(rms=None), dict(M=0), dict(M=2 ** 31), dict(Hn=0), dict(w=1), dict(h=1),
               dict(pd=_lib.FOTO_U8), dict(dd=7), dict(pts=ctypes.c_void_p(buf.ctypes.data + 8)),
               dict(disp=ctypes.c_void_p(buf.ctypes.data + 4), dd=f32),
               dict(model=ctypes.c_void_p(outs.ctypes.data + 4)), dict(info=ctypes.c_void_p(outs.ctypes.data + 2)),
               dict(rms=ctypes.c_void_p(outs.ctypes.data + 1))):
        assert fit(**kw) == E, kw
    # the options: each field has its range, and the default's model (-1) is no model
    for kw in (dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")),
               dict(rounds=-1), dict(min_inliers=-1)):
        assert fit(**kw) == E, kw
    for bad_model in (-1, 4):
        o = opts()
        o.model = bad_model
        assert L.foto_motion_fit_dev(ptr, f64, ptr, f64, None, 16, 96, 80, ctypes.byref(o), tptr, 8, optr, optr, optr, optr,
                                     None) == E

    fl = _lib.Flow(buf.ctypes.data, f64, 0, 2)

    def fit_flow(flow=fl, record=0, w=8, h=8, stride=2, o=True, t=tptr, Hn=8, model=optr, inl=optr):
        oo = opts()
        rc = L.foto_motion_fit_flow_dev(ctypes.byref(flow) if flow is not None else None, record, w, h, stride, None,
                                        ctypes.byref(oo) if o else None, t, Hn, model, inl, optr, optr, None)
        assert rc >= 0 or L.foto_last_error()
        return rc

    for kw in (dict(flow=None), dict(record=-1), dict(record=2), dict(stride=0), dict(w=1), dict(h=1), dict(o=False),
               dict(t=None), dict(Hn=0), dict(model=None), dict(inl=None), dict(flow=_lib.Flow(buf.ctypes.data, 0, 0, 1)),
               dict(flow=_lib.Flow(buf.ctypes.data, f64, 2, 1)), dict(flow=_lib.Flow(None, f64, 0, 1))):
        assert fit_flow(**kw) == E, kw

    def field(models=ptr, count=1, w=8, h=8, out=optr, dtype=f64, layout=0):
        return L.foto_motion_field_dev(models, count, w, h, out, dtype, layout, None)

    for kw in (dict(models=None), dict(out=None), dict(count=0), dict(w=0), dict(h=0), dict(w=65536, h=32768),
               dict(dtype=_lib.FOTO_U8), dict(layout=2), dict(models=ctypes.c_void_p(buf.ctypes.data + 4)),
               dict(out=ctypes.c_void_p(outs.ctypes.data + 4))):
        assert field(**kw) == E, kw

    def residual(flow=fl, models=ptr, count=1, w=8, h=8, out=optr):
        return L.foto_motion_residual_dev(ctypes.byref(flow) if flow is not None else None, models, count, w, h, out, None)

    for kw in (dict(flow=None), dict(models=None), dict(out=None), dict(count=0), dict(count=3), dict(w=0),
               dict(out=ctypes.c_void_p(outs.ctypes.data + 4))):
        assert residual(**kw) == E, kw
    assert (outs == 7.0).all() and L.foto_last_error()


def test_python_argument_errors():
    from foto import motion
    with pytest.raises(ValueError):
        motion._opts("rigid", 1.0, 3, 0)
    with pytest.raises(ValueError):
        motion._table(np.zeros((4, 4), dtype=np.int64))
    with pytest.raises(ValueError):
        motion._table(np.zeros((0, 4), dtype=np.uint32))
    assert motion._table(None).shape == (256, 4)
