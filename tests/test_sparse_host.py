"""CPU checks of the sparse tracking entries: the CLI's new flags, the C ABI's records, defaults and
argument errors (no device is touched), and the numpy restatement (tests/sparse_ref.py) that the
GPU tests hold the device to bit for bit.  The quality facts are checked here, on the restatement:
the device inherits them through bit equality."""
import ctypes

import numpy as np
import pytest

import sparse_ref as S
import tvl1_ref as T

W, H = 96, 80


# ------------------------------------------------------------------ CLI and ABI

def test_cli_flags_and_defaults():
    import main as M
    a = M.build_parser().parse_args(["a.png", "b.png", "--algo", "GN"])
    assert (a.lk, a.lk_radius, a.lk_levels, a.lk_iters, a.lk_check, a.save_tracks) == (0, 7, 4, 10, False, None)
    a = M.build_parser().parse_args(["a.png", "b.png", "--algo=TVL1", "--lk", "64", "--lk-radius", "4", "--lk-levels=2",
                                     "--lk-iters", "5", "--lk-check", "--save-tracks", "t.txt", "--stats"])
    assert (a.lk, a.lk_radius, a.lk_levels, a.lk_iters, a.lk_check, a.save_tracks) == (64, 4, 2, 5, True, "t.txt")
    # no existing switch changes meaning
    assert (a.tv_levels, a.tv_warps, a.tv_iters, a.gn_levels, a.Nt, a.median, a.stats) == (4, 5, 30, 1, 4, 0, True)
    with pytest.raises(SystemExit):
        M.build_parser().parse_args(["a.png", "b.png", "--lk-radius", "8"])


def test_track_rows_format():
    import main as M
    rows = M.track_rows(np.array([[3.0, 4.0]]), np.array([[0.1, -2.5]]), np.array([9], dtype=np.uint8), np.array([np.nan]))
    assert rows == ["3.0 4.0 0.1 -2.5 9 nan"]


def test_abi_records_defaults_and_signatures():
    from foto import _lib, sparse
    L = _lib.lib()
    for name in ("foto_corner_opts_default", "foto_corners_dev", "foto_lk_opts_default", "foto_lk_create",
                 "foto_lk_destroy", "foto_lk_device", "foto_lk_set_frames_dev", "foto_lk_track_dev",
                 "foto_flow_sample_dev"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    # double, 4 ints; 4 ints, double
    assert ctypes.sizeof(_lib.CornerOpts) == 24 and _lib.CornerOpts.window.offset == 8
    assert ctypes.sizeof(_lib.LKOpts) == 24 and _lib.LKOpts.min_eig.offset == 16
    c = _lib.CornerOpts()
    assert L.foto_corner_opts_default(ctypes.byref(c)) == 0
    assert {k: getattr(c, k) for k in sparse.CORNER_DEFAULTS} == sparse.CORNER_DEFAULTS == S.CORNER_DEFAULTS
    assert S.CORNER_DEFAULTS == dict(quality=0.01, window=3, nms=5, margin=8)
    o = _lib.LKOpts()
    assert L.foto_lk_opts_default(ctypes.byref(o)) == 0
    assert {k: getattr(o, k) for k in sparse.LK_DEFAULTS} == sparse.LK_DEFAULTS == S.LK_DEFAULTS
    assert S.LK_DEFAULTS == dict(radius=7, levels=4, min_size=16, iters=10, min_eig=1e-7)
    assert (sparse.FLAT, sparse.OUT, sparse.NONFINITE, sparse.INCONSISTENT) == (1, 2, 4, 8) == (
        S.FLAT, S.OUT, S.NONFINITE, S.INCONSISTENT)
    assert (_lib.FOTO_CORNER_MAX_WINDOW, _lib.FOTO_CORNER_MAX_NMS, _lib.FOTO_LK_MAX_RADIUS) == (7, 15, 7)
    with pytest.raises(TypeError):
        sparse.cached_lk(8, 8, bicubic=True)


def test_argument_errors_without_gpu():
    """Every argument error that needs no device is FOTO_ERR_ARG with a message, found before any
    HIP call."""
    from foto import _lib
    L = _lib.lib()
    E = _lib.FOTO_ERR_ARG
    assert L.foto_corner_opts_default(None) == E and L.foto_lk_opts_default(None) == E
    p = ctypes.c_void_p()

    def create(w, h, **kw):
        o = _lib.LKOpts()
        L.foto_lk_opts_default(ctypes.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        rc = L.foto_lk_create(w, h, ctypes.byref(o), ctypes.byref(p))
        assert rc >= 0 or L.foto_last_error()
        return rc

    assert create(1, 80) == E and create(96, 1) == E and create(0, 0) == E and create(65536, 32768) == E
    for kw in (dict(radius=0), dict(radius=8), dict(levels=0), dict(min_size=1), dict(iters=0), dict(min_eig=-1.0),
               dict(min_eig=float("nan")), dict(min_eig=float("inf"))):
        assert create(96, 80, **kw) == E, kw
    assert not p.value
    assert L.foto_lk_create(96, 80, None, None) == E
    assert L.foto_lk_device(None) == -1
    buf = np.zeros(4096)
    ptr = ctypes.c_void_p(buf.ctypes.data)
    im = _lib.Image(buf.ctypes.data, _lib.FOTO_F64, 16, 1, 1.0)
    assert L.foto_lk_set_frames_dev(None, ctypes.byref(im), ctypes.byref(im), None) == E
    assert L.foto_lk_track_dev(None, ptr, _lib.FOTO_F64, 4, 0, None, 0.5, ptr, _lib.FOTO_F64, ptr, None, None, None) == E

    def corners(image=im, w=16, h=16, max_count=8, pts=ptr, dtype=_lib.FOTO_F64, count=ptr, **kw):
        o = _lib.CornerOpts()
        L.foto_corner_opts_default(ctypes.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        rc = L.foto_corners_dev(ctypes.byref(image) if image is not None else None, w, h, ctypes.byref(o), max_count,
                                pts, dtype, count, None, None, None)
        assert rc >= 0 or L.foto_last_error()
        return rc

    assert corners(image=None) == E and corners(w=1) == E and corners(h=0) == E and corners(max_count=0) == E
    assert corners(pts=None) == E and corners(count=None) == E and corners(dtype=_lib.FOTO_U8) == E
    assert corners(pts=ctypes.c_void_p(buf.ctypes.data + 8)) == E       # not aligned to a float64 pair
    assert corners(count=ctypes.c_void_p(buf.ctypes.data + 2)) == E
    for kw in (dict(window=0), dict(window=8), dict(nms=0), dict(nms=16), dict(margin=-1), dict(quality=-0.1),
               dict(quality=1.5), dict(quality=float("nan"))):
        assert corners(**kw) == E, kw
    bad = _lib.Image(buf.ctypes.data, 7, 16, 1, 1.0)
    assert corners(image=bad) == E

    fl = _lib.Flow(buf.ctypes.data, _lib.FOTO_F64, 0, 1)
    f64 = _lib.FOTO_F64
    assert L.foto_flow_sample_dev(None, 8, 8, ptr, f64, 4, ptr, f64, None) == E
    assert L.foto_flow_sample_dev(ctypes.byref(fl), 1, 8, ptr, f64, 4, ptr, f64, None) == E
    assert L.foto_flow_sample_dev(ctypes.byref(fl), 8, 8, ptr, f64, 0, ptr, f64, None) == E
    assert L.foto_flow_sample_dev(ctypes.byref(fl), 8, 8, None, f64, 4, ptr, f64, None) == E
    assert L.foto_flow_sample_dev(ctypes.byref(fl), 8, 8, ptr, _lib.FOTO_U8, 4, ptr, f64, None) == E
    assert L.foto_flow_sample_dev(ctypes.byref(fl), 8, 8, ptr, f64, 4, None, f64, None) == E
    assert L.foto_flow_sample_dev(ctypes.byref(_lib.Flow(buf.ctypes.data, f64, 2, 1)), 8, 8, ptr, f64, 4, ptr, f64,
                                  None) == E
    assert L.foto_last_error()


# ------------------------------------------------------------------ the restatement's pieces

def test_box_sum_and_lane_order():
    rng = np.random.default_rng(3)
    P = rng.random((9, 11))
    B = S.box_sum(P, 2)
    Z = np.pad(P, 2)
    want = sum(Z[dy:dy + 9, dx:dx + 11] for dy in range(5) for dx in range(5))
    assert np.abs(B - want).max() < 1e-13 and B[0, 0] == pytest.approx(P[:3, :3].sum())
    for n in (9, 81, 225):
        V = rng.standard_normal((3, n))
        assert np.abs(S.wsum(V) - V.sum(axis=1)).max() < 1e-12
    # the order is the lanes': slot e of lane p = e % 64, then the tree
    V = np.zeros((1, 225))
    V[0, 0], V[0, 64], V[0, 32] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert S.wsum(V)[0] == 1.0            # (1 + 2^-53) rounds to 1, then 1 + 2^-53 again
    V[0, 64], V[0, 32], V[0, 1], V[0, 33] = 0.0, 0.0, 2.0 ** -53, 2.0 ** -53
    assert S.wsum(V)[0] == 1.0 + 2.0 ** -52   # lanes 1 and 33 meet (o = 32) before they reach lane 0 (o = 1)


def test_detector_constant_frame_has_no_corner():
    pts, count, R = S.corners(np.full(W * H, 0.37), W, H, 64)
    assert count == 0 and np.isnan(pts).all() and not R.any()


def test_detector_tile_ties_go_to_the_earlier_pixel():
    """A frame of identical 16 x 16 tiles: bit-equal responses at tile-equivalent pixels (the margin
    keeps every candidate's window inside the frame), so the strongest candidates tie exactly and
    a max_count below their number keeps the lowest raster indices."""
    frame = tile_frame()
    R = S.response(frame.ravel(), W, H)
    assert np.array_equal(R[16:32, 16:32], R[32:48, 48:64]) and np.array_equal(R[16:32, 16:32], R[48:64, 64:80])
    idx = S.candidates(R)
    key = R.ravel()[idx]
    strongest = idx[key == key.max()]
    assert len(strongest) >= 6      # one per tile the margin leaves room for
    k = len(strongest) - 2
    pts, count, _ = S.corners(frame.ravel(), W, H, k)
    assert count == k
    assert np.array_equal(pts[:, 1] * W + pts[:, 0], strongest[:k].astype(np.float64))
    # and with room for all of them the list is every candidate, in raster order
    pts, count, _ = S.corners(frame.ravel(), W, H, 4096)
    assert count == len(idx) and np.array_equal(pts[:count, 1] * W + pts[:count, 0], idx.astype(np.float64))
    assert np.isnan(pts[count:]).all()


def tile_frame():
    rng = np.random.default_rng(21)
    t = rng.random((16, 16))
    for _ in range(2):   # periodic smoothing: the tiling stays exact
        t = (t + np.roll(t, 1, 0) + np.roll(t, -1, 0) + np.roll(t, 1, 1) + np.roll(t, -1, 1)) / 5.0
    return np.tile(t, (H // 16, W // 16))


# ------------------------------------------------------------------ the quality facts

def ee(d, tu, tv):
    return np.hypot(d[:, 0] - tu, d[:, 1] - tv)


def test_quality_shift_needs_the_pyramid():
    """tvl1_ref.shift_pair(False): 96 x 80, a (5, 3) px shift, three levels.  Measured with this
    restatement: 17 corners, max EE 1.2e-14 px, max fb 1.9e-14; with levels = 1 max EE 13.97 px."""
    f0, f1 = T.shift_pair(False)
    pts, count, _ = S.corners(f0, W, H, 64)
    p = pts[:count]
    d, st, err, fb = S.track_checked(f0, f1, W, H, p)
    e = ee(d, 5.0, 3.0)
    print(f"shift: {count} corners, max EE {e.max():.3e}, max fb {fb.max():.3e}, status {sorted(set(st))}")
    assert count >= 8
    assert (e <= 1e-9).all() and (fb <= 1e-9).all()
    assert not st.any()
    d1, _, _, _ = S.lk_track(f0, f1, W, H, p, levels=1)
    e1 = ee(d1, 5.0, 3.0)
    print(f"shift, levels = 1: max EE {e1.max():.3f} px")
    assert e1.max() > 1.0


def test_quality_layered_the_check_finds_the_bad_tracks():
    """tvl1_ref.layered_pair(), the truth read at the corner pixel.  Measured with this restatement:
    18 corners; the 8 with fb < 1e-13 have EE < 1e-13, every other one has EE >= 0.08; the 2 with fb
    > 0.5 have EE 1.37 and 2.19."""
    f0, f1, tu, tv = T.layered_pair()
    pts, count, _ = S.corners(f0, W, H, 64)
    p = pts[:count]
    xi, yi = p[:, 0].astype(int), p[:, 1].astype(int)
    d, st, err, fb = S.track_checked(f0, f1, W, H, p)
    e = ee(d, tu[yi, xi], tv[yi, xi])
    for a, b, c in sorted(zip(fb, e, st)):
        print(f"layered: fb {a:.3e} EE {b:.3e} status {c}")
    tight = fb <= 1e-9
    assert tight.sum() >= 4 and (e[tight] <= 1e-9).all()
    bad = (st & S.INCONSISTENT) != 0
    assert np.array_equal(bad, ~(fb <= 0.5))
    assert (e[bad] > 1.0).all()


def test_status_bits_of_the_restatement():
    f0, f1 = T.shift_pair(False)
    flat = np.full(W * H, 0.5)
    P = np.array([[40.0, 40.0], [np.nan, 3.0], [np.inf, 3.0], [-4.0, 10.0], [40.5, 30.25]])
    d, st, err, _ = S.lk_track(flat, flat, W, H, P)
    assert list(st) == [S.FLAT, S.NONFINITE | S.OUT, S.NONFINITE | S.OUT, S.FLAT | S.OUT, S.FLAT]
    assert np.isnan(d[1:3]).all() and np.isnan(err[1:3]).all() and not d[[0, 3, 4]].any() and not err[[0, 3, 4]].any()
    d, st, err, _ = S.lk_track(f0, f1, W, H, P)
    assert np.isnan(d[1:3]).all() and np.isfinite(d[[0, 3, 4]]).all() and st[0] == 0
