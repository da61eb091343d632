"""Sparse tracking on the device (csrc/foto_sparse.hip) against its numpy restatement
(tests/sparse_ref.py), bit for bit: the corner response and the corner list, pyramidal
Lucas-Kanade, a dense flow sampled at points, the hand-off to the transport's point tracking and
the CLI.

Sizes.  The response kernel works on 32 x 16 tiles and the candidate kernels on 1024 pixels per
block: 96 x 80 is several of both, 33 x 35 is one pixel more than a tile in each direction and its
pyramid with min_size = 8 ends at 9 x 9, smaller than a 15 x 15 window."""
import contextlib
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import PKG  # noqa: E402,F401  (puts the package on sys.path)

import sparse_ref as S  # noqa: E402
import tvl1_ref as T  # noqa: E402
from foto import device as D  # noqa: E402
from foto import sparse  # noqa: E402
from foto.device import DeviceArray  # noqa: E402
from foto.synthetic import textured_pair  # noqa: E402

F32, F64 = np.float32, np.float64
_frames = {}


def frames(w, h):
    """The pair of a size, computed once and shared (read-only): the (5, 3) px shift of tvl1_ref at
    96 x 80, a (2, 1) px shift elsewhere."""
    if (w, h) not in _frames:
        pair = T.shift_pair(False) if (w, h) == (96, 80) else textured_pair(w, h, seed=5, dx=2, dy=1, smooth=3)
        for a in pair:
            a.setflags(write=False)
        _frames[w, h] = pair
    return _frames[w, h]


def dev(a, dtype=F64):
    return DeviceArray.from_numpy(np.ascontiguousarray(a, dtype=dtype))


def same(got, ref, what):
    assert S.same(got, ref), what


# ------------------------------------------------------------------ corners

@pytest.mark.parametrize("nms", [1, 5])
@pytest.mark.parametrize("window", [1, 3])
@pytest.mark.parametrize("w,h", [(96, 80), (33, 35)])
def test_response_and_corner_list(w, h, window, nms):
    f = frames(w, h)[0]
    d = dev(f.reshape(h, w))
    margin = 8 if w == 96 else 4   # (33 x 35 keeps 25 x 27 pixels; a box of radius 3 plus the gradient fits in 4)
    ref_all, n_all, R = S.corners(f, w, h, 4096, window=window, nms=nms, margin=margin)
    # (33 x 35 at c = 3, s = 5 has a single candidate; every other case has some to choose from)
    assert n_all >= (1 if (w, window, nms) == (33, 3, 5) else 4)
    for max_count, dtype in ((4096, F64), (max(1, n_all // 2), F32), (n_all, F64)):
        ref, n_ref, _ = S.corners(f, w, h, max_count, window=window, nms=nms, margin=margin)
        pts, count, resp = sparse.corners(d, max_count, window=window, nms=nms, margin=margin, return_response=True,
                                          dtype=dtype)
        same(resp.to_numpy(), R, f"response {w}x{h} c={window}")
        assert count == n_ref == min(n_all, max_count)
        same(pts.to_numpy(), ref.astype(dtype), f"corners {w}x{h} c={window} s={nms} max_count={max_count}")
    # the device count alone: no host wait, the same number
    pts, cnt = sparse.corners(d, 4096, window=window, nms=nms, margin=margin, wait=False, dtype=F64)
    assert sparse.device_count(cnt) == n_all
    same(pts.to_numpy(), ref_all, "corners, device count")


def test_corners_tile_ties():
    """Identical 16 x 16 tiles: the strongest candidates tie exactly; below their number the lowest
    raster indices survive."""
    from test_sparse_host import tile_frame, W, H
    frame = tile_frame()
    idx = S.candidates(S.response(frame.ravel(), W, H))
    d = dev(frame)
    for max_count in (3, len(idx) - 1, len(idx) + 5):
        ref, n_ref, _ = S.corners(frame.ravel(), W, H, max_count)
        pts, count = sparse.corners(d, max_count, dtype=F64)
        assert count == n_ref
        same(pts.to_numpy(), ref, f"tile ties, max_count={max_count}")
    pts, count = sparse.corners(dev(np.full((H, W), 0.37)), 16)
    assert count == 0 and np.isnan(pts.to_numpy()).all()


def test_corners_dtypes_and_strides():
    w, h = 96, 80
    f = frames(w, h)[0].reshape(h, w)
    u8 = np.uint8(np.round(255 * f))
    ref8, n8, R8 = S.corners((u8 / 255.0).ravel(), w, h, 64)
    pts, count, resp = sparse.corners(dev(u8, np.uint8), 64, return_response=True, dtype=F64)
    same(resp.to_numpy(), R8, "uint8 response")
    assert count == n8 and n8 >= 8
    same(pts.to_numpy(), ref8, "uint8 corners")
    f32 = f.astype(F32)
    ref32, n32, _ = S.corners(f32.astype(F64).ravel(), w, h, 64)
    pts, count = sparse.corners(dev(f32, F32), 64, dtype=F64)
    assert count == n32
    same(pts.to_numpy(), ref32, "float32 corners")
    # strided views: every second column of a wider array, and a transposed frame
    wide = np.zeros((h, 2 * w))
    wide[:, ::2] = f
    ref, n, _ = S.corners(f.ravel(), w, h, 64)
    pts, count = sparse.corners(dev(wide)[:, ::2], 64, dtype=F64)
    assert count == n
    same(pts.to_numpy(), ref, "strided corners")
    pts, count = sparse.corners(dev(np.ascontiguousarray(f.T)).T, 64, dtype=F64)
    same(pts.to_numpy(), ref, "transposed corners")


# ------------------------------------------------------------------ Lucas-Kanade

def points(w, h, M, R, seed):
    """Pixel centres, sub-pixel positions, within R of each border, outside the frame, one NaN."""
    rng = np.random.default_rng(seed)
    P = np.column_stack([rng.uniform(-3, w + 2, M), rng.uniform(-3, h + 2, M)])
    special = [(np.nan, 10.25), (w // 2, h // 2), (w // 2 + 0.5, h // 2 + 0.25), (R - 1, h // 2), (w - R, h // 2 + 0.5),
               (w // 3, R - 2.5), (w // 3, h - 1), (0, 0), (-2.0, 5.0), (w + 1.5, h + 3.0), (np.inf, 4.0)]
    k = min(M, len(special))
    P[:k] = special[:k] if M > 1 else [(w // 2 + 0.5, h // 2 + 0.25)]
    return P


@pytest.mark.parametrize("iters", [1, 10])
@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("radius", [1, 4, 7])
def test_lk_bits(radius, levels, iters):
    w, h = 96, 80
    f0, f1 = frames(w, h)
    P = points(w, h, 203, radius, seed=radius * 100 + levels * 10 + iters)
    opts = dict(radius=radius, levels=levels, iters=iters)
    with sparse.LK(w, h, **opts) as lk:
        lk.set_frames(dev(f0.reshape(h, w)), dev(f1.reshape(h, w)))
        for direction in (0, 1):
            d, st, err, _ = S.lk_track(f0, f1, w, h, P, direction=direction, **opts)
            gd, gst, gerr, _ = lk.track_raw(dev(P), direction=direction, dtype=F64)
            what = f"R={radius} levels={levels} iters={iters} direction={direction}"
            same(gd.to_numpy(), d, "d " + what)
            same(gst.to_numpy(), st, "status " + what)
            same(gerr.to_numpy(), err, "err " + what)
            assert np.isnan(d[0]).all() and np.isnan(d[10]).all() and np.isfinite(np.delete(d, [0, 10], 0)).all()


@pytest.mark.parametrize("M", [1, 5, 1000])
def test_lk_counts_dtypes_and_the_check(M):
    """M not a multiple of the four points of a block; float32 points and displacements; the
    forward-backward path: the prior, fb and the status OR."""
    w, h = 96, 80
    f0, f1 = frames(w, h)
    P = points(w, h, M, 7, seed=M).astype(F32)
    with sparse.LK(w, h) as lk:
        lk.set_frames(dev(f0.reshape(h, w)), dev(f1.reshape(h, w)))
        for dtype in (F32, F64):
            d, st, err, fb = S.track_checked(f0, f1, w, h, P, fb_tol=0.5, dtype=dtype)
            gd, gst, gerr, gfb = lk.track(dev(P, F32), check=True, fb_tol=0.5, dtype=dtype)
            same(gd.to_numpy(), d, f"d M={M} {dtype.__name__}")
            same(gst.to_numpy(), st, "status after the check")
            same(gerr.to_numpy(), err, "err")
            same(gfb.to_numpy(), fb, "fb")
        # the OR: bits the caller's buffer already has stay
        d, st, _, _ = S.lk_track(f0, f1, w, h, P)
        _, want, _, fb = S.lk_track(f0, f1, w, h, P, direction=1, prior=d, fb_tol=1e-12, status=st | np.uint8(0x40))
        mine = dev(st | np.uint8(0x40), np.uint8)
        _, got, _, gfb = lk.track_raw(dev(P, F32), direction=1, prior=dev(d), fb_tol=1e-12, dtype=F64, status=mine,
                                      err=False, fb=True)
        assert got is mine
        same(got.to_numpy(), want, "status OR")
        same(gfb.to_numpy(), fb, "fb at a tight tolerance")
        assert (want & 0x40).all() and (M == 1 or ((want & S.INCONSISTENT) != 0).any())


def test_lk_window_larger_than_a_level():
    """33 x 35 with min_size = 8: levels 33 x 35, 17 x 18 and 9 x 9; a 15 x 15 window exceeds the last."""
    from foto.gn import pyramid_sizes
    w, h = 33, 35
    assert [tuple(s) for s in pyramid_sizes(w, h, 4, 8)] == [(33, 35), (17, 18), (9, 9)]
    f0, f1 = frames(w, h)
    P = points(w, h, 61, 7, seed=9)
    with sparse.LK(w, h, min_size=8) as lk:
        lk.set_frames(dev(f0.reshape(h, w)), dev(f1.reshape(h, w)))
        d, st, err, fb = S.track_checked(f0, f1, w, h, P, min_size=8)
        gd, gst, gerr, gfb = lk.track(dev(P), check=True, dtype=F64)
        for g, r, name in ((gd, d, "d"), (gst, st, "status"), (gerr, err, "err"), (gfb, fb, "fb")):
            same(g.to_numpy(), r, name + " 33x35")


def test_lk_flat_patch_and_frame_inputs():
    """A flat frame gives FLAT with d = 0; uint8 and strided frames widen like every *_dev entry."""
    w, h = 96, 80
    P = points(w, h, 9, 7, seed=2)
    flat = np.full((h, w), 0.5)
    with sparse.LK(w, h) as lk:
        lk.set_frames(dev(flat), dev(flat))
        gd, gst, gerr = lk.track(dev(P), dtype=F64)
        d, st, err, _ = S.lk_track(flat.ravel(), flat.ravel(), w, h, P)
        same(gd.to_numpy(), d, "flat d")
        same(gst.to_numpy(), st, "flat status")
        same(gerr.to_numpy(), err, "flat err")
        assert (st[1:8] & S.FLAT).all() and not d[1:8].any()
        f0, f1 = (np.uint8(np.round(255 * f.reshape(h, w))) for f in frames(w, h))
        wide = np.zeros((h, 2 * w), dtype=np.uint8)
        wide[:, ::2] = f1
        lk.set_frames(dev(f0, np.uint8), dev(wide, np.uint8)[:, ::2])
        gd, gst, gerr = lk.track(dev(P), dtype=F64)
        d, st, err, _ = S.lk_track((f0 / 255.0).ravel(), (f1 / 255.0).ravel(), w, h, P)
        same(gd.to_numpy(), d, "uint8 d")
        same(gst.to_numpy(), st, "uint8 status")
        same(gerr.to_numpy(), err, "uint8 err")


def test_lk_errors_on_the_device():
    from foto._lib import FotoError
    w, h = 96, 80
    P = dev(points(w, h, 5, 7, seed=1))
    with sparse.LK(w, h) as lk:
        with pytest.raises(FotoError, match="no frames"):
            lk.track(P)
        with pytest.raises(ValueError):
            lk.set_frames(dev(np.zeros((h, w + 1))), dev(np.zeros((h, w + 1))))


# ------------------------------------------------------------------ sampling and hand-off

def test_sample():
    w, h = 33, 35
    rng = np.random.default_rng(4)
    P = points(w, h, 77, 3, seed=5)
    inter = rng.standard_normal((2, h, w, 2)).astype(F32)
    got = sparse.sample(dev(inter, F32), dev(P), layout="interleaved").to_numpy()
    ref = np.stack([S.sample_flow(inter[r, ..., 0], inter[r, ..., 1], w, h, P, F32) for r in range(2)])
    same(got, ref, "sample, 2 float32 interleaved records")
    assert np.isnan(got[:, 0]).all() and np.isfinite(got[:, 1:10]).all()
    planar = rng.standard_normal((3, h, w))
    got = sparse.sample(dev(planar), dev(P.astype(F32), F32)).to_numpy()
    same(got, S.sample_flow(planar[0], planar[1], w, h, P.astype(F32)), "sample, float64 planar")
    got = sparse.sample(dev(planar), dev(P), dtype=F32).to_numpy()
    same(got, S.sample_flow(planar[0], planar[1], w, h, P, F32), "sample, float32 out")


def test_corners_feed_the_transport_tracking():
    """The corners buffer goes into foto.device.bb_track as it is, and lk_track tracks the same
    points."""
    w, h = 48, 40
    f0, f1 = textured_pair(w, h, seed=5, dx=1, dy=0.5, smooth=3)
    a, b = dev(f0.reshape(h, w)), dev(f1.reshape(h, w))
    pts, count = sparse.corners(a, 6, nms=2, dtype=F32)   # (16 candidates at this radius)
    assert count == 6
    tr = D.bb_track(a, b, 4, pts, max_it=3, all_steps=False, dtype=F32).to_numpy()
    assert tr.shape == (1, 6, 2) and np.isfinite(tr).all()
    p2, disp, status, err, fb = D.lk_track(a, b, 6, check=True, dtype=F32, corner_opts=dict(nms=2))
    same(p2.to_numpy(), pts.to_numpy(), "lk_track's corners")
    d, st, e, f = S.track_checked(f0, f1, w, h, pts.to_numpy(), dtype=F32)
    same(disp.to_numpy(), d, "lk_track d")
    same(status.to_numpy(), st, "lk_track status")
    same(fb.to_numpy(), f, "lk_track fb")


def _quiet_main(argv):
    import main as M
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = M.main(argv)
    return res, buf.getvalue()


def test_cli_lk_rows_equal_the_library(tmp_path):
    import main as M
    import utils
    from PIL import Image
    w, h = 64, 48
    paths = []
    for k, f in enumerate(textured_pair(w, h, seed=5, dx=2, dy=1, smooth=3)):
        paths.append(str(tmp_path / f"f{k}.png"))
        Image.fromarray(np.uint8(np.round(255 * f.reshape(h, w))), "L").save(paths[-1])
    gt = str(tmp_path / "gt.flo")
    u, v = np.full(w * h, 2.0), np.full(w * h, 1.0)
    u[:w * 12] = 1e10          # Middlebury's unknown marker on the first rows
    utils.saveFlo(w, h, u, v, gt)
    tracks = str(tmp_path / "tracks.txt")
    _, out = _quiet_main(paths + ["--algo=GN", "--lk", "16", "--lk-radius", "4", "--lk-levels", "2", "--lk-check",
                                  f"--save-tracks={tracks}", f"--ground-truth={gt}"])
    f0, f1 = (utils.openGrayscaleImage(p)[0] for p in paths)
    res = D.lk_track(dev(f0.reshape(h, w)), dev(f1.reshape(h, w)), 16, check=True, dtype=F64, radius=4, levels=2)
    pts, disp, status, err = (x.to_numpy() for x in res[:4])
    rows = open(tracks).read().splitlines()
    assert rows == M.track_rows(pts, disp, status, err) and len(rows) >= 4
    # and the library is the restatement
    ref, n, _ = S.corners(f0, w, h, 16)
    d, st, e, _ = S.track_checked(f0, f1, w, h, ref[:n], radius=4, levels=2)
    same(pts, ref[:n], "CLI corners")
    same(disp, d, "CLI d")
    same(status, st, "CLI status")
    known = int((ref[:n, 1] >= 12).sum())
    assert f" - LK: {n} corners tracked" in out and f" - LK corners with known truth: {known}" in out
    assert 2 <= known < n
    lines = [l for l in out.splitlines() if "EE-mean at the corners" in l]
    assert len(lines) == 2 and lines[0].startswith(" - LK EE-mean") and lines[1].startswith(" - GN EE-mean")
    ee_lk = float(lines[0].split(": ")[1])
    k = ref[:n, 1] >= 12
    assert ee_lk == float(np.hypot(d[k, 0] - 2.0, d[k, 1] - 1.0).mean())
