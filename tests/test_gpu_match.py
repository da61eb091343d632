"""Feature matching on the device (csrc/foto_match.hip) against its numpy restatement
(tests/match_ref.py): integers equal, displacements bit for bit -- the descriptors, the Hamming
matcher, the mutual check, the hand-offs from the corner detector and to the fit and the renderer,
the caller's stream and the CLI.

Seams of the matcher.  A block holds FOTO_MATCH_QUERIES = 512 queries (two per lane) and walks its
split of the train set in LDS tiles of FOTO_MATCH_TILE = 256 descriptors; a launch aims at
FOTO_MATCH_BLOCKS = 1024 blocks: with qb = ceil(N0 / 512) query blocks and tiles = ceil(N1 / 256) the
train set is cut into min(tiles, max(1, 1024 / qb)) splits of whole tiles, merged by a second launch.
  the LDS tile     N1 = 255, 256, 257 (and 63 .. 65: a wavefront of staging threads)
  the query block  N0 = 511, 512, 513 (and 255 .. 257: the first of a lane's two queries)
  the train split  N0 <= 512: every tile is a split up to tiles = 1024, N1 = 262144; N1 = 262143,
                   262144, 262145 are one below, at and one above (the last: 513 splits of two tiles)
  the block aim    N0 = 262143, 262144 (qb = 512: two splits), 262145 (qb = 513: one split, so the
                   tile seams lie inside a split); N1 = 1025 there is five tiles, cut 3 + 2
There is no cap on the grid: grid.x = qb <= 2^22, grid.y = the splits <= 1024."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import PKG  # noqa: E402,F401  (puts the package on sys.path)

import match_ref as MR  # noqa: E402
import motion_ref as R  # noqa: E402
from foto import _lib  # noqa: E402
from foto import device as D  # noqa: E402
from foto import match, motion, render  # noqa: E402
from foto.device import DeviceArray  # noqa: E402
from foto.synthetic import textured_pair  # noqa: E402

F32, F64 = np.float32, np.float64
W, H = 96, 80
TILE, QB, BLOCKS = _lib.FOTO_MATCH_TILE, _lib.FOTO_MATCH_QUERIES, _lib.FOTO_MATCH_BLOCKS
_cache = {}


def dev(a, dtype=None):
    return DeviceArray.from_numpy(np.ascontiguousarray(a, dtype=dtype))


def same(got, ref, what):
    assert MR.same(got, ref), what


def frame(w=W, h=H, seed=2):
    key = ("frame", w, h, seed)
    if key not in _cache:
        _cache[key] = textured_pair(w, h, seed, 0, 0)[0].reshape(h, w)
        _cache[key].setflags(write=False)
    return _cache[key]


def table(K, patch):
    key = ("table", K, patch)
    if key not in _cache:
        _cache[key] = MR.pattern(K, patch, 0)
        _cache[key].setflags(write=False)
    return _cache[key]


def point_list(w, h, patch, M, seed):
    """Integer and sub-pixel points, points exactly ``patch`` and ``patch - 1`` from each border,
    .5 fractions (the keypoint pixel rounds them up), NaN and +-Inf, then random ones over a little
    more than the frame."""
    p, q = float(patch), float(patch - 1)
    fixed = [[p, p], [q, p], [p, q], [w - 1 - p, h - 1 - p], [w - p, h - 1 - p], [w - 1 - p, h - p], [p - 0.5, p],
             [p - 0.51, p], [w - 1 - p + 0.49, h - 1 - p], [w - 1 - p + 0.5, h - 1 - p], [p + 0.5, p + 0.5],
             [w / 2 + 0.25, h / 2 - 0.75], [np.nan, p], [p, np.nan], [np.inf, p], [p, -np.inf], [-1e30, 1e30]]
    rng = np.random.default_rng(seed)
    rnd = np.column_stack([rng.uniform(-3, w + 2, M), rng.uniform(-3, h + 2, M)])
    inner = np.column_stack([rng.uniform(p, w - 1 - p, M), rng.uniform(p, h - 1 - p, M)])
    rnd[::2] = inner[::2]
    rnd[::6] = np.round(rnd[::6])
    return np.concatenate([np.array(fixed), rnd])[:M]


def check_describe(F, dF, pts, dtype, what, **kw):
    P = pts.astype(dtype)
    K, patch = kw.get("orientations", 1), kw.get("patch", 15)
    ref = MR.describe(F, P, kw.get("blur", 2), patch, K, table(K, patch))
    got = match.describe(dF, dev(P, dtype), return_bin=True, table=table(K, patch), **kw)
    same(got[1].to_numpy(), ref[1], "state " + what)
    same(got[2].to_numpy(), ref[2], "bin " + what)
    same(got[0].to_numpy(), ref[0], "desc " + what)
    return ref


# ------------------------------------------------------------------ describe

@pytest.mark.parametrize("K", [1, 4, 32])
@pytest.mark.parametrize("patch", [2, 15, 31])
@pytest.mark.parametrize("blur", [0, 2, 3])
def test_describe_bits(blur, patch, K):
    for (w, h) in ((W, H), (64, 63)) if patch == 31 else ((W, H),):
        F = frame(w, h)
        pts = point_list(w, h, patch, 257, 10 * patch + K)
        desc, state, bins = check_describe(F, dev(F), pts, F64, f"{w}x{h} blur {blur} patch {patch} K {K}", blur=blur,
                                           patch=patch, orientations=K)
        assert (state == 0).sum() >= 40 and (state == 2).sum() >= 5 and (state == 6).sum() == 4
        if K > 1 and patch <= 15:
            assert len(np.unique(bins[state == 0])) >= 2   # the orientation path takes more than one bin


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 257])
def test_describe_point_counts_and_dtypes(M, dtype):
    F = frame()
    check_describe(F, dev(F), point_list(W, H, 15, M, M), dtype, f"M {M} {dtype.__name__}", orientations=4)
    desc, state = match.describe(dev(F), dev(point_list(W, H, 15, M, M), dtype), orientations=4)   # (no bin asked for)
    same(state.to_numpy(), MR.describe(F, point_list(W, H, 15, M, M).astype(dtype), 2, 15, 4)[1], "state, no bin")


def test_describe_frame_dtypes_and_strides():
    F = frame()
    pts = point_list(W, H, 15, 65, 3)
    u8 = np.uint8(np.round(255 * F))
    check_describe(u8.astype(F64) / 255.0, dev(u8), pts, F64, "uint8", orientations=4)
    check_describe(F.astype(F32).astype(F64), dev(F, F32), pts, F64, "float32", orientations=4)
    wide = np.zeros((H, 2 * W + 5))
    wide[:, 3:3 + 2 * W:2] = F
    check_describe(F, dev(wide)[:, 3:3 + 2 * W:2], pts, F64, "strided", orientations=4)
    check_describe(F.T.copy(), dev(F).T, point_list(H, W, 15, 65, 4), F64, "transposed view", orientations=4)
    check_describe(u8.astype(F64) / 3.0, D.as_image(dev(u8), divisor=3.0), pts, F64, "a divisor", orientations=4)


def test_describe_nan_pixel_inside_a_patch():
    """A NaN pixel: tests that read it (through the box sum) are false, the moments are NaN and the
    bin is 0; points whose patch does not hold it are as before."""
    F = frame().copy()
    F[40, 50] = np.nan
    pts = np.array([[50.0, 40.0], [52.0, 44.0], [60.0, 30.0], [20.0, 60.0], [80.0, 64.0]])
    for blur in (0, 2):
        desc, state, bins = check_describe(F, dev(F), pts, F64, f"NaN pixel, blur {blur}", blur=blur, orientations=32)
        assert list(bins[:3]) == [0, 0, 0] and (state == 0).all()
    clean = MR.describe(frame(), pts, 2, 15, 32, table(32, 15))
    same(desc[3:], clean[0][3:], "patches away from the NaN")


# ------------------------------------------------------------------ match

def descriptors(rng, n, pool=24, flips=6):
    """n descriptors around ``pool`` centres, a few bits flipped: small distances and many ties."""
    c = rng.integers(0, 2 ** 64, size=(pool, 4), dtype=np.uint64)
    d = c[rng.integers(0, pool, n)].copy()
    for _ in range(flips):
        on = rng.random(n) < 0.6
        d[np.arange(n), rng.integers(0, 4, n)] ^= np.where(on, np.uint64(1) << rng.integers(0, 64, n).astype(np.uint64),
                                                          np.uint64(0))
    return d


def match_set(n, seed, invalid=0.1):
    """(desc, state, pts float64) of n entries; ``invalid`` of them unusable."""
    key = ("set", n, seed, invalid)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        st = np.where(rng.random(n) < invalid, rng.choice([2, 6], n), 0).astype(np.uint8)
        pts = np.column_stack([rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n)])
        pts[::7] = np.round(pts[::7])
        _cache[key] = (descriptors(rng, n), st, pts)
        for a in _cache[key]:
            a.setflags(write=False)
    return _cache[key]


def check_match(q, t, what, pd=(F32, F32), dtype=F32, ref=None, **kw):
    (d0, s0, p0), (d1, s1, p1) = q, t
    P0, P1 = p0.astype(pd[0]), p1.astype(pd[1])
    rkw = dict(kw)
    rkw["ratio"] = match.ratio_code(kw.get("ratio", 0.8))
    if ref is None:
        ref = MR.match(d0, s0, P0, d1, s1, P1, dtype=dtype, **rkw)
    got = match.match(dev(d0), dev(s0), dev(P0), dev(d1), dev(s1), dev(P1), dtype=dtype, **kw)
    for g, r, name in zip(got, ref, ("idx", "dist", "status", "disp")):
        same(g.to_numpy(), r, f"{name} {what}")
    return ref


SIZES = [1, 2, 63, 64, 65, 257, 1025]


@pytest.mark.parametrize("N0", SIZES)
def test_match_sizes(N0):
    seen = np.zeros(256, dtype=np.int64)
    for N1 in SIZES + [255, 256]:
        idx, dist, status, disp = check_match(match_set(N0, N0), match_set(N1, 1000 + N1), f"{N0} x {N1}", max_dist=40)
        seen += np.bincount(status, minlength=256)
    if N0 >= 63:   # the cases hold rejections of each kind and unusable queries (clean matches: the planted test)
        kinds = np.arange(256)
        assert all(seen[(kinds & bit) != 0].sum() for bit in (MR.NONE, MR.AMBIGUOUS, MR.OUT))


@pytest.mark.parametrize("N0", [255, 256, 511, 512, 513])
def test_match_query_block_seams(N0):
    check_match(match_set(N0, N0), match_set(300, 9), f"{N0} x 300", max_dist=40, max_disp=30.0)


def test_match_options():
    q, t = match_set(257, 1), match_set(300, 2)
    for kw in (dict(max_dist=0), dict(max_dist=256), dict(ratio=None), dict(ratio=1 / 256), dict(ratio=205 / 256),
               dict(ratio=1.0), dict(max_disp=0.5), dict(max_disp=10.0), dict(max_disp=10.0, ratio=None, max_dist=256)):
        check_match(q, t, str(kw), **kw)
    # a gate that excludes everything: the train points are 500 px away
    far = (t[0], t[1], t[2] + 500.0)
    idx, dist, status, disp = check_match(q, far, "gate excludes all", max_disp=10.0)
    assert (idx == -1).all() and (dist == 257).all() and np.isnan(disp).all()
    assert ((status == (MR.NONE | MR.AMBIGUOUS)) | (q[1] != 0)).all()
    # all-invalid train, all-invalid query
    idx, dist, status, _ = check_match(q, (t[0], np.full(300, 2, np.uint8), t[2]), "all-invalid train")
    assert (idx == -1).all() and (dist == 257).all()
    idx, dist, status, _ = check_match((q[0], np.full(257, 6, np.uint8), q[2]), t, "all-invalid query")
    assert (idx == -1).all() and (status == 6).all() and (dist == 257).all()
    # NaN query and train points (corners' rows beyond the count) under a gate and without one
    p0, p1 = q[2].copy(), t[2].copy()
    p0[5], p1[::9] = np.nan, np.nan
    for kw in (dict(), dict(max_disp=25.0)):
        check_match((q[0], q[1], p0), (t[0], t[1], p1), f"NaN points {kw}", max_dist=256, ratio=None, **kw)


@pytest.mark.parametrize("pd", [(F32, F32), (F32, F64), (F64, F32), (F64, F64)])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_match_point_and_disp_dtypes(pd, dtype):
    check_match(match_set(65, 4), match_set(257, 5), f"{pd} -> {dtype}", pd=pd, dtype=dtype, max_dist=256, max_disp=40.0)
    check_match(match_set(65, 4), match_set(257, 5), f"{pd} -> {dtype}, no gate", pd=pd, dtype=dtype, max_dist=256)


def test_planted_duplicates_and_ties_across_seams():
    """Exact duplicates of a query on both sides of the tile seam (255 | 256), which for a small N0
    is a split seam too: the lower index wins and d2 = d1 = 0; one duplicate alone wins with d2 from
    the other side; a unusable duplicate at the lower index is passed over."""
    rng = np.random.default_rng(6)
    q = (rng.integers(0, 2 ** 64, size=(8, 4), dtype=np.uint64), np.zeros(8, np.uint8), np.zeros((8, 2)))
    d1 = rng.integers(0, 2 ** 64, size=(600, 4), dtype=np.uint64)
    s1 = np.zeros(600, np.uint8)
    d1[[255, 256]] = q[0][0]            # across the seam
    d1[[10, 511, 512]] = q[0][1]        # within a tile, and across the next seam
    d1[300] = q[0][2]                   # alone
    d1[[100, 520]] = q[0][3]
    s1[100] = 2                         # the lower duplicate is unusable
    d1[599] = q[0][4]                   # the last entry of a partial tile
    d1[0] = q[0][5]                     # the first
    t = (d1, s1, rng.uniform(0, 90, (600, 2)))
    idx, dist, status, _ = check_match(q, t, "planted", max_dist=256)
    assert list(idx[:6]) == [255, 10, 300, 520, 599, 0]
    assert list(dist[:2].ravel()) == [0, 0, 0, 0] and dist[2, 0] == 0 and dist[2, 1] > 64
    assert list(status[:6]) == [16, 16, 0, 0, 0, 0]
    check_match(q, t, "planted, no ratio", max_dist=256, ratio=None)


def tiled_queries(N0, distinct, seed):
    d, s, p = match_set(distinct, seed)
    reps = -(-N0 // distinct)
    return tuple(np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:N0] for a in (d, s, p))


@pytest.mark.parametrize("N0", [QB * (BLOCKS // 2) - 1, QB * (BLOCKS // 2), QB * (BLOCKS // 2) + 1])
def test_match_block_aim_seam(N0):
    """qb = 512 leaves two splits, qb = 513 one: N1 = 1025 is five tiles, cut 3 + 2 or walked by one
    block.  The queries repeat 257 distinct ones, so the restatement is computed on those."""
    distinct = 257
    q = tiled_queries(N0, distinct, 7)
    d1, s1, p1 = match_set(1025, 8)
    d1 = d1.copy()
    d1[[767, 768, 1024]] = q[0][3]    # ties across the split seam of the 3 + 2 cut (768) and in the last, partial tile
    s1 = s1.copy()
    s1[[767, 768, 1024]] = 0
    t = (d1, s1, p1)
    base = tuple(a[:distinct] for a in q)
    small = MR.match(base[0], base[1], base[2].astype(F32), t[0], t[1], t[2].astype(F32), max_dist=40, ratio=205)
    reps = -(-N0 // distinct)
    ref = tuple(np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:N0] for a in small)
    assert ref[0][3] == 767 or base[1][3] != 0
    check_match(q, t, f"N0 {N0}", ref=ref, max_dist=40)


@pytest.mark.parametrize("N1", [TILE * BLOCKS - 1, TILE * BLOCKS, TILE * BLOCKS + 1])
def test_match_train_split_seam(N1):
    """Up to 1024 tiles every tile is a split; one entry more and a split is two tiles."""
    q = match_set(3, 11, invalid=0.0)
    rng = np.random.default_rng(N1)
    d1 = rng.integers(0, 2 ** 64, size=(N1, 4), dtype=np.uint64)
    d1[[5, N1 - 1]] = q[0][0]                   # a tie between the first and the last split
    d1[N1 - 1 - TILE] = q[0][1]
    s1 = np.zeros(N1, np.uint8)
    s1[::1000] = 2
    s1[[5, N1 - 1, N1 - 1 - TILE]] = 0
    t = (d1, s1, rng.uniform(0, 90, (N1, 2)))
    idx, dist, status, _ = check_match(q, t, f"N1 {N1}", max_dist=256)
    assert idx[0] == 5 and idx[1] == N1 - 1 - TILE and list(dist[0]) == [0, 0]


# ------------------------------------------------------------------ cross

def test_cross_bits():
    rng = np.random.default_rng(12)
    for N0, N1 in ((1, 1), (5, 4), (257, 300), (1025, 63)):
        idx01 = rng.integers(-1, N1, N0).astype(np.int32)
        idx10 = rng.integers(-1, N0, N1).astype(np.int32)
        mutual = rng.random(N1) < 0.5
        has = np.flatnonzero(idx01 >= 0)
        idx10[idx01[has]] = np.where(mutual[idx01[has]], has, idx10[idx01[has]])
        st = rng.choice([0, 0, 1, 16, 6], N0).astype(np.uint8)
        ref = MR.cross(idx01, idx10, st)
        dst = dev(st)
        got = match.cross(dev(idx01), dev(idx10), dst)
        assert got is dst
        same(dst.to_numpy(), ref, f"cross {N0} x {N1}")
    # an idx01 pointing at an entry whose idx10 is -1; an idx01 of -1 is left alone
    idx01, idx10 = np.array([2, -1, 0, 1], np.int32), np.array([2, 3, -1], np.int32)
    st = np.array([0, 1, 16, 0], np.uint8)
    dst = dev(st)
    match.cross(dev(idx01), dev(idx10), dst)
    same(dst.to_numpy(), np.array([8, 1, 16, 0], np.uint8), "idx10 = -1")
    same(dst.to_numpy(), MR.cross(idx01, idx10, st), "idx10 = -1, restated")


def test_device_argument_errors():
    from foto._lib import FotoError
    q, t = match_set(16, 1), match_set(16, 2)
    dq = [dev(a) for a in q]
    dt = [dev(a) for a in t]
    host = np.zeros(64, np.int32)
    L = _lib.lib()
    vp = ctypes.c_void_p
    with pytest.raises(FotoError, match="not"):   # a host pointer where device memory is required
        _lib.check(L.foto_match_dev(vp(dq[0].ptr), vp(dq[1].ptr), vp(dq[2].ptr), 2, 16, vp(dt[0].ptr), vp(dt[1].ptr),
                                    vp(dt[2].ptr), 2, 16, None, vp(host.ctypes.data), vp(host.ctypes.data + 64),
                                    vp(host.ctypes.data + 192), None, 2, None))
    assert not host.any()
    idx, status = DeviceArray((16,), np.int32), DeviceArray((16,), np.uint8)
    with pytest.raises(FotoError, match="overlap"):   # dist over the train descriptors
        _lib.check(L.foto_match_dev(vp(dq[0].ptr), vp(dq[1].ptr), vp(dq[2].ptr), 2, 16, vp(dt[0].ptr), vp(dt[1].ptr),
                                    vp(dt[2].ptr), 2, 16, None, vp(idx.ptr), vp(dt[0].ptr), vp(status.ptr), None, 2,
                                    None))
    same(dt[0].to_numpy(), t[0], "the descriptors are untouched")
    with pytest.raises(ValueError):
        match.match(dq[0], dq[1], dq[2], dt[0], dev(t[1][:5]), dt[2])
    with pytest.raises(ValueError):
        match.describe(dev(frame()), dq[2], table=np.zeros((2, 256, 4), np.int8))


# ------------------------------------------------------------------ hand-offs

SHIFT = (40.5, -24.25)
PW, PH = 128, 96


def shift_pair():
    """test_match_host's shift pair (a), at 128 x 96 (the property holds there: checked on the CPU)."""
    if "pair" not in _cache:
        f0, f1 = textured_pair(PW, PH, 0, SHIFT[0], SHIFT[1])
        _cache["pair"] = (f0.reshape(PH, PW), f1.reshape(PH, PW))
        for a in _cache["pair"]:
            a.setflags(write=False)
        _cache["chain"] = MR.match_frames(f0, f1, PW, PH, 200)
    return _cache["pair"], _cache["chain"]


def check_fit(fit, ref, what):
    m, mask, info, rms = ref
    same(fit.model.to_numpy().ravel(), m, "model " + what)
    same(fit.inliers.to_numpy(), mask, "mask " + what)
    assert fit.counts() == tuple(int(v) for v in info), "info " + what
    same(np.float64(fit.rms()), np.float64(rms), "rms " + what)


def test_match_frames_and_match_motion_chain():
    """corners (both frames) -> describe -> match both ways -> cross -> fit, nothing downloaded in
    between: the corner counts stay on the device, the NaN rows beyond them are marked by describe
    and left out by the matcher and the fit."""
    (f0, f1), ref = shift_pair()
    a, b = dev(f0), dev(f1)
    got = D.match_frames(a, b, 200)
    for g, r, name in zip(got, ref, ("points", "disp", "status", "idx", "dist")):
        same(g.to_numpy(), r, "chain " + name)
    rfit = R.fit(ref[0], ref[1], PW, PH, "translation", status=ref[2])
    fit, gp, gd, gst = D.match_motion(a, b, "translation", 200)
    same(gp.to_numpy(), ref[0], "motion points")
    same(gd.to_numpy(), ref[1], "motion disp")
    same(gst.to_numpy(), ref[2], "motion status")
    check_fit(fit, rfit, "match_motion")
    n_in, n_valid, _, status = fit.counts()
    tx, ty = fit.matrix()[0, 2], fit.matrix()[1, 2]
    print(f"chain: {n_in} of {n_valid} matches are inliers, translation ({tx:.4f}, {ty:.4f})")
    assert status == 0 and n_in >= 4 and abs(tx - SHIFT[0]) <= 0.6904 and abs(ty - SHIFT[1]) <= 0.6904
    assert np.isnan(ref[0]).any()   # (fewer than 200 corners: NaN rows did reach every stage)
    # without the mutual check, and with options passed through
    got = D.match_frames(a, b, 200, check=False, orientations=4, ratio=None, max_disp=60.0, corner_opts=dict(nms=3))
    want = MR.match_frames(f0, f1, PW, PH, 200, check=False, orientations=4, ratio=0, max_disp=60.0,
                           corner_opts=dict(nms=3))
    for g, r, name in zip(got, want, ("points", "disp", "status", "idx", "dist")):
        same(g.to_numpy(), r, "options " + name)
    with pytest.raises(TypeError):
        D.match_frames(a, b, 200, radius=7)


def test_matches_feed_fit_field_and_reconstruct():
    (f0, f1), ref = shift_pair()
    a, b = dev(f0), dev(f1)
    pts, disp, status, _, _ = D.match_frames(a, b, 200)
    rfit = R.fit(ref[0], ref[1], PW, PH, "affine", status=ref[2])
    fit = motion.fit(pts, disp, PW, PH, "affine", status=status)
    check_fit(fit, rfit, "fit of the matches")
    fld = motion.field(fit, PW, PH, dtype=F64)
    same(fld.to_numpy(), R.field(rfit[0], PW, PH, F64), "field of the fit")
    got = render.reconstruct(b, fld, dtype=F64).to_numpy()
    want = render.reconstruct(b, dev(R.field(rfit[0], PW, PH, F64)), dtype=F64).to_numpy()
    same(got, want, "stabilised frame")


def test_match_on_the_callers_stream():
    """Every stage is enqueued on a caller's non-blocking stream with no synchronisation in between;
    the results are read after that stream alone."""
    (f0, f1), ref = shift_pair()
    rfit = R.fit(ref[0], ref[1], PW, PH, "translation", status=ref[2])
    _lib.lib()
    hip = ctypes.CDLL(D.mapped_hip_runtimes()[0])   # the runtime libfoto is bound to
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(stream), 1) == 0   # hipStreamNonBlocking
    try:
        a, b = dev(f0), dev(f1)
        assert hip.hipDeviceSynchronize() == 0   # (the uploads went through the null stream)
        fit, pts, disp, status = D.match_motion(a, b, "translation", 200, stream=stream.value)
        again = D.match_frames(a, b, 200, stream=stream.value)
        assert hip.hipStreamSynchronize(stream) == 0
        check_fit(fit, rfit, "caller's stream")
        same(disp.to_numpy(), ref[1], "caller's stream, disp")
        for g, r, name in zip(again, ref, ("points", "disp", "status", "idx", "dist")):
            same(g.to_numpy(), r, "caller's stream, second call, " + name)
    finally:
        assert hip.hipStreamDestroy(stream) == 0


# ------------------------------------------------------------------ the command line

def _quiet_main(argv):
    import main as M
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = M.main(argv)
    return res, buf.getvalue()


def test_cli_match_global_motion_and_tracks(tmp_path):
    from PIL import Image
    paths, frames = [], []
    for k, f in enumerate(textured_pair(PW, PH, 0, 40.0, -24.0)):
        paths.append(str(tmp_path / f"f{k}.png"))
        frames.append(np.uint8(np.round(255 * f.reshape(PH, PW))))
        Image.fromarray(frames[-1], "L").save(paths[-1])
    tr = str(tmp_path / "tracks.txt")
    _, out = _quiet_main(paths + ["--algo=TVL1", "--match", "200", "--global-motion", "translation", f"--save-tracks={tr}"])
    lines = out.splitlines()
    at = [k for k, l in enumerate(lines) if l.startswith(" - match: ")]
    assert len(at) == 1
    extra = lines[at[0]:at[0] + 4]
    assert extra[1].startswith(" - match motion (translation): ") and extra[2] == "saving tracks..."
    assert extra[3].startswith(" - global motion (translation): ")   # (of the solved flow, as without --match)
    f0, f1 = (f.astype(F64) / 255.0 for f in frames)
    p, d, st, idx, dist = MR.match_frames(f0, f1, PW, PH, 200, dtype=F64)
    rows = np.isfinite(p).all(axis=1)
    got = np.array([[float(v) for v in line.split()] for line in open(tr).read().splitlines()])
    assert got.shape == (rows.sum(), 6)
    same(got[:, :2], p[rows], "track points")
    same(got[:, 2:4], d[rows], "track displacements")
    same(got[:, 4].astype(np.uint8), st[rows], "track status")
    same(got[:, 5].astype(np.int32), dist[rows, 0], "track distances")
    m = R.fit(p, d, PW, PH, "translation", status=st)[0]
    nums = extra[1].split(": ")[1].split(" / ")[0].split()
    same(np.array([float(x) for x in nums]), m, "the printed matrix")
    assert abs(m[2] - 40.0) < 0.5 and abs(m[5] + 24.0) < 0.5
    assert extra[0] == f" - match: {int((st[rows] == 0).sum())} of {int(rows.sum())} corners matched (patch 15, 1 orientations, ratio 0.8)"
    with pytest.raises(SystemExit):
        _quiet_main(paths + ["--algo=TVL1", "--match", "50", "--lk", "50"])
