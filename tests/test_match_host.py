"""CPU checks of the feature-matching stage: the host tables, the C ABI's records, defaults and
argument errors (no device is touched), and the numpy restatement (tests/match_ref.py) that the GPU
tests hold the device to bit for bit.  The accuracy facts are checked here, on the restatement: the
device inherits them through bit equality."""
import ctypes

import numpy as np
import pytest

import match_ref as MR
import motion_ref as R
import sparse_ref as S

W, H = 96, 80
SHIFT = (40.5, -24.25)   # a quarter of the 160 x 128 frame: beyond the tracker, see test (a)

# The largest difference (px, either component, over the frame) between the field of the translation
# fitted to the matched tracks and the true shift, measured with this restatement on
# textured_pair(160, 128, seed, 40.5, -24.25) for the seeds 0 .. 3 (K = 200 corners, every default):
#   seed 0: 0.0833   seed 1: 0.2500   seed 2: 0.3452   seed 3: 0.2500
# (corners are whole pixels in both frames, so a match is right to half a pixel at best).  The test
# asserts twice the worst figure: the chain is deterministic, the margin covers a change of seed.
FIELD_ERR = 0.3452


# ------------------------------------------------------------------ the ABI

def test_abi_records_defaults_and_exports():
    from foto import _lib, match
    L = _lib.lib()
    for name in ("foto_describe_opts_default", "foto_match_opts_default", "foto_describe_dev", "foto_match_dev",
                 "foto_match_cross_dev"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    D, M = _lib.DescribeOpts, _lib.MatchOpts
    assert ctypes.sizeof(D) == 16 and (D.blur.offset, D.patch.offset, D.orientations.offset, D.reserved.offset) == (0, 4, 8, 12)
    assert ctypes.sizeof(M) == 24 and (M.max_disp.offset, M.max_dist.offset, M.ratio.offset, M.reserved.offset) == (0, 8, 12, 16)
    d = D(9, 9, 9, 9)
    assert L.foto_describe_opts_default(ctypes.byref(d)) == 0
    assert (d.blur, d.patch, d.orientations, d.reserved) == (2, 15, 1, 0)
    assert {k: getattr(d, k) for k in match.DESCRIBE_DEFAULTS} == match.DESCRIBE_DEFAULTS == MR.DESCRIBE_DEFAULTS
    m = M(9.0, 9, 9, (ctypes.c_int * 2)(9, 9))
    assert L.foto_match_opts_default(ctypes.byref(m)) == 0
    assert (m.max_disp, m.max_dist, m.ratio, list(m.reserved)) == (0.0, 64, 205, [0, 0])
    assert match.ratio_code(match.MATCH_DEFAULTS["ratio"]) == MR.MATCH_DEFAULTS["ratio"] == 205
    assert match.ratio_code(None) == 0 and match.ratio_code(1.0) == 256 and match.ratio_code(0.5) == 128
    assert (match.NONE, match.OUT, match.NONFINITE, match.NOT_MUTUAL, match.AMBIGUOUS) == (1, 2, 4, 8, 16)
    assert (MR.NONE, MR.OUT, MR.NONFINITE, MR.NOT_MUTUAL, MR.AMBIGUOUS) == (1, 2, 4, 8, 16)
    assert (match.OUT, match.NONFINITE, match.NOT_MUTUAL) == (_lib.FOTO_LK_OUT, _lib.FOTO_LK_NONFINITE, _lib.FOTO_LK_INCONSISTENT)
    assert (_lib.FOTO_MATCH_MAX_PATCH, _lib.FOTO_MATCH_MAX_ORIENT) == (MR.MAX_PATCH, MR.MAX_ORIENT) == (31, 32)


def test_argument_errors_without_gpu():
    """Every argument error that needs no device is FOTO_ERR_ARG with a message, found before any
    HIP call: the outputs (host memory here) stay as they were."""
    from foto import _lib
    L = _lib.lib()
    E = _lib.FOTO_ERR_ARG
    u8, f32, f64 = _lib.FOTO_U8, _lib.FOTO_F32, _lib.FOTO_F64
    assert L.foto_describe_opts_default(None) == E and L.foto_match_opts_default(None) == E
    buf = np.zeros(1 << 16)
    outs = np.full(256, 7.0)
    ptr, optr = ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(outs.ctypes.data)
    at = lambda a, off: ctypes.c_void_p(a.ctypes.data + off)
    tab, dirs = MR.pattern(2, 15, 0), MR.directions(2)
    tptr, dptr = tab.ctypes.data_as(ctypes.c_void_p), dirs.ctypes.data_as(ctypes.c_void_p)
    far = tab.copy()
    far[1, 200] = (11, 11, 0, 0)   # 242 > 225: outside the disc of 15
    image = lambda **kw: _lib.Image(**dict(dict(data=buf.ctypes.data, dtype=f64, stride_y=96, stride_x=1, divisor=1.0), **kw))

    def describe(frame=image(), w=96, h=80, pts=ptr, pd=f64, M=16, o=True, t=tptr, d=dptr, desc=optr, state=optr, b=optr,
                 **kw):
        oo = _lib.DescribeOpts(2, 15, 2, 0)
        for k, v in kw.items():
            setattr(oo, k, v)
        rc = L.foto_describe_dev(ctypes.byref(frame) if frame is not None else None, w, h, pts, pd, M,
                                 ctypes.byref(oo) if o else None, t, d, desc, state, b, None)
        assert rc >= 0 or L.foto_last_error()
        return rc

    for kw in (dict(frame=None), dict(pts=None), dict(t=None), dict(d=None), dict(desc=None), dict(state=None),
               dict(w=30), dict(h=30), dict(w=65536, h=32768), dict(frame=image(data=None)), dict(frame=image(dtype=7)),
               dict(frame=image(divisor=0.0)), dict(blur=-1), dict(blur=8), dict(patch=1), dict(patch=32),
               dict(orientations=0), dict(orientations=33), dict(t=far.ctypes.data_as(ctypes.c_void_p)), dict(M=0),
               dict(M=2 ** 31), dict(pd=u8), dict(pd=9), dict(pts=at(buf, 8)), dict(pts=at(buf, 4), pd=f32),
               dict(desc=at(outs, 4)), dict(b=at(outs, 2)), dict(d=at(buf, 4))):
        assert describe(**kw) == E, kw
    assert describe(patch=40, w=96, h=80) == E   # (w, h >= 2 patch + 1 holds for no allowed patch beyond 31 either)

    def match(d0=ptr, s0=ptr, p0=ptr, c0=f64, N0=16, d1=ptr, s1=ptr, p1=ptr, c1=f64, N1=16, o=True, idx=optr, dist=optr,
              status=optr, disp=optr, dd=f64, **kw):
        oo = _lib.MatchOpts(0.0, 64, 205, (ctypes.c_int * 2)(0, 0))
        for k, v in kw.items():
            setattr(oo, k, v)
        rc = L.foto_match_dev(d0, s0, p0, c0, N0, d1, s1, p1, c1, N1, ctypes.byref(oo) if o else None, idx, dist, status,
                              disp, dd, None)
        assert rc >= 0 or L.foto_last_error()
        return rc

    for kw in (dict(d0=None), dict(s0=None), dict(p0=None), dict(d1=None), dict(s1=None), dict(p1=None), dict(idx=None),
               dict(dist=None), dict(status=None), dict(N0=0), dict(N1=0), dict(N0=2 ** 31), dict(N1=2 ** 31),
               dict(max_disp=-1.0), dict(max_disp=float("nan")), dict(max_disp=float("inf")), dict(max_dist=-1),
               dict(max_dist=257), dict(ratio=-1), dict(ratio=257), dict(c0=u8), dict(c1=7), dict(dd=u8),
               dict(d0=at(buf, 8)), dict(d1=at(buf, 8)), dict(p0=at(buf, 8)), dict(p1=at(buf, 4), c1=f32),
               dict(idx=at(outs, 2)), dict(dist=at(outs, 2)), dict(disp=at(outs, 4), dd=f32)):
        assert match(**kw) == E, kw

    def cross(a=ptr, N0=16, b=ptr, N1=16, st=optr):
        return L.foto_match_cross_dev(a, N0, b, N1, st, None)

    for kw in (dict(a=None), dict(b=None), dict(st=None), dict(N0=0), dict(N1=0), dict(N0=2 ** 31), dict(N1=2 ** 31),
               dict(a=at(buf, 2)), dict(b=at(buf, 2))):
        assert cross(**kw) == E, kw
    assert (outs == 7.0).all() and L.foto_last_error()


def test_python_argument_errors():
    from foto import match
    for bad in (dict(orientations=0), dict(orientations=33), dict(patch=1), dict(patch=32)):
        with pytest.raises(ValueError):
            match.pattern(**bad)
    with pytest.raises(ValueError):
        match.directions(0)
    with pytest.raises(ValueError):
        match.ratio_code(1.5)
    with pytest.raises(ValueError):
        match._table(np.zeros((1, 256, 4), dtype=np.int16), 1, 15, 0)
    with pytest.raises(ValueError):
        match._table(np.zeros((2, 256, 4), dtype=np.int8), 1, 15, 0)
    assert match._table(None, 4, 7, 3).shape == (4, 256, 4)


# ------------------------------------------------------------------ the host tables

@pytest.mark.parametrize("patch", [2, 15, 31])
@pytest.mark.parametrize("K", [1, 4, 32])
def test_pattern_table(K, patch):
    from foto import match
    t = match.pattern(K, patch, 0)
    assert t.dtype == np.int8 and t.shape == (K, 256, 4) and t.flags.c_contiguous
    assert np.array_equal(t, match.pattern(K, patch, 0)) and np.array_equal(t, MR.pattern(K, patch, 0))
    assert not np.array_equal(t, match.pattern(K, patch, 1))
    assert np.array_equal(t[0], match.pattern(1, patch, 0)[0])   # bin 0 does not depend on K
    e = t.astype(np.int64).reshape(K, 512, 2)
    assert ((e ** 2).sum(axis=2) <= patch * patch).all()          # every end inside the disc
    if patch >= 15:   # the draw fills the disc: a spread near patch / 2.5 per coordinate, both signs
        assert 0.7 * patch / 2.5 < e[0].std() < 1.3 * patch / 2.5 and e[0].min() < 0 < e[0].max()
    if K == 4:        # the exact integer rotation (x, y) -> (-y, x), repeated
        for k in range(1, 4):
            assert np.array_equal(e[k, :, 0], -e[k - 1, :, 1]) and np.array_equal(e[k, :, 1], e[k - 1, :, 0])
    if K == 32:       # a rotated end is within a rounding of the rotated offset, and stays in the disc
        d = MR.directions(32)
        for k in (3, 8, 21):
            x = d[k, 0] * e[0, :, 0] - d[k, 1] * e[0, :, 1]
            y = d[k, 1] * e[0, :, 0] + d[k, 0] * e[0, :, 1]
            assert np.abs(e[k, :, 0] - x).max() <= 1.5 and np.abs(e[k, :, 1] - y).max() <= 1.5


def test_directions_table():
    from foto import match
    d = match.directions(4)
    assert d.dtype == np.float64 and np.array_equal(d, [[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])
    assert not np.signbit(d[d == 0]).any()
    for K in (1, 2, 3, 8, 32):
        d = match.directions(K)
        assert d.shape == (K, 2) and np.array_equal(d, MR.directions(K))
        assert np.abs(np.hypot(d[:, 0], d[:, 1]) - 1.0).max() < 1e-15
        if K % 4 == 0:
            assert np.array_equal(d[::K // 4], match.directions(4))
    assert np.array_equal(match.directions(2), [[1.0, 0.0], [-1.0, 0.0]])


# ------------------------------------------------------------------ accuracy (a): a shift beyond the tracker

def shift_pair(w, h, seed=0):
    from foto.synthetic import textured_pair
    return textured_pair(w, h, seed, SHIFT[0], SHIFT[1])


@pytest.mark.parametrize("w,h", [(160, 128), (128, 96)])
def test_matches_recover_a_shift_the_tracker_cannot_follow(w, h):
    """textured_pair(w, h, 0, 40.5, -24.25).  Pyramidal LK at its defaults (radius 7, 4 levels)
    starts from zero displacement and is lost: the share of clean statuses (forward-backward check
    included) is 0.013 at 160 x 128 and 0.050 at 128 x 96 -- asserted below one half.  The matches
    of the same corners, fed to the translation fit, recover the shift: field error 0.0833 px at
    160 x 128 (20 usable matches of 77 corners), 0.5000 px at 128 x 96 (9 of 40), against the bound
    2 FIELD_ERR = 0.6904."""
    f0, f1 = shift_pair(w, h)
    pts, n, _ = S.corners(f0, w, h, 200)
    st = S.track_checked(f0, f1, w, h, pts[:n].astype(np.float32), dtype=np.float32)[1]
    clean = float((st == 0).mean())
    p0, disp, status, idx, dist = MR.match_frames(f0, f1, w, h, 200)
    m, mask, info, rms = R.fit(p0, disp, w, h, "translation", status=status)
    u, v = R.field_uv(m, w, h)
    err = max(np.abs(u - SHIFT[0]).max(), np.abs(v - SHIFT[1]).max())
    print(f"{w} x {h}: {n} corners, LK clean share {clean:.3f}; matches usable {int((status == 0).sum())}, "
          f"fit info {[int(x) for x in info]}, field error {err:.4f} px")
    assert clean < 0.5
    assert info[3] == 0 and info[0] >= 4 and info[0] >= 0.4 * info[1]
    assert err <= 2 * FIELD_ERR
    # a usable match is a mutual, unambiguous nearest neighbour within the bound
    ok = status == 0
    assert (idx[ok] >= 0).all() and (dist[ok, 0] <= 64).all() and (dist[ok, 0] * 256 < 205 * dist[ok, 1]).all()
    assert np.isnan(disp[~ok & (idx < 0)]).all() and np.isfinite(disp[ok]).all()


# ------------------------------------------------------------------ accuracy (b): a quarter turn

def rotated_case(K, seed=0):
    from foto.synthetic import textured_pair
    f0 = textured_pair(W, H, seed, 0, 0)[0].reshape(H, W)
    f1 = np.ascontiguousarray(np.rot90(f0))     # f1[i][j] = f0[j][W - 1 - i]: (x, y) -> (y, W - 1 - x)
    co = dict(S.CORNER_DEFAULTS, margin=15)
    p0, n0, _ = S.corners(f0.ravel(), W, H, 200, **co)
    p1, n1, _ = S.corners(f1.ravel(), H, W, 200, **co)
    tab = MR.pattern(K, 15, 0)
    d0, s0, b0 = MR.describe(f0, p0, 2, 15, K, tab)
    d1, s1, b1 = MR.describe(f1, p1, 2, 15, K, tab)
    idx, dist, status, disp = MR.match_checked(d0, s0, p0, d1, s1, p1, dtype=np.float64)
    want = np.column_stack([p0[:, 1], (W - 1) - p0[:, 0]]) - p0
    return p0, n0, disp, status, want, (b0, b1, idx)


def test_orientation_bins_follow_a_quarter_turn():
    """np.rot90 of a 96 x 80 texture, K = 4, seeds 0 .. 2.  Measured with the restatement: every
    corner survives (share 1.000: 12, 15, 13 corners) and every surviving match lies on the rotated
    position (share 1.000) -- the K = 4 table is the exact integer rotation, so the descriptors of
    a corner and of its image are equal.  Asserted: survive >= 0.8, correct >= 0.9.  With K = 1 on
    the same pairs 0, 0 and 1 corners survive and the similarity fit finds no model."""
    rot = np.array([0.0, 1.0, 0.0, -1.0, 0.0, W - 1.0, 0.0, 0.0, 1.0])
    for seed in (0, 1, 2):
        p0, n0, disp, status, want, (b0, b1, idx) = rotated_case(4, seed)
        ok = status == 0
        correct = ok & (np.abs(disp - want).max(axis=1) == 0)
        survive, right = ok.sum() / n0, correct.sum() / max(ok.sum(), 1)
        print(f"seed {seed}: K = 4: {n0} corners, survive {survive:.3f}, correct {right:.3f}")
        assert n0 >= 8 and survive >= 0.8 and right >= 0.9
        assert ((b1[idx[ok]] - b0[ok]) % 4 == (b1[idx[ok][0]] - b0[ok][0]) % 4).all()   # the bins turn together
        m, mask, info, rms = R.fit(p0, disp, W, H, "similarity", status=status)
        assert info[3] == 0 and info[0] >= 0.9 * info[1] and np.abs(m - rot).max() < 1e-9
        p0, n0, disp, status, want, _ = rotated_case(1, seed)
        few = int((status == 0).sum())
        info1 = R.fit(p0, disp, W, H, "similarity", status=status)[2]
        print(f"seed {seed}: K = 1: {few} of {n0} corners survive, fit info {[int(x) for x in info1]}")
        assert few <= 0.2 * n0 and (info1[3] & R.NONE)


# ------------------------------------------------------------------ (c) tie rules and the pieces

def rand_desc(rng, n):
    return rng.integers(0, 2 ** 64, size=(n, 4), dtype=np.uint64)


def test_tie_rules():
    rng = np.random.default_rng(3)
    q = rand_desc(rng, 3)
    tr = rand_desc(rng, 6)
    tr[4] = tr[1] = q[0]                       # an exact duplicate of query 0, twice: the lower index wins
    tr[5] = q[1] ^ np.array([1, 0, 0, 0], dtype=np.uint64)
    z0, z1 = np.zeros(3, np.uint8), np.zeros(6, np.uint8)
    p0, p1 = np.zeros((3, 2)), np.arange(12.0).reshape(6, 2)
    for ratio in (1, 205, 256):
        idx, dist, st, disp = MR.match(q, z0, p0, tr, z1, p1, ratio=ratio)
        assert idx[0] == 1
        assert list(dist[0]) == [0, 0] and st[0] == MR.AMBIGUOUS   # a duplicate best: d2 = d1, ambiguous at any ratio > 0
        assert idx[1] == 5 and dist[1, 0] == 1 and (st[1] == 0) == (256 < ratio * dist[1, 1])
    idx, dist, st, disp = MR.match(q, z0, p0, tr, z1, p1, ratio=0)
    assert list(idx[:2]) == [1, 5] and st[0] == 0 and MR.same(disp[0], p1[1].astype(np.float32))
    # one lone candidate: d2 = 257, unambiguous below 205 / 256 of it, and the bound still holds
    z1[:] = 1
    z1[3] = 0
    idx, dist, st, disp = MR.match(q, z0, p0, tr, z1, p1, max_dist=256)
    assert (idx == 3).all() and (dist[:, 1] == 257).all() and (st == 0).all()
    idx, dist, st, disp = MR.match(q, z0, p0, tr, z1, p1, max_dist=64)
    assert (idx == -1).all() and (st == MR.NONE).all() and (dist[:, 0] > 64).all() and np.isnan(disp).all()
    # no candidate at all: both bits, (257, 257); an unusable query keeps its state
    z1[:] = 2
    z0[1] = MR.OUT
    idx, dist, st, disp = MR.match(q, z0, p0, tr, z1, p1)
    assert (idx == -1).all() and (dist == 257).all() and list(st) == [MR.NONE | MR.AMBIGUOUS, MR.OUT, MR.NONE | MR.AMBIGUOUS]


def test_gate_distance_and_cross():
    rng = np.random.default_rng(4)
    q, tr = rand_desc(rng, 5), rand_desc(rng, 9)
    tr[2], tr[7] = q[0], q[0]
    z0, z1 = np.zeros(5, np.uint8), np.zeros(9, np.uint8)
    p0 = np.tile([10.0, 10.0], (5, 1))
    p1 = np.column_stack([np.arange(9.0) * 3, np.full(9, 10.0)])   # x = 0, 3, .., 24
    assert MR.match(q, z0, p0, tr, z1, p1, ratio=0)[0][0] == 2
    # the gate is a box, closed at its edge: |6 - 10| <= 4 admits train 2; its duplicate at x = 21 is out
    idx, dist, st, _ = MR.match(q, z0, p0, tr, z1, p1, ratio=0, max_disp=4.0)
    assert idx[0] == 2 and dist[0, 1] > 0
    assert MR.match(q, z0, p0, tr, z1, p1, ratio=0, max_disp=3.999)[0][0] == -1
    idx, dist, st, _ = MR.match(q, z0, p0 + [12.0, 0.0], tr, z1, p1, ratio=0, max_disp=1.0)
    assert idx[0] == 7 and dist[0, 0] == 0      # x0 = 22: only train 7 (x = 21) is within 1
    p0n = p0.copy()
    p0n[3, 1] = np.nan                          # a NaN coordinate has no candidate under a gate
    idx, dist, st, _ = MR.match(q, z0, p0n, tr, z1, p1, ratio=0, max_dist=256, max_disp=100.0)
    assert idx[3] == -1 and st[3] == MR.NONE and (idx[[0, 1, 2, 4]] >= 0).all()
    assert MR.distances(q[:1], q[:1])[0, 0] == 0 and MR.distances(q[:1], ~q[:1])[0, 0] == 256
    # cross: kept where mutual, the bit where not, -1 untouched, an idx10 of -1 is not mutual
    idx01, idx10 = np.array([1, 0, -1, 2, 3], np.int32), np.array([1, 0, -1, 4], np.int32)
    st = np.array([0, 16, 1, 0, 0], np.uint8)
    assert list(MR.cross(idx01, idx10, st)) == [0, 16, 1, 8, 0] and list(st) == [0, 16, 1, 0, 0]
    assert list(MR.cross(np.array([0, 7], np.int32), np.array([0], np.int32), np.zeros(2, np.uint8))) == [0, 8]


def test_describe_pieces():
    rng = np.random.default_rng(5)
    F = rng.random((H, W))
    # the state rules: exactly patch from a border is inside, patch - 1 is not; .5 rounds up
    pts = np.array([[15.0, 15.0], [14.0, 15.0], [80.0, 64.0], [81.0, 64.0], [80.0, 65.0], [14.5, 15.0], [14.49, 15.0],
                    [80.49, 64.49], [80.5, 64.0], [np.nan, 20.0], [20.0, np.inf], [-np.inf, 20.0], [1e300, 20.0]])
    desc, state, bins = MR.describe(F, pts, 2, 15, 4)
    assert list(state) == [0, 2, 0, 2, 2, 0, 2, 0, 2, 6, 6, 6, 2]
    assert (desc[state != 0] == 0).all() and (bins[state != 0] == -1).all() and (bins[state == 0] >= 0).all()
    assert MR.same(desc[5], desc[0]) and MR.same(desc[7], desc[2])   # the keypoint pixel, not the point
    # the undivided box sum, and blur 0 = the frame
    B = MR.smoothed(F, 2)
    assert abs(B[40, 50] - F[38:43, 48:53].sum()) < 1e-12 and abs(B[0, 0] - F[:3, :3].sum()) < 1e-12
    assert MR.smoothed(F, 0) is F
    # bit t of word t / 64 is the comparison of test t
    tab = MR.pattern(1, 15, 0)
    d = MR.describe(F, pts[:1], 0, 15, 1, tab)[0][0]
    for t in (0, 63, 64, 200, 255):
        ax, ay, bx, by = (int(v) for v in tab[0, t])
        assert bool((int(d[t // 64]) >> (t % 64)) & 1) == bool(F[15 + ay, 15 + ax] < F[15 + by, 15 + bx])
    # the bin points at the bright side: a ramp rising along +x is bin 0, along +y bin 1 of 4
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for ramp, want in ((xx, 0), (yy, 1), (-xx, 2), (-yy, 3)):
        assert MR.describe(ramp + 100.0, [[40.0, 40.0]], 2, 15, 4)[2][0] == want
    # a NaN moment gives bin 0; a flat patch (both moments 0) too: ties go to the lower k
    G = F.copy()
    G[40, 40] = np.nan
    assert MR.describe(G, [[40.0, 40.0]], 2, 15, 32)[2][0] == 0
    assert MR.describe(np.ones((H, W)), [[40.0, 40.0]], 2, 15, 32)[2][0] == 0
    # the lane order: slot sums first, then the tree
    t = np.zeros((1, 200))
    t[0, 0], t[0, 64], t[0, 32] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert MR.lane_sum(t)[0] == 1.0
    t[0, 64], t[0, 32], t[0, 1], t[0, 33] = 0.0, 0.0, 2.0 ** -53, 2.0 ** -53
    assert MR.lane_sum(t)[0] == 1.0 + 2.0 ** -52
