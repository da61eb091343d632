"""Flow filtering on the device (include/foto.h, "flow filtering") against tests/filter_ref.py, the
numpy restatement of its definition.

Bar.  The result of a weighted median with integer weights is one of the samples and depends on no
order of summation, so every comparison here is on the BIT PATTERNS of the flow, and the masks and
the counts are equal: no tolerance is involved.  tests/test_filter_host.py pins the restatement
itself to scipy.ndimage.median_filter.

Sizes.  The kernel works on TW x TH = FOTO_MEDIAN_TILE_W x FOTO_MEDIAN_TILE_H tiles (32 x 8) staged
with an R-wide halo, one thread per pixel up to R = 2 and one wave per pixel above.  MULTI = (2 TW
+ 6) x (2 TH + 3) = 70 x 19 spans three tiles with a remainder in x and in y; TW + 2R + 1 by TH +
2R + 1 is one pixel wider than a tile with its halo; 2R x 2R truncates every window."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

from conftest import PKG, REPO  # noqa: F401

import chain_ref
import filter_ref as R
from foto import _lib, chain
from foto import device as D
from foto import filter as F

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
P, I = "planar", "interleaved"
COMBOS = [(d, l) for d in (F32, F64) for l in (P, I)]
TW, TH = _lib.FOTO_MEDIAN_TILE_W, _lib.FOTO_MEDIAN_TILE_H
MULTI = (2 * TW + 6, 2 * TH + 3)     # (w, h) = (70, 19): three tiles and a remainder along both axes


def dev(a):
    return D.DeviceArray.from_numpy(a)


def spiced_flow(K, h, w, layout, dtype, seed, special=True):
    """Positive and negative displacements with, sprinkled over u and v: NaN, +-inf, -0.0 beside +0.0,
    denormals, and runs of equal values (ties)."""
    f = R.random_flow(K, h, w, layout, dtype, seed)
    rng = np.random.default_rng(seed + 1000)
    uv = f[:, :2] if layout == P else f
    flat = uv.reshape(-1)
    n = flat.size
    if n >= 64:
        tie = rng.choice(n, n // 5, replace=False)
        flat[tie] = np.round(flat[tie] * 2) / 2                      # many equal values
    if special and n >= 16:
        tiny = np.finfo(dtype).smallest_subnormal
        vals = [np.nan, np.inf, -np.inf, -0.0, 0.0, tiny, -tiny, 3 * tiny]
        for k, i in enumerate(rng.choice(n - 1, max(8, n // 25), replace=False)):
            flat[i] = vals[k % len(vals)]
            if k % len(vals) == 3:
                flat[i + 1] = 0.0                                    # -0.0 beside +0.0
    uv[...] = flat.reshape(uv.shape)                                 # (the planar u, v planes reshape to a copy)
    return f


def guide_u8(h, w, seed, C=None):
    """A piecewise guide: two grey levels and noise, so range weights of every size occur."""
    rng = np.random.default_rng(seed)
    shape = (h, w) if C is None else (h, w, C)
    base = np.where(np.add.outer(np.arange(h), np.arange(w)) % 11 < 5, 60, 180)
    base = base if C is None else base[:, :, None]
    return np.clip(base + rng.integers(-40, 41, shape), 0, 255).astype(np.uint8)


def run_case(f, layout, *, guide=None, dguide=None, mask=None, dmask=None, divisor=None, out_dtype=None, out_layout=None,
             **kw):
    """median() on device arrays against the restatement: flow, mask and counts, bit for bit.
    ``dguide`` / ``dmask``: the device views to pass (default: uploads of ``guide`` / ``mask``)."""
    batched = f.ndim == 4
    if dguide is None and guide is not None:
        dguide = dev(guide)
    if dmask is None and mask is not None:
        dmask = dev(np.ascontiguousarray(mask))
    d = dev(f)
    got = F.median(d, in_layout=layout, guide=dguide, mask=dmask, dtype=None if out_dtype is None else np.dtype(out_dtype).name,
                   layout=out_layout, **kw)
    out, valid, table = (x.to_numpy() for x in got)
    rkw = dict(kw)
    rkw["rng"] = rkw.pop("range", None)
    want = R.median(f if batched else f[None], layout, guide=guide, divisor=divisor, mask=mask, out_dtype=out_dtype,
                    out_layout=out_layout, **rkw)
    want = want if batched else tuple(x[0] for x in want)
    R.same_bits(out, want[0])
    R.same_bits(valid, want[1])
    R.same_bits(table, want[2])
    h, w = valid.shape[-2:]
    assert np.all(table[..., :3].sum(axis=-1) == w * h) and np.all(table[..., 3] == 0)
    R.same_bits(d.to_numpy(), f)                                     # the input is read only
    return out, valid, table


# ------------------------------------------------------------------ 1. every radius on the multi-tile frame

@pytest.mark.parametrize("radius", [1, 2, 3, 4, 5, 6, 7])
def test_every_radius_on_the_multi_tile_frame(radius):
    w, h = MULTI
    f = spiced_flow(3, h, w, I, F32, seed=radius)
    sp, rg = F.tables(radius, sigma_s=0.6 * radius + 0.5, sigma_r=0.15)
    mask = np.random.default_rng(50 + radius).random((h, w)) < 0.85
    out, valid, table = run_case(f, I, guide=guide_u8(h, w, radius), mask=mask.astype(np.uint8), radius=radius,
                                 spatial=sp, range=rg)
    assert out.shape == (3, h, w, 2) and np.all(table[:, 1] > 0)    # some rejected pixels are filled


# ------------------------------------------------------------------ 2. small and awkward frames

def _small_sizes():
    s = [(1, 1, 1), (1, 1, 7), (2, 2, 1), (2, 2, 4), (1, 9, 2), (9, 1, 2), (1, 9, 5), (9, 1, 5)]
    s += [(2 * r, 2 * r, r) for r in (1, 2, 3, 7)]                   # every window is truncated
    s += [(TW + 2 * r + 1, TH + 2 * r + 1, r) for r in (2, 7)]       # one pixel wider than a tile with its halo
    return s


@pytest.mark.parametrize("w,h,radius", _small_sizes())
def test_small_frames(w, h, radius):
    f = spiced_flow(1, h, w, P, F64, seed=w + 7 * h)[0]
    guide = np.random.default_rng(w).random((h, w)).astype(F32)
    sp, rg = F.tables(radius, sigma_s=2.0, sigma_r=0.3)
    out, valid, table = run_case(f, P, guide=guide, radius=radius, spatial=sp, range=rg)
    assert out.shape == (3, h, w) and valid.shape == (h, w) and table.shape == (4,)
    run_case(f, P, radius=radius)                                    # all ones: the plain (lower) median


# ------------------------------------------------------------------ 3. dtypes and layouts, in and out

@pytest.mark.parametrize("di,li", COMBOS)
@pytest.mark.parametrize("do,lo", COMBOS)
def test_every_format_in_and_out(di, li, do, lo):
    w, h, K = TW + 5, TH + 3, 3
    radius = 2 if di == F32 else 3                                    # both selection paths
    f = spiced_flow(K, h, w, li, di, seed=11)
    sp, rg = F.tables(radius, sigma_s=1.5, sigma_r=0.2)
    out, _, _ = run_case(f, li, guide=guide_u8(h, w, 3), radius=radius, spatial=sp, range=rg, out_dtype=do, out_layout=lo)
    assert out.dtype == do
    if lo == P and li == P:                                          # m passes through
        R.same_bits(out[:, 2], f[:, 2].astype(do))
    if lo == P and li == I:
        assert not np.any(out[:, 2]) and not np.any(np.signbit(out[:, 2]))


# ------------------------------------------------------------------ 4. guides and masks

@pytest.mark.parametrize("radius", [2, 3])
@pytest.mark.parametrize("kind", ["u8", "f32", "f64", "row-padded", "one channel of hwc", "colour", "five channels",
                                  "strided mask", "float mask", "no guide", "no mask", "neither"])
def test_guides_and_masks(kind, radius):
    w, h = TW + 8, TH + 3
    f = spiced_flow(2, h, w, P, F32, seed=21)
    rng = np.random.default_rng(22)
    sp, rg = F.tables(radius, sigma_s=1.2, sigma_r=0.1)
    mask = (rng.random((h, w)) < 0.8).astype(np.uint8)
    g8 = guide_u8(h, w, 23)
    kw = dict(radius=radius, spatial=sp, range=rg, rounds=2)
    if kind == "u8":
        run_case(f, P, guide=g8, mask=mask, **kw)
    elif kind == "f32":
        run_case(f, P, guide=(g8 / 255).astype(F32), mask=mask, **kw)
    elif kind == "f64":                                               # with NaN and inf in the guide: the last range entry
        g = g8 / 255.0
        g[2, 3], g[5, 20], g[6, 21] = np.nan, np.inf, -np.inf
        run_case(f, P, guide=g, mask=mask, **kw)
    elif kind == "row-padded":
        wide = guide_u8(h, w + 9, 24)
        run_case(f, P, guide=wide[:, 4:4 + w], dguide=dev(wide)[:, 4:4 + w], mask=mask, **kw)
    elif kind == "one channel of hwc":
        hwc = guide_u8(h, w, 25, C=3)
        run_case(f, P, guide=hwc[:, :, 1], dguide=dev(hwc)[:, :, 1], mask=mask, **kw)
    elif kind == "colour":                                            # the maximum over the channels
        run_case(f, P, guide=guide_u8(h, w, 26, C=3), mask=mask, **kw)
    elif kind == "five channels":                                     # more than are staged on chip
        run_case(f, P, guide=rng.random((h, w, 5)), mask=mask, **kw)
    elif kind == "strided mask":
        wide = (rng.random((h, 2 * w)) < 0.8).astype(np.uint8)
        run_case(f, P, guide=g8, mask=wide[:, ::2], dmask=dev(wide)[:, ::2], **kw)
    elif kind == "float mask":                                        # non-zero = usable: NaN and -2.5 are
        fm = mask.astype(F64) * -2.5
        fm[1, 1] = np.nan
        run_case(f, P, guide=g8, mask=fm, **kw)
    elif kind == "no guide":
        run_case(f, P, mask=mask, **kw)
    elif kind == "no mask":
        run_case(f, P, guide=g8, **kw)
    else:
        run_case(f, P, **kw)


def test_guide_divisor_is_applied():
    w, h = 20, 9
    f = spiced_flow(1, h, w, I, F64, seed=31)[0]
    g = guide_u8(h, w, 32)
    sp, rg = F.tables(2, sigma_r=0.05)
    a, _, _ = run_case(f, I, guide=g, radius=2, spatial=sp, range=rg)                       # / 255
    im = D.as_image(dev(g), divisor=51.0)
    b = F.median(dev(f), in_layout=I, guide=im, radius=2, spatial=sp, range=rg)[0].to_numpy()
    R.same_bits(b, R.median(f[None], I, guide=g, divisor=51.0, radius=2, spatial=sp, rng=rg)[0][0])
    assert not np.array_equal(R.bits(a), R.bits(b))


# ------------------------------------------------------------------ 5. values

@pytest.mark.parametrize("radius,w,h", [(1, 2, 2), (2, 2, 2), (3, 4, 4), (7, 4, 4)])
def test_even_count_hits_half_the_total_exactly(radius, w, h):
    """Every window is the whole frame: n = w h candidates of weight 1, three distinct values.  u
    holds n / 2 of the smallest, so 2 cum == T exactly there and the LOWER median is that value; v
    holds n / 2 - 1 of it, so the median is the middle value."""
    n = w * h
    a, b, c = -1.5, 0.25, 2.0
    rng = np.random.default_rng(radius)
    u = rng.permutation([a] * (n // 2) + [b] * (n // 4) + [c] * (n - n // 2 - n // 4))
    v = rng.permutation([a] * (n // 2 - 1) + [b] * (n // 4 + 1) + [c] * (n - n // 2 - n // 4))
    f = np.stack([u.reshape(h, w), v.reshape(h, w), np.zeros((h, w))]).astype(F32)
    out, valid, table = run_case(f, P, radius=radius)
    assert np.all(out[0] == a) and np.all(out[1] == b) and valid.all() and table[0] == n


@pytest.mark.parametrize("radius,w,h", [(1, 2, 2), (3, 4, 4)])
def test_negative_zero_sorts_below_positive_zero(radius, w, h):
    n = w * h
    u = np.array([-0.0] * (n // 2) + [0.0] * (n // 2))               # the lower median is -0.0
    v = np.array([-0.0] * (n // 2 - 1) + [0.0] * (n // 2 + 1))       # ... +0.0
    f = np.stack([u.reshape(h, w), v.reshape(h, w), np.zeros((h, w))])
    out, _, _ = run_case(f, P, radius=radius)
    assert np.all(np.signbit(out[0])) and not np.any(np.signbit(out[1])) and not np.any(out[:2])


def test_denormals_and_huge_values_are_ordered():
    w, h = 12, 10
    rng = np.random.default_rng(41)
    tiny = 5e-324
    pool = np.array([tiny, -tiny, 3 * tiny, -7 * tiny, 1e-310, -1e-310, 1e308, -1e308, 0.0, -0.0, 1.0, -1.0])
    f = rng.choice(pool, (2, 3, h, w))
    for radius in (2, 4):
        run_case(f, P, radius=radius)


def test_non_finite_samples_are_never_candidates():
    w, h = TW + 3, TH + 2
    f = R.random_flow(1, h, w, P, F32, seed=43)[0]
    f[0, 3:5, 10:14] = np.nan                                         # two rows: every hole pixel has a usable neighbour at R = 1
    f[1, 8, 2] = np.inf
    f[0, 0, 0] = -np.inf
    for radius in (1, 3):
        out, valid, table = run_case(f, P, radius=radius)
        assert np.isfinite(out[:2]).all() and valid.all()              # every hole has usable neighbours: replaced
        assert table[0] == w * h - 10 and table[1] == 10 and table[2] == 0


# ------------------------------------------------------------------ 6. 64-bit weight sums

def test_largest_tables_need_64_bit_sums():
    """spatial = range = 65535 at R = 7: a full window sums 225 * 65535^2 = 9.66e11 > 2^32, and half of
    it is passed inside the window: a 32-bit partial sum picks another sample."""
    radius, w, h = 7, 21, 18
    f = R.random_flow(1, h, w, P, F32, seed=47)
    sp = np.full((15, 15), 65535, np.uint16)
    rg = np.full(4, 65535, np.uint16)
    out, valid, table = run_case(f, P, guide=guide_u8(h, w, 48), radius=radius, spatial=sp, range=rg)
    assert 225 * 65535 ** 2 > 2 ** 32 and h - 2 * radius >= 1 and w - 2 * radius >= 1   # full windows exist
    plain = R.median(f, P, radius=radius)[0]                            # equal weights: the plain lower median
    R.same_bits(out, plain)


# ------------------------------------------------------------------ 7. holes

@pytest.mark.parametrize("radius", [1, 3])
@pytest.mark.parametrize("rounds", [1, 2, 3])
def test_a_masked_square_fills_from_its_rim(radius, rounds):
    side = 2 * radius + 3
    w, h = TW + 6, max(TH + 4, side + 6)
    f = spiced_flow(2, h, w, P, F64, seed=51, special=False)
    mask = np.ones((h, w), np.uint8)
    y0, x0 = 3, TW - 4                                               # the hole straddles a tile seam
    mask[y0:y0 + side, x0:x0 + side] = 0
    sp, rg = F.tables(radius, sigma_s=1.0 * radius)
    out, valid, table = run_case(f, P, mask=mask, radius=radius, rounds=rounds, fill_only=True, spatial=sp, range=rg)
    keep = mask == 1
    R.same_bits(out[:, :2][:, :, keep], f[:, :2][:, :, keep])        # usable pixels keep their input bits
    assert np.all(table[:, 0] == w * h - side * side)
    assert np.all(table[:, 0] + table[:, 1] + table[:, 2] == w * h)
    # a round reaches `radius` pixels into the hole from every side
    assert np.all(table[:, 2] == max(0, side - 2 * radius * rounds) ** 2), table


@pytest.mark.parametrize("radius", [2, 4])
def test_a_fully_masked_frame_stays_as_it_is(radius):
    w, h = TW + 1, TH + 1
    f = spiced_flow(2, h, w, I, F32, seed=53)
    out, valid, table = run_case(f, I, mask=np.zeros((h, w), np.uint8), radius=radius, rounds=3)
    R.same_bits(out, f)
    assert not valid.any() and np.array_equal(table, [[0, 0, w * h, 0]] * 2)


def test_fill_on_the_output_of_consistency():
    w, h = 64, 48
    fwd, bwd = chain_ref.cons_case(1, h, w, seed=17, dtype=F32)
    dfwd, dbwd = dev(fwd[0]), dev(bwd[0])
    valid, ctable = chain.consistency(dfwd, dbwd)                     # device arrays all the way
    guide = guide_u8(h, w, 55)
    sp, rg = F.tables(2, sigma_s=2.0, sigma_r=0.2)
    out, v2, table = F.fill(dfwd, valid, guide=dev(guide), radius=2, rounds=3, spatial=sp, range=rg)
    vm = valid.to_numpy()
    want = R.median(fwd, P, guide=guide, mask=vm, radius=2, rounds=3, fill_only=True, spatial=sp, rng=rg)
    R.same_bits(out.to_numpy(), want[0][0])
    R.same_bits(v2.to_numpy(), want[1][0])
    R.same_bits(table.to_numpy(), want[2][0])
    t, ct = table.to_numpy(), ctable.to_numpy()
    assert t[0] == ct[0] == vm.sum() and 0 < t[1] and t[:3].sum() == w * h
    assert np.isfinite(out.to_numpy()[:2][:, v2.to_numpy() == 1]).all()
    assert F.fill(dfwd, valid)[2].to_numpy()[0] == ct[0]              # the defaults: 8 rounds, radius 2, all ones


def test_numpy_arrays_are_uploaded_and_downloaded():
    w, h = 20, 11
    f = spiced_flow(2, h, w, I, F32, seed=57)
    guide, mask = guide_u8(h, w, 58, C=3), np.random.default_rng(59).random((h, w)) < 0.7
    sp, rg = F.tables(3, 2.0, 0.1)
    got = F.median(f, in_layout=I, guide=guide, mask=mask, radius=3, spatial=sp, range=rg, dtype="float64", layout=P)
    assert all(isinstance(x, np.ndarray) for x in got)
    want = R.median(f, I, guide=guide, mask=mask, radius=3, spatial=sp, rng=rg, out_dtype=F64, out_layout=P)
    for a, b in zip(got, want):
        R.same_bits(a, b)


# ------------------------------------------------------------------ 8. calls and arguments

def _raw_call(fl, w, h, o, out, valid=None, table=None, dtype=_lib.FOTO_F32, layout=0, stream=None):
    return _lib.lib().foto_flow_median_dev(ctypes.byref(fl), None, 0, 0, None, w, h, ctypes.byref(o), ctypes.c_void_p(out),
                                           dtype, layout, ctypes.c_void_p(valid), ctypes.c_void_p(table),
                                           ctypes.c_void_p(stream))


def test_the_same_call_twice_gives_the_same_bits():
    w, h = MULTI
    f = spiced_flow(3, h, w, P, F32, seed=61)
    d, g = dev(f), dev(guide_u8(h, w, 62))
    sp, rg = F.tables(5, 2.5, 0.1)
    runs = [tuple(x.to_numpy() for x in F.median(d, guide=g, radius=5, rounds=3, spatial=sp, range=rg)) for _ in range(2)]
    for a, b in zip(*runs):
        R.same_bits(a, b)
    assert runs[0][2][:, :3].sum() == 3 * w * h


def test_null_outputs_and_argument_errors_leave_the_outputs_untouched():
    L = _lib.lib()
    w, h, K = TW + 5, TH + 3, 2
    f = R.random_flow(K, h, w, P, F32, seed=63)
    d = dev(f)
    fl = _lib.Flow()
    fl.data, fl.dtype, fl.layout, fl.records = d.ptr, _lib.FOTO_F32, 0, K
    o = F.median_opts(3)
    want = R.median(f, P, radius=3)
    out = dev(np.full((K, 3, h, w), 7.25, F32))
    # valid_out and table are optional
    assert _raw_call(fl, w, h, o, out.ptr) == 0, L.foto_last_error()
    R.same_bits(out.to_numpy(), want[0])
    valid, table = dev(np.full((K, h, w), 9, np.uint8)), dev(np.full((K, 4), 7.25))
    out = dev(np.full((K, 3, h, w), 7.25, F32))
    assert _raw_call(fl, w, h, o, out.ptr, valid.ptr) == 0
    R.same_bits(valid.to_numpy(), want[1])
    out, valid = dev(np.full((K, 3, h, w), 7.25, F32)), dev(np.full((K, h, w), 9, np.uint8))
    # an output over the input, over another output, a host pointer, a misaligned out: nothing is written
    ARG = _lib.FOTO_ERR_ARG
    assert _raw_call(fl, w, h, o, d.ptr, valid.ptr, table.ptr) == ARG and L.foto_last_error()
    assert _raw_call(fl, w, h, o, d.ptr + 4 * (K * 3 * h * w - 1), valid.ptr, table.ptr) == ARG    # the last element
    assert _raw_call(fl, w, h, o, out.ptr, d.ptr, table.ptr) == ARG
    assert _raw_call(fl, w, h, o, out.ptr, valid.ptr, out.ptr) == ARG                      # the table over out
    assert _raw_call(fl, w, h, o, out.ptr, out.ptr + 16, table.ptr) == ARG
    assert _raw_call(fl, w, h, o, out.ptr + 2, valid.ptr, table.ptr) == ARG
    host = np.zeros((K, 3, h, w), F32)
    assert _raw_call(fl, w, h, o, host.ctypes.data, valid.ptr, table.ptr) == ARG
    hostfl = _lib.Flow()
    hostfl.data, hostfl.dtype, hostfl.layout, hostfl.records = f.ctypes.data, _lib.FOTO_F32, 0, K
    assert _raw_call(hostfl, w, h, o, out.ptr, valid.ptr, table.ptr) == ARG
    bad = F.median_opts(3)
    bad.radius = 8
    assert _raw_call(fl, w, h, bad, out.ptr, valid.ptr, table.ptr) == ARG
    assert np.all(out.to_numpy() == 7.25) and np.all(valid.to_numpy() == 9) and np.all(table.to_numpy() == 7.25)
    R.same_bits(d.to_numpy(), f)
    assert not host.any()
    with pytest.raises(_lib.FotoError):
        F.median(d, out=d)
    # and the entry still works
    assert _raw_call(fl, w, h, o, out.ptr, valid.ptr, table.ptr) == 0
    R.same_bits(out.to_numpy(), want[0])
    R.same_bits(table.to_numpy(), want[2])


def test_caller_stream_orders_the_call():
    """The inputs are produced by foto_dev_memcpy on the null stream; the call runs for a non-blocking
    caller stream, several rounds through the scratch; the results are read after synchronising that
    stream only."""
    w, h = MULTI
    _lib.lib()
    hip = ctypes.CDLL(D.mapped_hip_runtimes()[0])   # the runtime libfoto is bound to
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(stream), 1) == 0   # hipStreamNonBlocking
    try:
        f = spiced_flow(2, h, w, I, F64, seed=71)
        guide = guide_u8(h, w, 72, C=3)
        mask = (np.random.default_rng(73).random((h, w)) < 0.6).astype(np.uint8)
        sp, rg = F.tables(4, 2.0, 0.1)
        kw = dict(radius=4, rounds=3, spatial=sp)
        d, dg, dm, ds = dev(f), dev(guide), dev(mask), dev(f[:1, :5, :7])
        got = F.median(d, in_layout=I, guide=dg, mask=dm, range=rg, stream=stream.value, **kw)
        small = F.median(ds, in_layout=I, radius=2, stream=stream.value)   # then a call of another shape
        assert hip.hipStreamSynchronize(stream) == 0
        want = R.median(f, I, guide=guide, mask=mask, rng=rg, **kw)
        for a, b in zip(got, want):
            R.same_bits(a.to_numpy(), b)
        R.same_bits(small[0].to_numpy(), R.median(np.ascontiguousarray(f[:1, :5, :7]), I, radius=2)[0])
    finally:
        assert hip.hipStreamDestroy(stream) == 0


# ------------------------------------------------------------------ 9. the command line

def _pair_pngs(tmp_path, w, h):
    from PIL import Image
    from foto.synthetic import textured_pair
    paths = []
    for k, fr in enumerate(textured_pair(w, h, seed=3, dx=1.5, dy=0.5)):
        paths.append(str(tmp_path / f"f{k}.png"))
        Image.fromarray(np.round(fr.reshape(h, w) * 255).astype(np.uint8), "L").save(paths[-1])
    return paths


def test_cli_median_writes_the_filtered_flo(tmp_path):
    """main.py --algo=GN --median 2 writes the .flo that foto.filter.median gives on the unfiltered
    run's .flo with main.py's guide and tables.  (The filter runs on the float64 flow before the
    float32 .flo is written; rounding is monotone in the key, so the median commutes with it.)"""
    import main as M
    import utils as U
    w, h = 40, 30
    paths = _pair_pngs(tmp_path, w, h)
    plain, filt = str(tmp_path / "plain.flo"), str(tmp_path / "median.flo")
    outs = []
    for extra in ([f"--out={plain}"], [f"--out={filt}", "--median", "2"]):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            M.main(paths + ["--algo=GN"] + extra)
        outs.append(buf.getvalue())
    assert "median filter" not in outs[0] and " - median filter: radius 2, 1 round(s), guided by f0" in outs[1]
    assert [l for l in outs[1].splitlines() if "median filter" not in l and "time" not in l and "IE" not in l] == \
           [l for l in outs[0].splitlines() if "time" not in l and "IE" not in l]
    _, _, u0, v0 = U.openFlo(plain)
    _, _, u1, v1 = U.openFlo(filt)
    flo = np.ascontiguousarray(np.stack([u0, v0], axis=-1).reshape(h, w, 2))
    guide = U.openGrayscaleImage(paths[0])[0].reshape(h, w)
    sp, rg = M.median_tables(2)
    want, _, _ = F.median(flo, in_layout=I, guide=guide, radius=2, spatial=sp, range=rg)
    R.same_bits(np.stack([u1, v1], axis=-1).reshape(h, w, 2), want)
    assert not np.array_equal(u0, u1)                                 # the filter did something
    R.same_bits(want, R.median(flo[None], I, guide=guide, radius=2, spatial=sp, rng=rg)[0][0])


def test_cli_fill_occluded_accounts_for_every_rejected_pixel(tmp_path):
    """--fill-occluded: the pixels the cross-check rejects are either filled or counted as unfilled,
    the class counts are those of the solved flow, and the written flow is finite where filled."""
    import re
    import main as M
    import utils as U
    w, h = 40, 30
    paths = _pair_pngs(tmp_path, w, h)
    flo = str(tmp_path / "filled.flo")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        M.main(paths + ["--algo=GN", "--median", "2", "--fill-occluded", f"--save-consistency={tmp_path / 'c.png'}",
                        f"--out={flo}"])
    out = buf.getvalue()
    filled, unfilled = (int(x) for x in re.search(r"occluded pixels filled / unfilled: (\d+) / (\d+)", out).groups())
    classes = [int(x) for x in re.search(r"not finite: (\d+) / (\d+) / (\d+) / (\d+)", out).groups()]
    assert sum(classes) == w * h and filled + unfilled == w * h - classes[0]
    _, _, u, v = U.openFlo(flo)
    assert np.count_nonzero(~(np.isfinite(u) & np.isfinite(v))) <= unfilled
