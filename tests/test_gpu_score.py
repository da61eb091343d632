"""Scoring on the device (include/foto.h, "scoring") against tests/score_ref.py, the numpy
restatement of its definitions.

Bars.  Counts, EE max, every EE A(p) and the EE map are bit-identical, for float64 and for float32
input: the argument of the square root is computed in the same operations and sqrt is correctly
rounded.  Threshold fractions are exact.  Means, standard deviations, IE, NE, every AE value, AE
A(p) and the AE map are within 1e-13 relative (the bar of flow_errors parity in test_dropin.py): the
numpy and the device acos differ in the last places only, the sums in order only.

Inputs are gt = rng.normal(0, 2, (2, h, w)) and flow = gt + rng.normal(0, 0.7, (R, 2, h, w)) from
np.random.default_rng(seed) at the sizes of SHAPES.  Exact fractions and AE order statistics need the
inputs to stay clear of the thresholds and of each other; `precondition` asserts that on the numpy
values, with a margin of 1e-9 relative (four orders above the bar), and fails the test otherwise."""
import contextlib
import ctypes
import io
import re

import numpy as np
import pytest

from conftest import PKG  # noqa: F401  (puts the package on sys.path)

import score_ref
from foto import _lib, evaluate
from foto import device as D

pytestmark = pytest.mark.gpu

# w, h, records, seed
SHAPES = [(1, 1, 1, 4),      # the smallest input
          (37, 29, 3, 1),    # five 256-pixel blocks, odd row length, several records
          (130, 18, 2, 2),   # a second odd-length shape
          (257, 65, 1, 3)]   # many blocks: the cross-block hand-off and the global histogram both run
IDS = [f"{w}x{h}x{r}" for w, h, r, _ in SHAPES]
EXACT = [0, 1, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 17, 18, 19, 20, 25, 26, 27, 28, 29, 30, 31]
CLOSE = [2, 3, 14, 15, 16, 21, 22, 23, 24]
RTOL = 1e-13

_inputs = {}


def inputs(w, h, R, seed):
    """(gt (2, h, w), flow (R, 2, h, w)) float64, made once per shape and never changed."""
    key = (w, h, R, seed)
    if key not in _inputs:
        rng = np.random.default_rng(seed)
        gt = rng.normal(0, 2, (2, h, w))
        flow = gt + rng.normal(0, 0.7, (R, 2, h, w))
        gt.setflags(write=False)
        flow.setflags(write=False)
        _inputs[key] = (gt, flow)
    return _inputs[key]


def as_flow(uv, layout, dtype):
    """(R, 2, h, w) -> a planar (R, 3, h, w) (m = 0) or interleaved (R, h, w, 2) array of dtype."""
    uv = np.asarray(uv)
    if layout == "planar":
        return np.ascontiguousarray(np.concatenate([uv, np.zeros_like(uv[:, :1])], axis=1).astype(dtype))
    return np.ascontiguousarray(np.moveaxis(uv, 1, -1).astype(dtype))


def flo_payload(gt):
    """(2, h, w) -> what utils.openFlo reads: float32 (h, w, 2)."""
    return np.ascontiguousarray(np.moveaxis(np.asarray(gt), 0, -1).astype(np.float32))


def precondition(table, maps, ee_thr=score_ref.EE_THR, ae_thr=score_ref.AE_THR, pct=score_ref.PCT, margin=1e-9):
    """On the numpy values: no AE is NaN where the pixel is valid, no EE or AE within `margin`
    relative of a threshold, AE order statistics at the percentiles `margin` apart from their
    neighbours."""
    for r in range(table.shape[0]):
        ee, ae = maps[r, 0].ravel(), maps[r, 1].ravel()
        valid = ~np.isnan(ee)
        assert not np.any(np.isnan(ae[valid])), "an AE is NaN"
        for x, thr in ((ee[valid], ee_thr), (ae[valid], ae_thr)):
            for t in thr:
                assert not np.any(np.abs(x - t) <= margin * t), f"a value within {margin} of the threshold {t}"
        s = np.sort(ae[valid])
        for p in pct:
            if s.size < 2:
                continue
            k = score_ref.rank(p, s.size) - 1
            for j in (k - 1, k + 1):
                if 0 <= j < s.size:
                    assert abs(s[j] - s[k]) >= margin * s[k], f"AE order statistics at p = {p} closer than {margin}"


def compare(table, ref, maps=None, ref_maps=None):
    table, ref = np.asarray(table), np.asarray(ref)
    assert table.shape == ref.shape
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(table[:, CLOSE] - ref[:, CLOSE]) / np.abs(ref[:, CLOSE])
    print("max relative difference of the 1e-13 columns:", np.max(rel[np.isfinite(rel)], initial=0.0))
    np.testing.assert_array_equal(table[:, EXACT], ref[:, EXACT])
    np.testing.assert_allclose(table[:, CLOSE], ref[:, CLOSE], rtol=RTOL, atol=0, equal_nan=True)
    if maps is not None:
        maps = np.asarray(maps).reshape(ref_maps.shape)
        want = ref_maps.astype(maps.dtype)
        np.testing.assert_array_equal(maps[:, 0], want[:, 0])
        if maps.dtype == np.float64:
            np.testing.assert_allclose(maps[:, 1], want[:, 1], rtol=RTOL, atol=0, equal_nan=True)
        else:   # (a float32 map: the rounding of a value that differs in its last float64 places)
            np.testing.assert_allclose(maps[:, 1], want[:, 1], rtol=2.0 ** -23, atol=0, equal_nan=True)


def dev(a):
    return D.DeviceArray.from_numpy(a)


# ------------------------------------------------------------------ dtypes and layouts

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_flow_dtypes_and_layouts(shape, dtype, layout):
    """{F32, F64} x {planar, interleaved} for the flow; the ground truth as a 1-record .flo payload
    and as per-record planar float64; maps in float64."""
    w, h, R, seed = shape
    gt, flow = inputs(*shape)
    fl = as_flow(flow, layout, dtype)
    for g, g_layout in ((flo_payload(gt), "flo"), (as_flow(np.repeat(gt[None], R, 0), "planar", np.float64), "planar")):
        ref, ref_maps = score_ref.score_flow(fl, g, layout, _GT[g_layout])
        precondition(ref, ref_maps)
        s = evaluate.score_flow(dev(fl), dev(g), layout=layout, gt_layout=g_layout, maps="float64")
        compare(s.host(), ref, s.maps.to_numpy(), ref_maps)
    assert s.ee_mean.shape == (R,) and s.ee_R.shape == (R, 3) and s.ae_A.shape == (R, 3)
    np.testing.assert_array_equal(s.ae_degrees()["A"], np.rad2deg(s.host()[:, 21:24]))


_GT = {"flo": "interleaved", "planar": "planar"}


def test_single_record_without_record_axis_and_float32_maps():
    w, h, R, seed = SHAPES[1]
    gt, flow = inputs(*SHAPES[1])
    fl = as_flow(flow, "planar", np.float32)[0]   # (3, h, w)
    ref, ref_maps = score_ref.score_flow(fl, flo_payload(gt))
    s = evaluate.score_flow(dev(fl), dev(flo_payload(gt)), maps="float32")
    compare(s.host(), ref, s.maps.to_numpy(), ref_maps)
    assert s.maps.shape == (2, h, w) and np.ndim(s.ee_mean) == 0 and s.ee_A.shape == (3,)
    assert s.n == w * h


# ------------------------------------------------------------------ mask, unknown flow, NaN

@pytest.mark.parametrize("shape", SHAPES[1:], ids=IDS[1:])
def test_strided_uint8_mask(shape):
    w, h, R, seed = shape
    gt, flow = inputs(*shape)
    rng = np.random.default_rng(100 + seed)
    big = (rng.random((h, 2 * w + 3)) < 0.6).astype(np.uint8) * rng.integers(1, 255, (h, 2 * w + 3)).astype(np.uint8)
    dmask = dev(big)[:, 1:2 * w + 1:2]   # every other column of a padded row
    mask = big[:, 1:2 * w + 1:2]
    fl = as_flow(flow, "interleaved", np.float32)
    ref, ref_maps = score_ref.score_flow(fl, flo_payload(gt), "interleaved", mask=mask)
    precondition(ref, ref_maps)
    assert 0 < ref[0, 0] < w * h
    s = evaluate.score_flow(dev(fl), dev(flo_payload(gt)), layout="interleaved", mask=dmask, maps="float64")
    compare(s.host(), ref, s.maps.to_numpy(), ref_maps)


@pytest.mark.parametrize("shape", SHAPES[1:], ids=IDS[1:])
def test_unknown_ground_truth(shape):
    """7 % of the ground-truth pixels carry Middlebury's marker 1e10: not valid."""
    w, h, R, seed = shape
    gt, flow = inputs(*shape)
    rng = np.random.default_rng(200 + seed)
    g = flo_payload(gt)
    unknown = rng.random((h, w)) < 0.07
    g[unknown] = 1e10
    fl = as_flow(flow, "planar", np.float64)
    ref, ref_maps = score_ref.score_flow(fl, g)
    precondition(ref, ref_maps)
    assert np.all(ref[:, 0] == w * h - np.count_nonzero(unknown)) and np.count_nonzero(unknown) > 0
    s = evaluate.score_flow(dev(fl), dev(g), maps="float64")
    compare(s.host(), ref, s.maps.to_numpy(), ref_maps)
    assert np.all(np.isnan(s.maps.to_numpy()[:, :, unknown]))


def test_nan_flow_is_dropped():
    w, h, R, seed = SHAPES[1]
    gt, flow = inputs(*SHAPES[1])
    fl = as_flow(flow, "planar", np.float64)
    fl[0, 0, 3, 5] = np.nan
    fl[1, 1, 0, 0] = np.nan
    fl[2, 0, h - 1, w - 1] = fl[2, 1, h - 1, w - 1] = np.nan
    ref, ref_maps = score_ref.score_flow(fl, flo_payload(gt))
    assert np.all(ref[:, 0] == w * h) and np.all(ref[:, 1] == w * h - 1) and np.all(ref[:, 13] == w * h - 1)
    s = evaluate.score_flow(dev(fl), dev(flo_payload(gt)), maps="float64")
    compare(s.host(), ref, s.maps.to_numpy(), ref_maps)


def test_ee_cap():
    """EE above the cap is not kept (the reference's 50 by default; here 1.2 and +inf)."""
    gt, flow = inputs(*SHAPES[2])
    fl, g = as_flow(flow, "interleaved", np.float64), flo_payload(gt)
    for cap in (1.2, np.inf):
        ref, _ = score_ref.score_flow(fl, g, "interleaved", ee_cap=cap)
        s = evaluate.score_flow(dev(fl), dev(g), layout="interleaved", ee_cap=cap)
        compare(s.host(), ref)
    assert 0 < score_ref.score_flow(fl, g, "interleaved", ee_cap=1.2)[0][0, 1] < fl[0].size // 2


# ------------------------------------------------------------------ order statistics

def _exact_gt(shape):
    """A ground truth on a grid of 1/8, so that gt + 3 and gt + 4 are exact."""
    gt, _ = inputs(*shape)
    return np.round(gt * 8) / 8


def test_ties_everywhere():
    w, h, R, seed = SHAPES[3]
    gt = _exact_gt(SHAPES[3])
    flow = (gt + np.array([3.0, 4.0])[:, None, None])[None]
    fl, g = as_flow(flow, "planar", np.float32), flo_payload(gt)
    ref, ref_maps = score_ref.score_flow(fl, g)
    assert np.all(ref[0, [2, 4, 9, 10, 11]] == 5.0) and ref[0, 3] == 0.0
    s = evaluate.score_flow(dev(fl), dev(g), maps="float64")
    compare(s.host(), ref, s.maps.to_numpy(), ref_maps)
    assert np.all(s.ee_A == 5.0) and np.all(s.ee_R == 1.0)


def test_rank_on_the_boundary_of_two_values():
    w, h = 20, 10
    rng = np.random.default_rng(7)
    gt = np.round(rng.normal(0, 2, (2, h, w)) * 8) / 8
    low = np.zeros(h * w, bool)
    low[rng.permutation(h * w)[:100]] = True            # 100 errors of 5, 100 of 10
    scale = np.where(low.reshape(h, w), 1.0, 2.0)
    flow = (gt + np.array([3.0, 4.0])[:, None, None] * scale)[None]
    fl, g = as_flow(flow, "interleaved", np.float64), flo_payload(gt)
    pct = (50.0, 50.5, 0.5, 100.0)                      # k = 100, 101, 1, 200
    assert [score_ref.rank(p, 200) for p in pct] == [100, 101, 1, 200]
    ref, _ = score_ref.score_flow(fl, g, "interleaved", pct=pct)
    assert list(ref[0, 9:13]) == [5.0, 10.0, 5.0, 10.0]
    s = evaluate.score_flow(dev(fl), dev(g), layout="interleaved", percentiles=pct)
    compare(s.host(), ref)
    assert list(s.ee_A[0]) == [5.0, 10.0, 5.0, 10.0]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_minimum_and_maximum(shape):
    """p = 100 is the maximum; a p small enough that k = 1 the minimum; four percentiles, one
    threshold, none for AE."""
    w, h, R, seed = shape
    gt, flow = inputs(*shape)
    fl, g = as_flow(flow, "planar", np.float64), flo_payload(gt)
    pct = (100.0, 1e-6, 50.0, 99.9)
    ref, ref_maps = score_ref.score_flow(fl, g, pct=pct, ee_thr=(1.0,), ae_thr=())
    s = evaluate.score_flow(dev(fl), dev(g), percentiles=pct, ee_thresholds=(1.0,), ae_thresholds=())
    compare(s.host(), ref)
    t = s.host()
    for r in range(R):
        assert t[r, 9] == t[r, 4] == ref_maps[r, 0].max() and t[r, 10] == ref_maps[r, 0].min()
        assert t[r, 21] == t[r, 16] and np.all(np.isnan(t[r, 6:9])) and np.all(np.isnan(t[r, 17:21]))
    assert s.ae_R.shape == (R, 0) and s.ee_R.shape == (R, 1)


# ------------------------------------------------------------------ empty sets, guards, repeatability

def test_mask_of_zeros_and_guard_cells():
    """n = 0: NaN statistics; nothing is written outside the table and the maps."""
    w, h, R, seed = SHAPES[1]
    gt, flow = inputs(*SHAPES[1])
    fl, g = as_flow(flow, "planar", np.float32), flo_payload(gt)
    table = dev(np.full((R + 2, 32), 7.25))
    maps = dev(np.full((R + 2, 2, h, w), 7.25, np.float32))
    s = evaluate.score_flow(dev(fl), dev(g), mask=dev(np.zeros((h, w), np.uint8)), out=table[1:R + 1],
                            maps=maps[1:R + 1])
    t, m = table.to_numpy(), maps.to_numpy()
    assert np.all(t[[0, R + 1]] == 7.25) and np.all(m[[0, R + 1]] == 7.25)
    ref, ref_maps = score_ref.score_flow(fl, g, mask=np.zeros((h, w), np.uint8))
    compare(t[1:R + 1], ref, m[1:R + 1], ref_maps)
    assert np.all(t[1:R + 1, [0, 1, 13]] == 0) and np.all(np.isnan(t[1:R + 1, 2:13])) and np.all(np.isnan(m[1:R + 1]))
    assert np.all(t[1:R + 1, 25:] == 0) and np.all(np.isnan(s.ee_mean))
    # and with a mask again: the guards stay, the rows are rewritten
    mask = np.ones((h, w), np.uint8)
    evaluate.score_flow(dev(fl), dev(g), mask=dev(mask), out=table[1:R + 1], maps=maps[1:R + 1])
    t, m = table.to_numpy(), maps.to_numpy()
    assert np.all(t[[0, R + 1]] == 7.25) and np.all(m[[0, R + 1]] == 7.25)
    compare(t[1:R + 1], *score_ref.score_flow(fl, g)[:1])


@pytest.mark.parametrize("shape", SHAPES[1:], ids=IDS[1:])
def test_same_call_twice_and_host_entry(shape):
    """The same call gives the same bits, and the host entry the device entry's bits."""
    w, h, R, seed = shape
    gt, flow = inputs(*shape)
    fl, g = as_flow(flow, "planar", np.float32), flo_payload(gt)
    mask = (np.random.default_rng(seed).random((h, w)) < 0.8).astype(np.uint8)
    dfl, dg, dm = dev(fl), dev(g), dev(mask)
    a = evaluate.score_flow(dfl, dg, mask=dm, maps="float64")
    b = evaluate.score_flow(dfl, dg, mask=dm, maps="float64")
    c = evaluate.score_flow(fl, g, mask=mask, maps="float64")
    ta, tb, tc = (x.host().view(np.uint64) for x in (a, b, c))
    np.testing.assert_array_equal(ta, tb)
    np.testing.assert_array_equal(ta, tc)
    ma, mb = a.maps.to_numpy().view(np.uint64), b.maps.to_numpy().view(np.uint64)
    np.testing.assert_array_equal(ma, mb)
    np.testing.assert_array_equal(ma, c.maps.view(np.uint64))
    compare(c.table, score_ref.score_flow(fl, g, mask=mask)[0])
    # a strided host mask (bool), float32 host maps
    pad = np.zeros((h, w + 5), bool)
    pad[:, 2:w + 2] = mask != 0
    d = evaluate.score_flow(fl, g, mask=pad[:, 2:w + 2], maps="float32")
    np.testing.assert_array_equal(d.table.view(np.uint64), tc)
    np.testing.assert_array_equal(d.maps.view(np.uint32), c.maps.astype(np.float32).view(np.uint32))


def test_agrees_with_flow_errors_dev():
    """A 1-record planar float64 call with no mask against the parent's foto_flow_errors_dev."""
    w, h, R, seed = SHAPES[3]
    gt, flow = inputs(*SHAPES[3])
    fl = as_flow(flow, "planar", np.float64)
    g = as_flow(gt[None], "planar", np.float64)
    s = evaluate.score_flow(dev(fl), dev(g), gt_layout="planar")
    dfl, dg = dev(fl), dev(g)
    old = evaluate.flow_errors_device(dfl[0, 0], dfl[0, 1], dg[0, 0], dg[0, 1], w, h)
    np.testing.assert_allclose(s.host()[0, [2, 3, 14, 15]], old, rtol=RTOL, atol=0)


# ------------------------------------------------------------------ frames

@pytest.mark.parametrize("shape", SHAPES[1:], ids=IDS[1:])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("masked", [False, True], ids=["all", "mask"])
def test_score_frames(shape, dtype, masked):
    w, h, K, seed = shape[0], shape[1], 3, shape[3]
    rng = np.random.default_rng(300 + seed)
    truth = rng.random((h, w))
    noisy = np.clip(truth + rng.normal(0, 0.05, (K, h, w)), 0, 1)
    frames = np.uint8(255 * noisy) if dtype == np.uint8 else noisy.astype(np.float32)
    truth_in = np.uint8(255 * truth) if dtype == np.uint8 else truth
    mask = (rng.random((h, w)) < 0.7).astype(np.uint8) if masked else None
    ref = score_ref.score_frames(frames, truth_in, mask=mask, ne_eps=0.5)
    s = evaluate.score_frames(dev(frames), dev(truth_in), mask=dev(mask) if masked else None, ne_eps=0.5)
    t = s.host()
    print("max relative difference:", np.max(np.abs(t - ref) / np.abs(ref)))
    np.testing.assert_array_equal(t[:, [0, 3]], ref[:, [0, 3]])
    np.testing.assert_allclose(t[:, 1:3], ref[:, 1:3], rtol=RTOL, atol=0)
    assert s.ie.shape == (K,) and np.all(s.ne < s.ie)
    # one frame of a larger buffer, through a strided view, and numpy arrays
    big = dev(np.concatenate([frames, frames], axis=2))
    one = evaluate.score_frames(big[1, :, w:], dev(truth_in), mask=dev(mask) if masked else None, ne_eps=0.5)
    np.testing.assert_array_equal(one.host().view(np.uint64), t[1:2].view(np.uint64))
    assert np.ndim(one.ie) == 0
    hst = evaluate.score_frames(frames, truth_in, mask=mask, ne_eps=0.5)
    np.testing.assert_array_equal(hst.host().view(np.uint64), t.view(np.uint64))


def test_score_frames_smallest_and_empty():
    ref = score_ref.score_frames(np.full((1, 1), 0.25), np.full((1, 1), 0.75))
    s = evaluate.score_frames(dev(np.full((1, 1), 0.25)), dev(np.full((1, 1), 0.75)))
    np.testing.assert_array_equal(s.host(), ref)
    assert list(ref[0]) == [1.0, 127.5, 127.5, 127.5]
    e = evaluate.score_frames(dev(np.zeros((2, 4, 5), np.float32)), dev(np.ones((4, 5))), mask=dev(np.zeros((4, 5))))
    assert np.all(e.n == 0) and np.all(np.isnan(e.host()[:, 1:]))


# ------------------------------------------------------------------ argument errors on the device

def test_argument_errors():
    w, h, R, seed = SHAPES[1]
    gt, flow = inputs(*SHAPES[1])
    fl, g = as_flow(flow, "planar", np.float32), flo_payload(gt)
    dfl, dg = dev(fl), dev(g)
    table = dev(np.full((R, 32), 7.25))
    L = _lib.lib()

    def call(f, gg, tab, maps=None, records_gt=1):
        a, b = _lib.Flow(f, _lib.FOTO_F32, 0, R), _lib.Flow(gg, _lib.FOTO_F32, 1, records_gt)
        return L.foto_score_flow_dev(ctypes.byref(a), ctypes.byref(b), None, w, h, None, ctypes.c_void_p(tab),
                                     ctypes.c_void_p(maps), _lib.FOTO_F32, None)

    assert call(dfl.ptr, dg.ptr, table.ptr) == 0
    assert call(fl.ctypes.data, dg.ptr, table.ptr) == _lib.FOTO_ERR_ARG            # a host flow
    assert call(dfl.ptr, g.ctypes.data, table.ptr) == _lib.FOTO_ERR_ARG            # a host ground truth
    host_table = np.zeros((R, 32))
    assert call(dfl.ptr, dg.ptr, host_table.ctypes.data) == _lib.FOTO_ERR_ARG      # a host table
    assert call(dfl.ptr, dg.ptr, dfl.ptr) == _lib.FOTO_ERR_ARG                     # the table over the flow
    assert call(dfl.ptr, dg.ptr, dg.ptr) == _lib.FOTO_ERR_ARG                      # the table over the ground truth
    assert call(dfl.ptr, dg.ptr, table.ptr, maps=dfl.ptr) == _lib.FOTO_ERR_ARG     # the maps over the flow
    assert call(dfl.ptr, dg.ptr, table.ptr, maps=table.ptr) == _lib.FOTO_ERR_ARG   # the maps over the table
    assert call(dfl.ptr, dfl.ptr, table.ptr, records_gt=2) == _lib.FOTO_ERR_ARG    # 2 records for 3
    assert L.foto_last_error()
    table.copy_from(dev(np.full((R, 32), 7.25)))
    for bad in (lambda: call(dfl.ptr, dg.ptr, dfl.ptr), lambda: call(fl.ctypes.data, dg.ptr, table.ptr)):
        assert bad() == _lib.FOTO_ERR_ARG
    assert np.all(table.to_numpy() == 7.25)                                        # the outputs are untouched
    np.testing.assert_array_equal(dfl.to_numpy(), fl)
    with pytest.raises(_lib.FotoError):
        evaluate.score_flow(dfl, dg, out=_overlapping_out(dfl, R))
    # frames: a host buffer, the table over the frames
    fr = np.zeros((2, h, w))
    dfr = dev(fr)
    with pytest.raises(_lib.FotoError):
        evaluate.score_frames(dfr, dev(fr[0]), out=dfr.reshape(-1)[:8].reshape(2, 4))
    im = _lib.Image(fr.ctypes.data, _lib.FOTO_F64, w, 1, 1.0)
    tr = _lib.Image(dfr.ptr, _lib.FOTO_F64, w, 1, 1.0)
    assert L.foto_score_frames_dev(ctypes.byref(im), 2, w * h, ctypes.byref(tr), None, w, h, 1.0,
                                   ctypes.c_void_p(table.ptr), None) == _lib.FOTO_ERR_ARG


def _overlapping_out(dflow, R):
    """A float64 (R, 32) view of the first bytes of a float32 flow buffer: an `out` over an input."""
    class View:
        __cuda_array_interface__ = dict(shape=(R, 32), typestr="<f8", data=(dflow.ptr, False), version=3, strides=None)
    return View()


# ------------------------------------------------------------------ main.py --stats

def test_cli_stats(gold, tmp_path):
    """Without --stats stdout and the benchmark file are what they were; with it the extra lines
    follow the reference's."""
    import main as M
    import utils as U
    d = gold("cli.npz")
    p0, p1 = tmp_path / "f0.png", tmp_path / "f1.png"
    d["png0"].tofile(p0)
    d["png1"].tofile(p1)
    w, h = 36, 28
    rng = np.random.default_rng(11)
    uG, vG = rng.normal(0, 0.5, w * h), rng.normal(0, 0.5, w * h)
    U.saveFlo(w, h, uG, vG, str(tmp_path / "gt.flo"))
    runs = {}
    for name, extra in (("plain", []), ("stats", ["--stats"])):
        bench = tmp_path / f"{name}.txt"
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            u, v, m = M.main([str(p0), str(p1), "--algo=GN", f"--ground-truth={tmp_path / 'gt.flo'}",
                              f"--save-benchmark={bench}"] + extra)
        strip = lambda s: re.sub(r"time: \S+", "time: T", s)
        runs[name] = (strip(buf.getvalue()), strip(open(bench).read()), u, v)
    out0, txt0, u, v = runs["plain"]
    out1, txt1, _, _ = runs["stats"]
    names = ["EE-R0.5", "EE-R1.0", "EE-R2.0", "EE-A50", "EE-A75", "EE-A95",
             "AE-R2.5", "AE-R5.0", "AE-R10.0", "AE-A50", "AE-A75", "AE-A95"]
    assert [ln.split(":")[0] for ln in txt0.split("\n")] == ["EE-mean", "EE-stddev", "AE-mean", "AE-stddev", "IE", "time"]
    assert txt1.startswith(txt0 + "\n") and [ln.split(":")[0] for ln in txt1[len(txt0) + 1:].split("\n")] == names
    assert "EE-R" not in out0 and "AE-A" not in out0
    extra_out = [ln for ln in out1.split("\n") if ln not in out0.split("\n")]
    assert [ln.split(":")[0] for ln in extra_out] == [" - " + n for n in names]
    assert out1.replace("\n".join(extra_out) + "\n", "") == out0
    flow = np.stack([u.reshape(h, w), v.reshape(h, w), np.zeros((h, w))])
    _, _, uu, vv = U.openFlo(str(tmp_path / "gt.flo"))
    ref, _ = score_ref.score_flow(flow, np.stack([uu, vv], -1).reshape(h, w, 2))
    want = list(ref[0, 5:8]) + list(ref[0, 9:12]) + list(ref[0, 17:20]) + list(np.rad2deg(ref[0, 21:24]))
    got = [float(ln.split(": ")[1]) for ln in txt1[len(txt0) + 1:].split("\n")]
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)
