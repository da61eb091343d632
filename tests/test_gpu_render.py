"""Rendering on the GPU (include/foto.h, "rendering"; foto/render.py): flow buffers as the *_dev
entries write them -> the clipped reconstruction, the luminosity map and the colour code, for one
or many records, from strided uint8 / float32 / float64 frames with one or three channels.

Checkers.  Warp: oracle.apply_opticalflow per record and channel on the flow widened to float64
and np.float64(pixel) / divisor, np.clip, np.uint8(255 * x); uint8 results must be equal, float
results equal as values (np.array_equal(..., equal_nan=True): a black pixel under a negative
bilinear weight gives -0.0, and np.clip's treatment of signed zeros is no contract).  The oracle
cannot index with a NaN displacement (its int64 cast of NaN is out of range), so the checker feeds
it 0 there and sets the pixel to NaN afterwards -- the weights are NaN whatever the taps -- which
is the deviation include/foto.h states (NaN stays NaN in a float output and is 0 in uint8).
Colour: a float64 numpy restatement of bin/color_flow.flow_to_color, written here.  The device's
atan2 is the one operation not correctly rounded, so a sample is *sensitive* if the checker's
uint8 changes when its arctan2 result moves by j * np.spacing for some j in -6..6 (the OpenCL bound
for atan2).  Outside the sensitive set the output must be equal, inside it one of the 13
variants; the sensitive share must be <= 1 % of a case's samples (grids of at least 100 samples:
on a 1 x 1 or 2 x 1 grid one sample is already a third or a sixth of the case).  The maximum
radius must equal the checker's exactly.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import PKG  # noqa: E402  (puts the package on sys.path)

from foto import _lib, evaluate, gn, render  # noqa: E402
from foto import device as D  # noqa: E402
from foto.bb import BBSolver  # noqa: E402
from foto.device import DeviceArray  # noqa: E402
from foto.synthetic import textured_pair  # noqa: E402
from oracle import foto_oracle as O  # noqa: E402

GRIDS = [(37, 29), (7, 6), (1, 1), (2, 1)]
RECORDS = [1, 4]
NP_DT = {"float32": np.float32, "float64": np.float64}


# ------------------------------------------------------------------ inputs

def warp_flow(w, h, R, seed=0):
    """(R, 3, n) float64: u, v ~ N(0, 3), m ~ N(0, 0.3), plus the hand-set entries (as many as the
    grid has room for; every value is a float32, so both flow dtypes hold the same field)."""
    n = w * h
    rng = np.random.default_rng(seed + 1000 * R + n)
    f = np.empty((R, 3, n))
    f[:, :2] = rng.normal(0, 3, (R, 2, n))
    f[:, 2] = rng.normal(0, 0.3, (R, n))
    f = f.astype(np.float32).astype(np.float64)
    hand = [(0, 1000.0, 0.0, None), (1, -1000.0, 0.0, None), (2, 0.0, 1000.0, None), (3, 0.0, -1000.0, None),
            (4, 2.0, -1.0, None), (5, 0.0, 0.0, None), (6, -0.0, -0.0, None), (7, np.nan, 0.5, None),
            (8, 0.0, 0.0, -1.5), (9, 0.0, 0.0, 3.0)]   # (pixel, u, v, m): borders, integers, -0, NaN, clip ends
    for k in range(R):
        for p, u, v, m in hand:
            if n > 10:
                q = (p * 7 + 3 * k) % n
            elif (p // n) % R == k:     # a tiny grid: the entries spread over pixels, then records
                q = p % n
            else:
                continue
            f[k, 0, q], f[k, 1, q] = u, v
            if m is not None:
                f[k, 2, q] = m
    return f


def flow_device(f, w, h, dtype, layout):
    """the (R, 3, n) float64 field as a device flow array of `dtype` in `layout`"""
    R = f.shape[0]
    if layout == "planar":
        a = f.reshape(R, 3, h, w)
    else:
        a = np.stack([f[:, 0], f[:, 1]], axis=-1).reshape(R, h, w, 2)
    return DeviceArray.from_numpy(np.ascontiguousarray(a, dtype=NP_DT[dtype]))


def source(kind, C, w, h, seed=0):
    """(device view, values (h, w, C) float64 = pixel / divisor, reconstruct kwargs, has_channel_axis)"""
    rng = np.random.default_rng(seed + 17 * C + w)
    if kind == "hwc_u8":      # interleaved uint8: stride_x = 3 (C = 1: one channel of such a frame)
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        img.reshape(-1)[:: 5] = 255
        d = DeviceArray.from_numpy(img)
        if C == 1:
            return d[:, :, 1], img[:, :, 1:2].astype(np.float64) / 255, {}, False
        return d, img.astype(np.float64) / 255, {}, True
    if kind == "chw_f32":     # planar float32
        img = rng.random((C, h, w)).astype(np.float32)
        return DeviceArray.from_numpy(img), np.moveaxis(img, 0, -1).astype(np.float64), dict(channels_last=False), True
    assert kind == "padded_f64"   # a row-padded float64 view
    if C == 1:
        buf = rng.random((h, w + 5))
        return DeviceArray.from_numpy(buf)[:, :w], buf[:, :w, None].copy(), {}, False
    buf = rng.random((h, w + 5, C))
    return DeviceArray.from_numpy(buf)[:, :w, :], buf[:, :w, :].copy(), {}, True


# ------------------------------------------------------------------ checkers

def warp_checker(vals, f, w, h, use_m):
    """(R, h, w, C) float64: clip(apply_opticalflow(vals_c, u_k, v_k, w, h, m_k), 0, 1)"""
    R, C = f.shape[0], vals.shape[2]
    out = np.empty((R, h, w, C))
    for k in range(R):
        u, v = f[k, 0].copy(), f[k, 1].copy()
        nan = np.isnan(u) | np.isnan(v)
        u[nan], v[nan] = 0.0, 0.0
        for c in range(C):
            x = O.apply_opticalflow(vals[:, :, c].ravel(), u, v, w, h, f[k, 2] if use_m else None)
            x[nan] = np.nan
            out[k, :, :, c] = np.clip(x, 0, 1).reshape(h, w)
    return out


def to_u8(x):
    """np.uint8(255 * x) (main.py:142), NaN -> 0"""
    return np.where(np.isnan(x), 0, np.uint8(255 * np.where(np.isnan(x), 0.0, x))).astype(np.uint8)


def colorwheel():
    RY, YG, GC, CB, BM, MR = 15, 6, 4, 11, 13, 6
    cols = [(255, 255 * i // RY, 0) for i in range(RY)]
    cols += [(255 - 255 * i // YG, 255, 0) for i in range(YG)]
    cols += [(0, 255, 255 * i // GC) for i in range(GC)]
    cols += [(0, 255 - 255 * i // CB, 255) for i in range(CB)]
    cols += [(255 * i // BM, 0, 255) for i in range(BM)]
    cols += [(255, 0, 255 - 255 * i // MR) for i in range(MR)]
    return np.array(cols, dtype=np.float64)


def color_checker(u, v, maxmotion, shift=0):
    """((n, 3) uint8, maxrad) of one record, float64 in flow_to_color's order; `shift` moves the
    arctan2 result by that many np.spacing steps"""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        unknown = (np.abs(u) > 1e9) | (np.abs(v) > 1e9) | np.isnan(u) | np.isnan(v)
    rad = np.sqrt(u * u + v * v)
    maxrad = float(np.max(rad[~unknown])) if np.any(~unknown) else -1.0
    if maxmotion > 0:
        maxrad = float(maxmotion)
    if maxrad <= 0:
        maxrad = 1.0
    fx, fy = np.where(unknown, 0.0, u) / maxrad, np.where(unknown, 0.0, v) / maxrad
    cw = colorwheel()
    ncols = cw.shape[0]
    r = np.sqrt(fx * fx + fy * fy)
    at = np.arctan2(-fy, -fx)
    at = at + shift * np.spacing(at)
    a = at / np.pi
    fk = (a + 1.0) / 2.0 * (ncols - 1)
    k0 = np.clip(fk.astype(np.int32), 0, ncols - 1)
    k1 = (k0 + 1) % ncols
    f = fk - k0
    img = np.zeros((u.size, 3), dtype=np.uint8)
    for b in range(3):
        col0, col1 = cw[k0, b] / 255.0, cw[k1, b] / 255.0
        col = (1 - f) * col0 + f * col1
        col = np.where(r <= 1, 1 - r * (1 - col), col * 0.75)
        img[:, b] = np.where(unknown, 0, (255.0 * col).astype(np.int32)).astype(np.uint8)
    return img, maxrad


def color_variants(u, v, maxmotion):
    """(image, the 13 shifted images stacked, sensitive mask, maxrad) of one record"""
    base, maxrad = color_checker(u, v, maxmotion)
    var = np.stack([color_checker(u, v, maxmotion, j)[0] for j in range(-6, 7)])
    return base, var, np.any(var != base[None], axis=0), maxrad


def assert_color(got, uv, maxmotion, share=True):
    """got (R, n, 3) uint8 against the checker on uv (R, 2, n)"""
    for k in range(uv.shape[0]):
        base, var, sens, _ = color_variants(uv[k, 0], uv[k, 1], maxmotion)
        print(f"record {k}: {int(sens.sum())} sensitive of {sens.size} samples, "
              f"{int((got[k] != base).sum())} differ from the unshifted checker")
        assert np.array_equal(got[k][~sens], base[~sens])
        assert np.all(np.any(var == got[k][None], axis=0)[sens])
        if share:
            assert sens.sum() <= 0.01 * sens.size


def color_flow_field(w, h, R, seed=0):
    """(R, 2, n) float64 of float32 values: u ~ N(0, 3), v ~ N(0, 2), the hand-set entries, and (R > 1)
    record 2 with every pixel unknown"""
    n = w * h
    rng = np.random.default_rng(seed + 77 * R + n)
    f = np.stack([rng.normal(0, 3, (R, n)), rng.normal(0, 2, (R, n))], axis=1).astype(np.float32).astype(np.float64)
    hand = [(0.0, 0.0), (1.5, 0.0), (-1.5, 0.0), (0.0, 1.5), (0.0, -1.5), (np.nan, 1.0), (2e9, 0.0)]
    for k in range(R):
        for i, (u, v) in enumerate(hand):
            if n > 7:
                q = (i * 5 + 2 * k) % n
            elif (i // n) % R == k:     # a tiny grid: the entries spread over pixels, then records
                q = i % n
            else:
                continue
            f[k, 0, q], f[k, 1, q] = u, v
    if R > 2:
        f[2, 0, ::2], f[2, 1, ::2] = np.nan, 0.0
        f[2, 0, 1::2], f[2, 1, 1::2] = 1.0, -2e9
    return f


def odd_out(shape):
    """a contiguous uint8 device array whose address is odd: the luminosity then stores byte by byte
    instead of 4 pixels per 32-bit word, and no entry may assume more than element alignment"""
    size = int(np.prod(shape))
    d = DeviceArray((size + 1,), np.uint8)[1:].reshape(shape)
    assert d.ptr % 4 == 1
    return d


# ------------------------------------------------------------------ 1. warp parity

@pytest.mark.parametrize("kind,C", [(k, c) for k in ("hwc_u8", "chw_f32", "padded_f64") for c in (1, 3)])
@pytest.mark.parametrize("R", RECORDS)
@pytest.mark.parametrize("w,h", GRIDS)
def test_warp_parity(w, h, R, kind, C):
    f = warp_flow(w, h, R)
    src, vals, kw, has_c = source(kind, C, w, h)
    shape = (R, h, w) + ((C,) if has_c else ())
    for use_m in (True, False):
        want = warp_checker(vals, f, w, h, use_m).reshape(shape)
        if (w, h) == (37, 29):
            assert np.isnan(want).any() and (want == 0).any() and (want == 1).any()   # NaN and both clip ends
        for fdt in ("float32", "float64"):
            for layout in ("planar", "interleaved"):
                if use_m and layout == "interleaved":
                    continue
                fl = flow_device(f, w, h, fdt, layout)
                got = render.reconstruct(src, fl, layout=layout, use_m=use_m, dtype="uint8", **kw)
                assert got.shape == shape and got.dtype == np.uint8
                assert np.array_equal(got.to_numpy(), to_u8(want)), (use_m, fdt, layout)
                got = render.reconstruct(src, fl, layout=layout, use_m=use_m, dtype="float64", **kw).to_numpy()
                assert np.array_equal(got, want, equal_nan=True), (use_m, fdt, layout)
                got = render.reconstruct(src, fl, layout=layout, use_m=use_m, dtype="float32", **kw).to_numpy()
                assert got.dtype == np.float32
                assert np.array_equal(got, want.astype(np.float32), equal_nan=True), (use_m, fdt, layout)


def test_warp_unbatched_and_odd_out():
    """a (3, h, w) flow gives an (h, w, C) result; a uint8 `out` may sit at an odd address; the
    host convenience gives the checker's values"""
    w, h = 37, 29
    f = warp_flow(w, h, 1)
    src, vals, kw, _ = source("hwc_u8", 3, w, h)
    want = to_u8(warp_checker(vals, f, w, h, True))[0]
    fl = flow_device(f, w, h, "float32", "planar")
    got = render.reconstruct(src, fl.reshape(3, h, w))
    assert got.shape == (h, w, 3) and np.array_equal(got.to_numpy(), want)
    out = odd_out((1, h, w, 3))
    assert render.reconstruct(src, fl, out=out) is out
    assert np.array_equal(out.to_numpy()[0], want)
    host = render.reconstruct_host(vals[:, :, 0], f.reshape(1, 3, h, w), dtype="float64")
    assert np.array_equal(host, warp_checker(vals[:, :, :1], f, w, h, True)[..., 0], equal_nan=True)


@pytest.mark.parametrize("C", [2, 4])
@pytest.mark.parametrize("w,h", [(37, 29), (2, 1)])
def test_warp_other_channel_counts(w, h, C):
    """channel counts besides 1 and 3: the loop over channels is a run-time one"""
    R = 4
    f = warp_flow(w, h, R)
    img = np.random.default_rng(C).integers(0, 256, (h, w, C), dtype=np.uint8)
    want = to_u8(warp_checker(img.astype(np.float64) / 255, f, w, h, True))
    got = render.reconstruct(DeviceArray.from_numpy(img), flow_device(f, w, h, "float32", "planar"))
    assert got.shape == (R, h, w, C) and np.array_equal(got.to_numpy(), want)


# ------------------------------------------------------------------ 2. same build

@pytest.mark.parametrize("w,h", GRIDS)
def test_warp_equals_warp_dev(w, h):
    """float64 output with one channel = np.clip(foto_warp_dev) on the same float64 data, value for
    value, the NaN displacement included: both kernels call one tap function, which keeps its
    taps in the frame, and both give a NaN pixel there."""
    R = 4
    f = warp_flow(w, h, R)
    src, vals, kw, _ = source("padded_f64", 1, w, h)
    f1 = DeviceArray.from_numpy(np.ascontiguousarray(vals[:, :, 0]))
    fl = flow_device(f, w, h, "float64", "planar")
    for use_m in (True, False):
        got = render.reconstruct(src, fl, use_m=use_m, dtype="float64").to_numpy()
        for k in range(R):
            ref = evaluate.warp_device(f1, fl[k, 0], fl[k, 1], w, h, fl[k, 2] if use_m else None).to_numpy()
            assert np.array_equal(got[k], np.clip(ref, 0, 1), equal_nan=True), (use_m, k)


# ------------------------------------------------------------------ 3. luminosity

@pytest.mark.parametrize("fdt", ["float32", "float64"])
@pytest.mark.parametrize("R", RECORDS)
@pytest.mark.parametrize("w,h", GRIDS)
def test_luminosity(w, h, R, fdt):
    f = warp_flow(w, h, R)
    f[:, 2, 0] = np.nan
    if w * h > 2:
        f[:, 2, 1], f[:, 2, 2] = -1.5, 3.0
    m = f[:, 2].reshape(R, h, w)
    want = np.where(np.isnan(m), 0, np.uint8(255 * np.clip((np.nan_to_num(m) + 1) / 2, 0, 1))).astype(np.uint8)
    fl = flow_device(f, w, h, fdt, "planar")
    got = render.luminosity(fl)
    assert got.shape == (R, h, w) and got.dtype == np.uint8 and np.array_equal(got.to_numpy(), want)
    out = odd_out((R, h, w))
    assert render.luminosity(fl, out=out) is out and np.array_equal(out.to_numpy(), want)
    if R == 1:
        assert np.array_equal(render.luminosity(fl.reshape(3, h, w)).to_numpy(), want[0])


# ------------------------------------------------------------------ 4. colour

@pytest.mark.parametrize("maxmotion", [0.0, 2.0])
@pytest.mark.parametrize("R", RECORDS)
@pytest.mark.parametrize("w,h", GRIDS)
def test_color(w, h, R, maxmotion):
    sys.path.insert(0, os.path.join(PKG, "bin"))
    try:
        from color_flow import flow_to_color
    finally:
        sys.path.pop(0)
    n = w * h
    f = color_flow_field(w, h, R)
    want_mr = np.array([color_checker(f[k, 0], f[k, 1], maxmotion)[1] for k in range(R)])
    if R > 2:
        assert want_mr[2] == (2.0 if maxmotion > 0 else 1.0)   # every pixel unknown
    f3 = np.concatenate([f, np.zeros((R, 1, n))], axis=1)
    for fdt in ("float32", "float64"):
        for layout in ("planar", "interleaved"):
            fl = flow_device(f3, w, h, fdt, layout)
            mr = DeviceArray.from_numpy(np.full(R, -7.0))
            got = render.flow_color(fl, layout=layout, maxmotion=maxmotion, maxrad=mr)
            assert got.shape == (R, h, w, 3) and got.dtype == np.uint8
            img = got.to_numpy().reshape(R, n, 3)
            assert np.array_equal(mr.to_numpy(), want_mr), (mr.to_numpy(), want_mr)   # exactly
            assert_color(img, f, maxmotion, share=3 * n >= 100)
            # the library's scratch instead of the caller's array, and an odd `out` address
            out = odd_out((R, h, w, 3))
            render.flow_color(fl, layout=layout, maxmotion=maxmotion, out=out)
            assert np.array_equal(out.to_numpy().reshape(R, n, 3), img)
    # against the float32 tool: at most one level, on at most 1 % of the samples
    for k in range(R):
        tool = flow_to_color(f[k, 0], f[k, 1], w, h, maxmotion).reshape(n, 3).astype(np.int32)
        d = np.abs(img[k].astype(np.int32) - tool)
        print(f"record {k}: {int((d > 0).sum())} of {d.size} samples differ from the float32 tool, max {int(d.max())}")
        assert d.max() <= 1
        if 3 * n >= 100:
            assert (d > 0).sum() <= 0.01 * d.size
    host, hmr = render.flow_color_host(f3.reshape(R, 3, h, w), maxmotion=maxmotion, return_maxrad=True)
    assert np.array_equal(host.reshape(R, n, 3), img) and np.array_equal(hmr, want_mr)


# ------------------------------------------------------------------ 5. end to end

def test_end_to_end_bb_path():
    w, h, Nt = 40, 30, 6
    f0, f1 = (x.reshape(h, w) for x in textured_pair(w, h))
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    with BBSolver.from_device(DeviceArray.from_numpy(f0), DeviceArray.from_numpy(f1), Nt) as s:
        s.iterate(3, stop_rules=False)
        path = s.flow_path_device(dtype="float32")
        rec = render.reconstruct(DeviceArray.from_numpy(rgb), path)
        lum = render.luminosity(path)
    assert path.shape == (Nt - 1, 3, h, w) and rec.shape == (Nt - 1, h, w, 3)
    f = path.to_numpy().astype(np.float64).reshape(Nt - 1, 3, h * w)
    assert np.abs(f[-1, :2]).max() > 0.01                  # a flow that moves something
    want = to_u8(warp_checker(rgb.astype(np.float64) / 255, f, w, h, True))
    assert np.array_equal(rec.to_numpy(), want)
    m = f[:, 2].reshape(Nt - 1, h, w)
    assert np.array_equal(lum.to_numpy(), np.uint8(255 * np.clip((m + 1) / 2, 0, 1)))


def test_end_to_end_gn_color():
    w, h = 40, 30
    f0, f1 = (x.reshape(h, w) for x in textured_pair(w, h, seed=3))
    with gn.Plan(w, h, 0.1, 0.2) as P:
        flow, info, _ = P.solve_device(DeviceArray.from_numpy(f0), DeviceArray.from_numpy(f1), dtype="float32")
        mr = DeviceArray((1,), np.float64)
        img = render.flow_color(flow, maxrad=mr)
    assert info == 0 and img.shape == (h, w, 3)
    f = flow.to_numpy().astype(np.float64).reshape(1, 3, h * w)
    assert mr.to_numpy()[0] == color_checker(f[0, 0], f[0, 1], 0.0)[1]
    assert_color(img.to_numpy().reshape(1, h * w, 3), f[:, :2], 0.0)


# ------------------------------------------------------------------ 6. contract

def _flow_desc(d, layout, R):
    fl = _lib.Flow()
    fl.data, fl.dtype, fl.layout, fl.records = d.ptr, _lib.FOTO_F64, layout, R
    return fl


def test_contract_errors_leave_out_untouched():
    w, h, R = 37, 29, 2
    L = _lib.lib()
    f = warp_flow(w, h, R)
    planar, inter = flow_device(f, w, h, "float64", "planar"), flow_device(f, w, h, "float64", "interleaved")
    src = DeviceArray.from_numpy(np.random.default_rng(0).random((h, w)))
    im = D.as_image(src)
    sentinel = np.full((R, h, w), 0xA5, dtype=np.uint8)
    out = DeviceArray.from_numpy(sentinel)
    host = np.zeros(R * 3 * h * w)
    hostp = host.ctypes.data

    def warp(image, fl, use_m, optr, odt=_lib.FOTO_U8):
        return L.foto_render_warp_dev(ctypes.byref(image), 1, 1, ctypes.byref(fl), use_m, w, h, ctypes.c_void_p(optr),
                                      odt, None)
    fp, fi = _flow_desc(planar, 0, R), _flow_desc(inter, 1, R)
    assert warp(im, fi, 1, out.ptr) == _lib.FOTO_ERR_ARG                     # layout 1 carries no m
    # aliasing: out inside the flow buffer, out on the frame
    assert warp(im, fp, 1, planar.ptr + 64, _lib.FOTO_F64) == _lib.FOTO_ERR_ARG
    one = _flow_desc(planar, 0, 1)
    assert L.foto_render_warp_dev(ctypes.byref(im), 1, 1, ctypes.byref(one), 0, w, h, ctypes.c_void_p(src.ptr),
                                  _lib.FOTO_F64, None) == _lib.FOTO_ERR_ARG
    # host pointers: the frame, the flow, out
    him = D.as_image({"ptr": hostp, "typestr": "<f8", "shape": (h, w), "strides": None})
    assert warp(him, fp, 1, out.ptr) == _lib.FOTO_ERR_ARG
    hf = _lib.Flow()
    hf.data, hf.dtype, hf.layout, hf.records = hostp, _lib.FOTO_F64, 0, R
    assert warp(im, hf, 1, out.ptr) == _lib.FOTO_ERR_ARG
    assert warp(im, fp, 1, hostp) == _lib.FOTO_ERR_ARG
    # a flow of more records than its allocation holds
    assert warp(im, _flow_desc(planar, 0, R + 1), 1, out.ptr) == _lib.FOTO_ERR_ARG
    # luminosity and colour: layout, aliasing, host pointers
    assert L.foto_render_lum_dev(ctypes.byref(fi), w, h, ctypes.c_void_p(out.ptr), None) == _lib.FOTO_ERR_ARG
    assert L.foto_render_lum_dev(ctypes.byref(fp), w, h, ctypes.c_void_p(planar.ptr), None) == _lib.FOTO_ERR_ARG
    assert L.foto_render_lum_dev(ctypes.byref(hf), w, h, ctypes.c_void_p(out.ptr), None) == _lib.FOTO_ERR_ARG
    out3 = DeviceArray.from_numpy(np.full((R, h, w, 3), 0xA5, dtype=np.uint8))
    assert L.foto_render_color_dev(ctypes.byref(fp), w, h, 0.0, ctypes.c_void_p(planar.ptr), None, None) == _lib.FOTO_ERR_ARG
    assert L.foto_render_color_dev(ctypes.byref(fp), w, h, 0.0, ctypes.c_void_p(out3.ptr), ctypes.c_void_p(hostp),
                                   None) == _lib.FOTO_ERR_ARG
    assert L.foto_render_color_dev(ctypes.byref(fp), w, h, 0.0, ctypes.c_void_p(out3.ptr),
                                   ctypes.c_void_p(planar.ptr), None) == _lib.FOTO_ERR_ARG
    assert L.foto_last_error()
    # nothing was written: the sentinels, the flow and the frame are as they were
    assert np.array_equal(out.to_numpy(), sentinel) and np.all(out3.to_numpy() == 0xA5)
    assert np.array_equal(planar.to_numpy().reshape(R, 3, -1), f, equal_nan=True)
    assert np.all(host == 0)
    # and the entries still work
    got = render.reconstruct(src, planar, out=out)
    assert np.array_equal(got.to_numpy(), to_u8(warp_checker(src.to_numpy()[:, :, None], f, w, h, True))[..., 0])


def _hip():
    return ctypes.CDLL(D.mapped_hip_runtimes()[0])   # the runtime libfoto is bound to


def test_caller_stream_orders_the_call():
    """The frame is produced by a foto_dev_memcpy on the null stream; the call runs for a
    non-blocking caller stream; the result is read after synchronising that stream only."""
    w, h, R = 37, 29, 4
    _lib.lib()
    hip = _hip()
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(stream), 1) == 0   # hipStreamNonBlocking
    try:
        f = warp_flow(w, h, R)
        src, vals, kw, _ = source("hwc_u8", 3, w, h)
        fl = flow_device(f, w, h, "float32", "planar")
        rec = render.reconstruct(src, fl, stream=stream.value)
        col = render.flow_color(fl, stream=stream.value)
        lum = render.luminosity(fl, stream=stream.value)
        assert hip.hipStreamSynchronize(stream) == 0
        assert np.array_equal(rec.to_numpy(), to_u8(warp_checker(vals, f, w, h, True)))
        assert_color(col.to_numpy().reshape(R, w * h, 3), f[:, :2], 0.0, share=False)
        m = f[:, 2].reshape(R, h, w)
        assert np.array_equal(lum.to_numpy(), np.uint8(255 * np.clip((m + 1) / 2, 0, 1)))
    finally:
        assert hip.hipStreamDestroy(stream) == 0


def test_scratch_grows_with_records():
    """maxrad_or_null = NULL: the library's scratch serves 1 record, then grows for 40"""
    w, h = 7, 6
    for R in (1, 40, 3):
        f = color_flow_field(w, h, R, seed=R)
        f3 = np.concatenate([f, np.zeros((R, 1, w * h))], axis=1)
        img = render.flow_color(flow_device(f3, w, h, "float32", "planar")).to_numpy()
        assert_color(img.reshape(R, w * h, 3), f, 0.0, share=False)
