"""GPU evaluation helpers: the backward warp and the flow / intensity
error metrics of the reference's utils.py, through libfoto's C ABI.

warp            utils.apply_opticalflow (utils.py:186-248)  bit-identical
flow_errors     utils.EE + utils.AE     (utils.py:294-338)  up to summation order
intensity_error utils.IE                (utils.py:340-354)  up to summation order
"""
import ctypes

import numpy as np

from ._lib import check, dptr, f64, lib


def warp(f1, u, v, w, h, m=None):
    """(1 + m) f1 (or f1 if m is None) warped backwards by (u, v)."""
    n = w * h
    f = f64(f1, n, "f1")
    uu, vv = f64(u, n, "u"), f64(v, n, "v")
    mm = None if m is None else f64(np.broadcast_to(np.asarray(m, dtype=np.float64), (n,)), n, "m")
    out = np.empty(n)
    check(lib().foto_warp(dptr(f), dptr(uu), dptr(vv), dptr(mm) if mm is not None else None, w, h, dptr(out)))
    return out


def flow_errors(u, v, uGT, vGT, w, h):
    """(AEE, SDEE, AAE, SDAE): endpoint error <= 50 and non-NaN angular error (radians)."""
    n = w * h
    a = [f64(np.asarray(x, dtype=np.float64)[:n], n, name) for x, name in ((u, "u"), (v, "v"), (uGT, "uGT"), (vGT, "vGT"))]
    out = np.empty(4)
    check(lib().foto_flow_errors(*(dptr(x) for x in a), w, h, dptr(out)))
    return tuple(float(x) for x in out)


def intensity_error(I, IGT, w, h):
    """RMS of 255 I - 255 IGT."""
    n = w * h
    a, b = f64(I, n, "I"), f64(IGT, n, "IGT")
    out = np.empty(1)
    check(lib().foto_intensity_error(dptr(a), dptr(b), w, h, dptr(out)))
    return float(out[0])


# ------------------------------------------------------------------ device buffers
# The same three calls on contiguous float64 device arrays (foto.device.DeviceArray, torch ROCm
# tensors, ...): the same kernels and reduction order, without the uploads.

def _dev_f64(x, n, name):
    from . import device as D
    ptr, typestr, shape, strides, _ = D.device_interface(x)
    size = int(np.prod(shape, dtype=np.int64))
    if typestr != "<f8" or size != n:
        raise ValueError(f"{name}: expected {n} float64 values on the device, got {size} of {typestr}")
    if not D.c_contiguous(shape, strides, 8):
        raise ValueError(f"{name}: must be C-contiguous")
    return ctypes.c_void_p(ptr)


def warp_device(f1, u, v, w, h, m=None, out=None, stream=None):
    """warp() on device arrays; returns the DeviceArray (or ``out``) of h x w float64."""
    from . import device as D
    n = w * h
    if out is None:
        out = D.DeviceArray((h, w), np.float64)
    st = D.stream_handle(stream, f1, u, v)
    check(lib().foto_warp_dev(_dev_f64(f1, n, "f1"), _dev_f64(u, n, "u"), _dev_f64(v, n, "v"),
                              _dev_f64(m, n, "m") if m is not None else None, w, h, _dev_f64(out, n, "out"),
                              ctypes.c_void_p(st)))
    return out


def flow_errors_device(u, v, uGT, vGT, w, h, stream=None):
    """flow_errors() on device arrays (host scalars back)."""
    from . import device as D
    n = w * h
    out = np.empty(4)
    st = D.stream_handle(stream, u, v, uGT, vGT)
    check(lib().foto_flow_errors_dev(_dev_f64(u, n, "u"), _dev_f64(v, n, "v"), _dev_f64(uGT, n, "uGT"),
                                     _dev_f64(vGT, n, "vGT"), w, h, dptr(out), ctypes.c_void_p(st)))
    return tuple(float(x) for x in out)


def intensity_error_device(I, IGT, w, h, stream=None):
    """intensity_error() on device arrays (a host scalar back)."""
    from . import device as D
    n = w * h
    out = np.empty(1)
    st = D.stream_handle(stream, I, IGT)
    check(lib().foto_intensity_error_dev(_dev_f64(I, n, "I"), _dev_f64(IGT, n, "IGT"), w, h, dptr(out),
                                         ctypes.c_void_p(st)))
    return float(out[0])


# ------------------------------------------------------------------ scoring
# include/foto.h, "scoring": every record of a flow buffer against a ground truth in one call --
# float32 / float64, planar / interleaved, a mask, Middlebury's unknown-flow marker -- with the
# robustness measures R(t) and the accuracy percentiles A(p) beside the means; frames likewise,
# with the normalised interpolation error NE.  numpy arrays go through the host entry, device
# arrays through the device entry, which leaves the table on the device and never waits.

SCORE_COLS = 32
EE_THRESHOLDS = (0.5, 1.0, 2.0)
AE_THRESHOLDS = tuple(float(np.deg2rad(d)) for d in (2.5, 5.0, 10.0))   # radians
PERCENTILES = (50.0, 75.0, 95.0)
_GT_LAYOUTS = {"flo": "interleaved", "planar": "planar", "interleaved": "interleaved"}


def score_opts(ee_cap=50.0, ee_thresholds=EE_THRESHOLDS, ae_thresholds=AE_THRESHOLDS, percentiles=PERCENTILES):
    """The _lib.ScoreOpts of these settings; ValueError for more than four of a kind (the values
    themselves are foto_score_check's to judge)."""
    from . import _lib
    o = _lib.ScoreOpts()
    o.ee_cap = float(ee_cap)
    for name, cnt, vals in (("ee_thr", "n_ee_thr", ee_thresholds), ("ae_thr", "n_ae_thr", ae_thresholds),
                            ("pct", "n_pct", percentiles)):
        vals = [float(x) for x in vals]
        if len(vals) > 4:
            raise ValueError(f"{name}: {len(vals)} values; a score takes up to 4")
        setattr(o, cnt, len(vals))
        for i, x in enumerate(vals):
            getattr(o, name)[i] = x
    return o


class _Scored:
    """A statistics table as the library wrote it: ``.table`` is the raw [records][cols] array, a
    numpy array from the host entry and a device array from the device entry; ``host()`` is its
    numpy copy (a device table is downloaded once, on first use: that is the only wait)."""

    def __init__(self, table, batched):
        self.table = table
        self.batched = batched
        self._host = table if isinstance(table, np.ndarray) else None

    def host(self):
        if self._host is None:
            t = self.table
            if not hasattr(t, "to_numpy"):
                from . import device as D
                ptr, _, shape, _, _ = D.device_interface(t)
                host = np.empty(shape, np.float64)
                check(lib().foto_dev_memcpy(host.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), host.nbytes,
                                            D.D2H))
                self._host = host
            else:
                self._host = t.to_numpy()
        return self._host

    def _col(self, a, b=None):
        t = self.host()
        c = t[:, a] if b is None else t[:, a:b]
        return c if self.batched else c[0]


class FlowScore(_Scored):
    """score_flow's result, one entry per record (scalars for a flow without a record axis): ``n``
    valid pixels; ``ee_n``, ``ee_mean``, ``ee_std``, ``ee_max``, ``ee_R`` (one column per
    threshold), ``ee_A`` (one per percentile) and the ``ae_*`` twins in radians; ``maps`` when asked
    for.  ``ae_degrees()`` gives the AE statistics in degrees."""

    def __init__(self, table, batched, opts, maps=None):
        super().__init__(table, batched)
        self.opts = opts
        self.maps = maps
        self.ee_thresholds = tuple(opts.ee_thr[:opts.n_ee_thr])
        self.ae_thresholds = tuple(opts.ae_thr[:opts.n_ae_thr])
        self.percentiles = tuple(opts.pct[:opts.n_pct])

    n = property(lambda s: s._col(0))
    ee_n = property(lambda s: s._col(1))
    ee_mean = property(lambda s: s._col(2))
    ee_std = property(lambda s: s._col(3))
    ee_max = property(lambda s: s._col(4))
    ee_R = property(lambda s: s._col(5, 5 + s.opts.n_ee_thr))
    ee_A = property(lambda s: s._col(9, 9 + s.opts.n_pct))
    ae_n = property(lambda s: s._col(13))
    ae_mean = property(lambda s: s._col(14))
    ae_std = property(lambda s: s._col(15))
    ae_max = property(lambda s: s._col(16))
    ae_R = property(lambda s: s._col(17, 17 + s.opts.n_ae_thr))
    ae_A = property(lambda s: s._col(21, 21 + s.opts.n_pct))

    def ae_degrees(self):
        """{"mean", "std", "max", "A"} of AE in degrees (R is a fraction and has no unit)."""
        return {"mean": np.rad2deg(self.ae_mean), "std": np.rad2deg(self.ae_std), "max": np.rad2deg(self.ae_max),
                "A": np.rad2deg(self.ae_A)}


class FrameScore(_Scored):
    """score_frames' result, one entry per frame: ``n`` pixels, ``ie`` (utils.IE), ``ne``, ``max_abs``."""
    n = property(lambda s: s._col(0))
    ie = property(lambda s: s._col(1))
    ne = property(lambda s: s._col(2))
    max_abs = property(lambda s: s._col(3))


def _host_iface(a):
    """A numpy array as the mapping foto.device reads descriptors from (the array is kept alive)."""
    return {"ptr": a.ctypes.data, "typestr": a.dtype.str if a.dtype.itemsize > 1 else "|u1", "shape": a.shape,
            "strides": None if a.flags.c_contiguous else a.strides, "keep": a}


def _host_flow(a, what):
    a = np.asarray(a)
    if a.dtype not in (np.float32, np.float64):
        raise ValueError(f"{what}: dtype {a.dtype}; a flow is float32 or float64")
    return _host_iface(np.ascontiguousarray(a))


def _host_image(a, what):
    a = np.asarray(a)
    if a.dtype == np.bool_:
        a = a.view(np.uint8)
    if a.dtype not in (np.uint8, np.float32, np.float64):
        raise ValueError(f"{what}: dtype {a.dtype}; uint8 (or bool), float32 or float64")
    return _host_iface(a)


def score_flow(flow, gt, *, layout="planar", gt_layout="flo", mask=None, ee_cap=50.0, ee_thresholds=EE_THRESHOLDS,
               ae_thresholds=AE_THRESHOLDS, percentiles=PERCENTILES, maps=None, out=None, stream=None):
    """Every record of ``flow`` ((3, h, w) / (R, 3, h, w) planar or (h, w, 2) / (R, h, w, 2)
    interleaved, float32 or float64) against ``gt``: one record, used for every record of the flow,
    or as many as the flow; ``gt_layout`` "flo" is the interleaved payload of a .flo file.  numpy
    arrays take the host entry (foto_score_flow), device arrays the device entry
    (foto_score_flow_dev; ``out``: a float64 (R, 32) device array for the table).  ``mask``: a 2-D
    array, non-zero = evaluate.  ``maps``: "float32" / "float64" (or an array of shape
    ([R,] 2, h, w)) to get the per-pixel EE and AE, NaN where not valid, as ``.maps``.  Returns a
    FlowScore; on the device nothing waits until one of its statistics is read."""
    from . import _lib
    from . import device as D
    from .render import flow_arg
    if gt_layout not in _GT_LAYOUTS:
        raise ValueError(f"gt_layout {gt_layout!r}: 'flo' / 'interleaved' ((h, w, 2) pairs) or 'planar'")
    host = isinstance(flow, np.ndarray)
    if host != isinstance(gt, np.ndarray) or (mask is not None and host != isinstance(mask, np.ndarray)):
        raise TypeError("score_flow: flow, gt and mask are all numpy arrays or all device arrays")
    opts = score_opts(ee_cap, ee_thresholds, ae_thresholds, percentiles)
    fl, R, h, w, batched = flow_arg(_host_flow(flow, "flow") if host else flow, layout)
    g, Rg, hg, wg, _ = flow_arg(_host_flow(gt, "gt") if host else gt, _GT_LAYOUTS[gt_layout])
    if (hg, wg) != (h, w):
        raise ValueError(f"gt is {hg} x {wg} (h x w), the flow {h} x {w}")
    if Rg not in (1, R):
        raise ValueError(f"gt has {Rg} records: 1 (for every record) or the flow's {R}")
    im = None
    if mask is not None:
        im = D.as_image(_host_image(mask, "mask") if host else mask, 1.0)
        if im.shape != (h, w):
            raise ValueError(f"mask is {im.shape[0]} x {im.shape[1]} (h x w), the flow {h} x {w}")
    mshape = ((R,) if batched else ()) + (2, h, w)
    mptr, mcode, mobj = None, _lib.FOTO_F64, None
    if host:
        if out is not None:
            raise ValueError("out: a device array for the device entry; the host entry returns a numpy table")
        table = np.full((R, SCORE_COLS), np.nan)
        if maps is not None:
            mobj = maps if isinstance(maps, np.ndarray) else np.empty(mshape, D._dtype_name(maps, D._OUT_DTYPES, "maps"))
            if mobj.shape != mshape or mobj.dtype not in (np.float32, np.float64) or not mobj.flags.c_contiguous:
                raise ValueError(f"maps: expected a C-contiguous float32 / float64 array of shape {mshape}")
            mptr, mcode = mobj.ctypes.data, D._OUT_DTYPES[mobj.dtype.name]
        check(lib().foto_score_flow(ctypes.byref(fl), ctypes.byref(g), ctypes.byref(im) if im is not None else None,
                                    w, h, ctypes.byref(opts), ctypes.c_void_p(table.ctypes.data),
                                    ctypes.c_void_p(mptr), mcode))
        return FlowScore(table, batched, opts, mobj)
    own_maps = maps is not None and isinstance(maps, (str, type, np.dtype))
    if maps is not None and not own_maps:   # (the caller's buffers are judged before anything is allocated)
        ts = D.device_interface(maps)[1]
        mobj, mptr, mcode = D._shaped_target(maps, np.dtype(ts).name, D._OUT_DTYPES, mshape, "maps")
    if own_maps:
        D._dtype_name(maps, D._OUT_DTYPES, "maps")
    table, tptr, _ = D._shaped_target(out, "float64", {"float64": _lib.FOTO_F64}, (R, SCORE_COLS), "score tables")
    if own_maps:
        mobj, mptr, mcode = D._shaped_target(None, maps, D._OUT_DTYPES, mshape, "maps")
    st = D.stream_handle(stream, flow, gt)
    check(lib().foto_score_flow_dev(ctypes.byref(fl), ctypes.byref(g), ctypes.byref(im) if im is not None else None,
                                    w, h, ctypes.byref(opts), ctypes.c_void_p(tptr), ctypes.c_void_p(mptr), mcode,
                                    ctypes.c_void_p(st)))
    return FlowScore(table, batched, opts, mobj)


def score_frames(frames, truth, *, mask=None, ne_eps=1.0, divisor=None, out=None, stream=None):
    """``frames`` ((K, h, w) or (h, w); uint8, float32 or float64; any strides -- the output of
    interpolate, frames_device or reconstruct) against the grey frame ``truth``: per frame the pixel
    count, IE (utils.IE, RMS of 255 I - 255 T), the normalised interpolation error NE =
    sqrt(mean(d^2 / (|grad 255 T|^2 + ne_eps))) and max |d| (foto_score_frames_dev).  ``divisor``
    defaults to 255 for uint8 and 1 otherwise, for frames and truth each.  numpy arrays are uploaded
    first.  Returns a FrameScore (``out``: a float64 (K, 4) device array for the table)."""
    from . import _lib
    from . import device as D
    if isinstance(frames, np.ndarray):
        frames = D.DeviceArray.from_numpy(np.asarray(_host_image(frames, "frames")["keep"]))
    if isinstance(truth, np.ndarray):
        truth = D.DeviceArray.from_numpy(np.asarray(_host_image(truth, "truth")["keep"]))
    if isinstance(mask, np.ndarray):
        mask = D.DeviceArray.from_numpy(np.asarray(_host_image(mask, "mask")["keep"]))
    ptr, typestr, shape, strides, _ = D.device_interface(frames)
    if typestr not in D._DTYPES:
        raise ValueError(f"frames: typestr {typestr!r}; frames are uint8, float32 or float64")
    if len(shape) not in (2, 3):
        raise ValueError(f"frames of shape {shape}: (K, h, w) or (h, w)")
    batched = len(shape) == 3
    code, npdt = D._DTYPES[typestr]
    item = np.dtype(npdt).itemsize
    if strides is None:
        strides = D.packed_strides(shape, item)
    if any(int(s) % item for s in strides):
        raise ValueError(f"frames: byte strides {tuple(strides)} are not multiples of the {item}-byte item size")
    K = int(shape[0]) if batched else 1
    (h, w), (sy, sx) = shape[-2:], strides[-2:]
    srec = int(strides[0]) // item if batched and K > 1 else 1
    fr = D.make_image(ptr, code, int(sy) // item, int(sx) // item, divisor, (h, w), frames)
    tr = D.as_image(truth, divisor)
    if tr.shape != (h, w):
        raise ValueError(f"truth is {tr.shape[0]} x {tr.shape[1]} (h x w), the frames {h} x {w}")
    im = None
    if mask is not None:
        im = D.as_image(mask, 1.0)
        if im.shape != (h, w):
            raise ValueError(f"mask is {im.shape[0]} x {im.shape[1]} (h x w), the frames {h} x {w}")
    table, tptr, _ = D._shaped_target(out, "float64", {"float64": _lib.FOTO_F64}, (K, 4), "score tables")
    st = D.stream_handle(stream, frames, truth)
    check(lib().foto_score_frames_dev(ctypes.byref(fr), K, srec, ctypes.byref(tr),
                                      ctypes.byref(im) if im is not None else None, int(w), int(h), float(ne_eps),
                                      ctypes.c_void_p(tptr), ctypes.c_void_p(st)))
    return FrameScore(table, batched)
