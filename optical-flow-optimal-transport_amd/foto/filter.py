"""Flow filtering (include/foto.h, "flow filtering"): the last stage of a classical flow pipeline on
flow buffers that stay on the device.

``median``  the edge-aware weighted median of Sun, Roth and Black (CVPR 2010), guided by an image
``fill``    the same operator with the rejected pixels at weight zero and the usable ones kept:
            holes -- what ``foto.chain.consistency`` marks invalid -- filled from their neighbours
``tables``  the two integer weight tables of a Gaussian spatial and range term, made on the host

A flow is what ``foto.chain`` takes: a C-contiguous float32 / float64 array, "planar" (3, h, w) or
(K, 3, h, w) = u, v, m, or "interleaved" (h, w, 2) or (K, h, w, 2) = (u, v).  Device arrays
(``DeviceArray``, torch tensors, anything with ``__cuda_array_interface__``) stay on the device and
nothing waits; numpy arrays are uploaded and the results downloaded.
"""
import ctypes

import numpy as np

from . import _lib
from . import device as D
from ._lib import check, lib
from .chain import _F64, _flow_target
from .render import _host_flow, flow_arg, source_arg

MAX_RADIUS, MAX_ROUNDS, MAX_RANGE = _lib.FOTO_MEDIAN_MAX_RADIUS, _lib.FOTO_MEDIAN_MAX_ROUNDS, _lib.FOTO_MEDIAN_MAX_RANGE
FILL_ROUNDS = 8
COUNTS = ("usable", "filled", "unfilled")   # the first three columns of the table


def _radius(radius):
    if int(radius) != radius or not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"radius = {radius!r} is outside [1, {MAX_RADIUS}]")
    return int(radius)


def tables(radius, sigma_s=None, sigma_r=None, levels=256, scale=255.0, unit=1024):
    """(spatial, range) as uint16 for ``median``: spatial[dy + R][dx + R] = round(unit exp(-(dx^2 +
    dy^2) / (2 sigma_s^2))), range[k] = round(unit exp(-(k / scale)^2 / (2 sigma_r^2))) for k <
    ``levels`` -- entry k serves the guide differences that ``range_scale = scale`` rounds to k, so
    sigma_r is in the guide's units (a uint8 guide has values in [0, 1]).  ``None`` for a sigma: all
    ones, (2R + 1, 2R + 1), or no range term, one entry.  Both centres are at least 1.  Computed by
    numpy on the host: the device never evaluates exp."""
    R = _radius(radius)
    if not 1 <= unit <= 65535:
        raise ValueError(f"unit = {unit!r} is outside [1, 65535]")

    def gauss(d2, sigma):
        if not (np.isfinite(sigma) and sigma > 0):
            raise ValueError(f"sigma = {sigma!r} must be finite and > 0")
        return np.clip(np.round(unit * np.exp(-d2 / (2.0 * float(sigma) ** 2))), 0, 65535).astype(np.uint16)

    if sigma_s is None:
        spatial = np.ones((2 * R + 1, 2 * R + 1), np.uint16)
    else:
        d = np.arange(-R, R + 1, dtype=np.float64)
        spatial = gauss(d[:, None] ** 2 + d[None, :] ** 2, sigma_s)
    if sigma_r is None:
        rng = np.ones(1, np.uint16)
    else:
        if int(levels) != levels or not 1 <= levels <= MAX_RANGE:
            raise ValueError(f"levels = {levels!r} is outside [1, {MAX_RANGE}]")
        if not (np.isfinite(scale) and scale > 0):
            raise ValueError(f"scale = {scale!r} must be finite and > 0")
        rng = gauss((np.arange(int(levels), dtype=np.float64) / float(scale)) ** 2, sigma_r)
    spatial[R, R] = max(int(spatial[R, R]), 1)
    rng[0] = max(int(rng[0]), 1)
    return spatial, rng


def median_opts(radius=2, rounds=1, fill_only=False, spatial=None, range=None, range_scale=255.0):
    """The _lib.MedianOpts of a call; ValueError for what foto_filter_check would reject."""
    R = _radius(radius)
    if int(rounds) != rounds or not 1 <= rounds <= MAX_ROUNDS:
        raise ValueError(f"rounds = {rounds!r} is outside [1, {MAX_ROUNDS}]")
    if not (np.isfinite(range_scale) and range_scale > 0):
        raise ValueError(f"range_scale = {range_scale!r} must be finite and > 0")
    side = 2 * R + 1
    sp = np.ones((side, side), np.uint16) if spatial is None else np.asarray(spatial)
    rg = np.ones(1, np.uint16) if range is None else np.asarray(range)
    if sp.shape != (side, side):
        raise ValueError(f"spatial of shape {sp.shape}: radius {R} takes ({side}, {side})")
    if rg.ndim != 1 or not 1 <= rg.size <= MAX_RANGE:
        raise ValueError(f"range of shape {rg.shape}: 1 .. {MAX_RANGE} entries")
    for name, a in (("spatial", sp), ("range", rg)):
        if a.dtype.kind not in "iu" or a.min() < 0 or a.max() > 65535:
            raise ValueError(f"{name}: integer weights in [0, 65535] (uint16)")
    if sp[R, R] == 0 or rg[0] == 0:
        raise ValueError("the centre weight spatial[R][R] and range[0] must be > 0")
    o = _lib.MedianOpts()
    o.radius, o.rounds, o.fill_only, o.n_range, o.range_scale = R, int(rounds), 1 if fill_only else 0, rg.size, float(range_scale)
    flat = sp.astype(np.uint16).ravel()
    o.spatial[:flat.size] = flat.tolist()
    o.range[:rg.size] = rg.astype(np.uint16).tolist()
    return o


def _host_image(a):
    a = np.asarray(a)
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    if a.dtype not in (np.uint8, np.float32, np.float64):
        a = a.astype(np.float64)
    return D.DeviceArray.from_numpy(np.ascontiguousarray(a))


def _guide_arg(guide, host, h, w):
    if isinstance(guide, _lib.Image):
        if not hasattr(guide, "shape"):
            raise TypeError("guide: a foto_image made by foto.device.as_image (it carries the frame's shape), or an array")
        im, C, sc = guide, 1, 1
    else:
        if isinstance(guide, np.ndarray):
            if not host:
                raise TypeError("guide: a device array for a device flow (numpy arrays go with a numpy flow)")
            guide = _host_image(guide)
        im, C, sc, _ = source_arg(guide, channels_last=True)
    if im.shape != (h, w):
        raise ValueError(f"guide is {im.shape[0]} x {im.shape[1]} (h x w), the flow {h} x {w}")
    return im, C, sc


def _mask_arg(mask, host, h, w):
    if isinstance(mask, np.ndarray):
        if not host:
            raise TypeError("mask: a device array for a device flow (numpy arrays go with a numpy flow)")
        mask = _host_image(mask)
    if isinstance(mask, _lib.Image) and not hasattr(mask, "shape"):
        raise TypeError("mask: a foto_image made by foto.device.as_image (it carries the frame's shape), or an array")
    im = D.as_image(mask, divisor=1.0)
    if im.shape != (h, w):
        raise ValueError(f"mask is {im.shape[0]} x {im.shape[1]} (h x w), the flow {h} x {w}")
    return im


def median(flow, *, in_layout="planar", guide=None, mask=None, radius=2, rounds=1, fill_only=False, spatial=None,
           range=None, range_scale=255.0, dtype=None, layout=None, out=None, valid_out=None, table_out=None,
           stream=None):
    """The weighted median of every record of ``flow`` over (2 radius + 1)^2 windows truncated at the
    border, ``rounds`` times (foto_flow_median_dev).  A neighbour's weight is ``spatial[dy + R][dx +
    R] * range[k]``, k the guide difference max_c |I_c(q) - I_c(p)| times ``range_scale``, rounded and
    capped at the last entry -- ``tables`` makes both; None: all ones -- and 0 where the neighbour is
    not usable: not finite, or ``mask`` zero there.  The result is the lower weighted median, one of
    the samples, for u and v separately; a pixel with no usable neighbour stays as it is, unfilled.
    ``fill_only`` leaves the usable pixels as they are.  ``guide``: (h, w) or (h, w, C), uint8 (values
    / 255) or float; ``mask``: (h, w), non-zero = usable -- ``foto.chain.consistency``'s ``valid``.
    Returns (flow, valid, table): the flow in ``dtype`` / ``layout`` (None: the input's; the m plane
    of a planar result is the input's), ``valid`` uint8 ([K,] h, w) = usable after the last round,
    ``table`` float64 ([K,] 4) = the counts in COUNTS' order and 0.  ``out`` / ``valid_out`` /
    ``table_out``: device arrays for the three."""
    host = isinstance(flow, np.ndarray)
    if host:
        if out is not None or valid_out is not None or table_out is not None:
            raise ValueError("out / valid_out / table_out: device arrays for device input; numpy input returns numpy arrays")
        flow = _host_flow(flow)
    o = median_opts(radius, rounds, fill_only, spatial, range, range_scale)
    fl, K, h, w, batched = flow_arg(flow, in_layout)
    gim, C, sc = (None, 0, 0) if guide is None else _guide_arg(guide, host, h, w)
    mim = None if mask is None else _mask_arg(mask, host, h, w)
    lead = (K,) if batched else ()
    def targets(given):   # the caller's arrays are checked before anything is allocated
        v = D._shaped_target(valid_out, "uint8", {"uint8": _lib.FOTO_U8}, lead + (h, w), "masks") \
            if (valid_out is not None) == given else None
        t = D._shaped_target(table_out, "float64", _F64, lead + (4,), "counts") \
            if (table_out is not None) == given else None
        return v, t

    v0, t0 = targets(True)
    out, ptr, code, lcode = _flow_target(fl, in_layout, dtype, layout, lead, h, w, out)
    v1, t1 = targets(False)
    (valid, vptr, _), (table, tptr, _) = v0 or v1, t0 or t1
    objs = [x for x in (flow, guide, mask) if x is not None and not isinstance(x, (_lib.Image, np.ndarray))]
    check(lib().foto_flow_median_dev(ctypes.byref(fl), None if gim is None else ctypes.byref(gim), C, sc,
                                     None if mim is None else ctypes.byref(mim), w, h, ctypes.byref(o),
                                     ctypes.c_void_p(ptr), code, lcode, ctypes.c_void_p(vptr), ctypes.c_void_p(tptr),
                                     ctypes.c_void_p(D.stream_handle(stream, *objs))))
    res = (out, valid, table)
    return tuple(x.to_numpy() for x in res) if host else res


def fill(flow, valid, *, rounds=FILL_ROUNDS, **kw):
    """``median(flow, mask=valid, fill_only=True, rounds=rounds, ...)``: the pixels ``valid`` rejects
    (and the non-finite ones) are replaced by the weighted median of their usable neighbours, round
    after round from the rim of a hole inwards -- a hole of half-width d needs about d / radius
    rounds; what is still unfilled is counted in the table.  The usable pixels keep their bits."""
    if "mask" in kw or "fill_only" in kw:
        raise TypeError("fill: the mask is `valid` and fill_only is implied")
    return median(flow, mask=valid, fill_only=True, rounds=rounds, **kw)
