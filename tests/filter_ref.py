"""The numpy restatement of the flow filter (include/foto.h, "flow filtering"), literally: per pixel
the truncated window, the integer weights, the candidates ordered by the monotone 64-bit key, and
the smallest key of a usable candidate whose cumulative weight reaches half the total.  Plain loops
over the pixels; the sizes are tiny.  The selected value is one of the samples and the weights are
integers (numpy uint64 sums, exact), so the device has to give the same bits."""
import numpy as np

TOP = np.uint64(1) << np.uint64(63)


def keys(x):
    """key = bits ^ (sign ? ~0 : 1 << 63) of float64 values: ordered as the values, -0.0 < +0.0."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b ^ TOP)


def split(flow, layout):
    """(u, v, m or None) as float64 [K][h][w] of a flow with a record axis."""
    f = np.asarray(flow)
    if layout == "planar":
        return f[:, 0].astype(np.float64), f[:, 1].astype(np.float64), f[:, 2]
    return f[..., 0].astype(np.float64), f[..., 1].astype(np.float64), None


def guide_values(guide, divisor=None):
    """float64 (h, w, C) = (double)pixel / divisor; the divisor defaults to 255 for uint8 and 1 otherwise."""
    g = np.asarray(guide)
    if divisor is None:
        divisor = 255.0 if g.dtype == np.uint8 else 1.0
    g = g.astype(np.float64)
    if g.ndim == 2:
        g = g[:, :, None]
    return g if divisor == 1.0 else g / divisor


def weighted_median(vals, wt, usable, T, shuffle=None):
    """The lower weighted median of the window's candidates: the value of the smallest key k among the
    usable ones with 2 * sum(wt[key <= k]) >= T.  ``shuffle``: a Generator that permutes the window
    order first (the result may not depend on it)."""
    if shuffle is not None:
        p = shuffle.permutation(vals.size)
        vals, wt, usable = vals[p], wt[p], usable[p]
    k = keys(vals)
    order = np.argsort(k, kind="stable")
    ks, cs = k[order], np.cumsum(wt[order], dtype=np.uint64)
    cum = cs[np.searchsorted(ks, k, side="right") - 1]          # per candidate: the weight of the keys <= its own
    ok = usable & (np.uint64(2) * cum >= np.uint64(T))
    assert ok.any()
    a = np.flatnonzero(ok)[np.argmin(k[ok])]
    return vals[a]


def one_round(u, v, V, G, R, spatial, rng, range_scale, fill_only, shuffle=None):
    h, w = u.shape
    nr = rng.size
    nu, nv, nV = u.copy(), v.copy(), V.copy()
    for j in range(h):
        for i in range(w):
            if fill_only and V[j, i]:
                continue
            y0, y1, x0, x1 = max(0, j - R), min(h, j + R + 1), max(0, i - R), min(w, i + R + 1)
            us = V[y0:y1, x0:x1].ravel()
            sp = spatial[y0 - j + R:y1 - j + R, x0 - i + R:x1 - i + R].ravel().astype(np.uint64)
            if G is None:
                gw = np.ones(us.size, np.uint64)
            else:
                with np.errstate(invalid="ignore"):
                    d = np.abs(G[y0:y1, x0:x1, :] - G[j, i, :]).reshape(us.size, -1)
                bad = np.isnan(d).any(axis=1)
                dmax = np.where(np.isnan(d), 0.0, d).max(axis=1)
                with np.errstate(invalid="ignore", over="ignore"):
                    t = np.floor(dmax * range_scale + 0.5)
                top = bad | ~(t < nr - 1)
                gw = rng[np.where(top, nr - 1, np.where(top, 0.0, t)).astype(np.int64)].astype(np.uint64)
            wt = np.where(us, sp * gw, np.uint64(0)).astype(np.uint64)
            assert wt.max() < 2 ** 32                              # the weight is a uint32
            T = int(wt.sum(dtype=np.uint64))
            if T == 0:
                continue                                           # unfilled: keeps its value, stays outside V
            nu[j, i] = weighted_median(u[y0:y1, x0:x1].ravel(), wt, us, T, shuffle)
            nv[j, i] = weighted_median(v[y0:y1, x0:x1].ravel(), wt, us, T, shuffle)
            nV[j, i] = True
    return nu, nv, nV


def median(flow, layout="planar", guide=None, divisor=None, mask=None, radius=2, rounds=1, fill_only=False,
           spatial=None, rng=None, range_scale=255.0, out_dtype=None, out_layout=None, shuffle=None):
    """(out, valid uint8 [K][h][w], table float64 [K][4]) of a flow WITH a record axis: (K, 3, h, w)
    planar or (K, h, w, 2) interleaved.  ``guide`` (h, w) or (h, w, C), ``mask`` (h, w)."""
    flow = np.asarray(flow)
    R = int(radius)
    u, v, m = split(flow, layout)
    K, h, w = u.shape
    spatial = np.ones((2 * R + 1, 2 * R + 1), np.uint16) if spatial is None else np.asarray(spatial, np.uint16)
    rng = np.ones(1, np.uint16) if rng is None else np.asarray(rng, np.uint16)
    assert spatial.shape == (2 * R + 1, 2 * R + 1) and spatial[R, R] > 0 and rng[0] > 0
    G = None if guide is None else guide_values(guide, divisor)
    out_dtype = flow.dtype if out_dtype is None else np.dtype(out_dtype)
    out_layout = layout if out_layout is None else out_layout
    out = np.zeros((K, 3, h, w) if out_layout == "planar" else (K, h, w, 2), out_dtype)
    valid = np.zeros((K, h, w), np.uint8)
    table = np.zeros((K, 4))
    for k in range(K):
        V0 = np.isfinite(u[k]) & np.isfinite(v[k])
        if mask is not None:
            V0 &= np.asarray(mask) != 0
        fu, fv, V = u[k], v[k], V0
        for _ in range(int(rounds)):
            fu, fv, V = one_round(fu, fv, V, G, R, spatial, rng, float(range_scale), fill_only, shuffle)
        with np.errstate(over="ignore", invalid="ignore"):
            if out_layout == "planar":
                out[k, 0], out[k, 1] = fu.astype(out_dtype), fv.astype(out_dtype)
                if m is not None:
                    out[k, 2] = m[k].astype(out_dtype)
            else:
                out[k, ..., 0], out[k, ..., 1] = fu.astype(out_dtype), fv.astype(out_dtype)
        valid[k] = V
        table[k] = [V0.sum(), (~V0 & V).sum(), (~V).sum(), 0]
    return out, valid, table


def random_flow(K, h, w, layout, dtype, seed, scale=3.0):
    rng = np.random.default_rng(seed)
    f = rng.uniform(-scale, scale, (K, 3, h, w))
    f[:, 2] *= 0.1
    if layout == "interleaved":
        f = np.ascontiguousarray(np.moveaxis(f[:, :2], 1, -1))
    return f.astype(dtype)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    np.testing.assert_array_equal(bits(got), bits(want))
