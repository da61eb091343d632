"""numpy restatement of the flow algebra (include/foto.h, "flow algebra"), operation for operation
in the kernels' order (csrc/foto_chain.hip): the yardstick of tests/test_gpu_chain.py, compared to
the device and never the device to itself.  S is gn_pyr_ref.sample, sample_sum's order.

Flows are float64 (or float32, widened exactly) arrays with a record axis: planar (K, 3, h, w) =
u, v, m or interleaved (K, h, w, 2) = (u, v).  Results are float64; a float32 device output is
expected to equal ``ref.astype(np.float32)``.
"""
import numpy as np

from gn_pyr_ref import sample

ALPHA1, ALPHA2 = 0.01, 0.5
SHIFTS = [(2, 1), (-1, 3), (3, -2), (1, 1), (-2, 2)]     # the constant integer shifts of the exactness case
# w, h, K, seed of the cross-check cases (cons_case)
CONS = [(2, 2, 1, 11), (3, 2, 2, 12), (37, 29, 3, 13), (130, 18, 2, 14), (64, 48, 5, 15)]


def split(flow, layout):
    """(u, v, m or None), each (K, h, w) float64, of a flow with a record axis."""
    f = np.asarray(flow)
    assert f.ndim == 4 and f.dtype in (np.float32, np.float64), (f.shape, f.dtype)
    f = f.astype(np.float64)
    if layout == "planar":
        assert f.shape[1] == 3
        return f[:, 0], f[:, 1], f[:, 2]
    assert layout == "interleaved" and f.shape[3] == 2
    return f[..., 0], f[..., 1], None


def join(u, v, m, layout):
    """The flow buffer of planes (K, h, w): planar (m None: +0.0) or interleaved."""
    if layout == "planar":
        return np.stack([u, v, np.zeros_like(u) if m is None else m], axis=1)
    return np.stack([u, v], axis=-1)


def grid(h, w):
    jj, ii = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    return ii, jj


def S(f, x, y):
    h, w = f.shape
    return sample(f, w, h, x.ravel(), y.ravel()).reshape(h, w)


def compose(flow, layout="planar", out_layout=None, last_only=False):
    """C_0 = F_0, C_k = C_{k-1} + S(F_k; p + C_{k-1}); 1 + M_k = (1 + M_{k-1}) (1 + S(m_k; .))."""
    u, v, m = split(flow, layout)
    out_layout = layout if out_layout is None else out_layout
    K, h, w = u.shape
    x, y = grid(h, w)
    cu, cv = u[0].copy(), v[0].copy()
    M = None if m is None else m[0].copy()
    U, V, MM = [cu], [cv], [M]
    for k in range(1, K):
        px, py = x + cu, y + cv
        if M is not None:
            M = (1.0 + M) * (1.0 + S(m[k], px, py)) - 1.0
        su, sv = S(u[k], px, py), S(v[k], px, py)
        cu, cv = cu + su, cv + sv
        U.append(cu), V.append(cv), MM.append(M)
    if last_only:
        U, V, MM = U[-1:], V[-1:], MM[-1:]
    return join(np.stack(U), np.stack(V), None if m is None else np.stack(MM), out_layout)


def invert(flow, iters, layout="planar", out_layout=None):
    """B = 0, then B <- -S(F; p + B) ``iters`` times; m = +0.0."""
    u, v, _ = split(flow, layout)
    out_layout = layout if out_layout is None else out_layout
    K, h, w = u.shape
    x, y = grid(h, w)
    BU, BV = [], []
    for k in range(K):
        bu, bv = np.zeros((h, w)), np.zeros((h, w))
        for _ in range(iters):
            px, py = x + bu, y + bv
            bu, bv = -S(u[k], px, py), -S(v[k], px, py)
        BU.append(bu), BV.append(bv)
    return join(np.stack(BU), np.stack(BV), None, out_layout)


def consistency(fwd, bwd, layout="planar", bwd_layout=None, alpha1=ALPHA1, alpha2=ALPHA2):
    """(valid uint8 (K, h, w), table float64 (K, 4), err float64 (K, h, w), cls int (K, h, w),
    margin (K, h, w)): margin is |e - thr| / max(e, thr), the relative distance of a class 0 / 1
    pixel from the threshold (inf elsewhere)."""
    fu, fv, _ = split(fwd, layout)
    bu, bv, _ = split(bwd, layout if bwd_layout is None else bwd_layout)
    K, h, w = fu.shape
    assert bu.shape[0] in (1, K)
    x, y = grid(h, w)
    valid, table, err, cls, margin = [], [], [], [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            kb = k if bu.shape[0] == K else 0
            Fu, Fv = fu[k], fv[k]
            qx, qy = x + Fu, y + Fv
            Bu, Bv = S(bu[kb], qx, qy), S(bv[kb], qx, qy)
            du, dv = Fu + Bu, Fv + Bv
            e = du * du + dv * dv
            thr = alpha1 * ((Fu * Fu + Fv * Fv) + (Bu * Bu + Bv * Bv)) + alpha2
            c = np.zeros((h, w), np.int64)
            c[e > thr] = 1
            c[(qx < 0) | (qx > w - 1) | (qy < 0) | (qy > h - 1)] = 2
            c[~(np.isfinite(Fu) & np.isfinite(Fv) & np.isfinite(Bu) & np.isfinite(Bv))] = 3
            cls.append(c)
            valid.append((c == 0).astype(np.uint8))
            table.append([np.count_nonzero(c == q) for q in range(4)])
            err.append(np.where(c == 3, np.nan, np.sqrt(e)))
            margin.append(np.where(c <= 1, np.abs(e - thr) / np.maximum(e, thr), np.inf))
    return (np.stack(valid), np.array(table, dtype=np.float64), np.stack(err), np.stack(cls), np.stack(margin))


# ------------------------------------------------------------------ the test flows

def random_flow(K, h, w, layout, dtype, seed, sigma=2.0):
    """N(0, sigma^2) px displacements (many paths leave the frame and hit the clamp), m in N(0, 0.1^2)."""
    rng = np.random.default_rng(seed)
    u, v = sigma * rng.standard_normal((2, K, h, w))
    m = 0.1 * rng.standard_normal((K, h, w))
    return np.ascontiguousarray(join(u, v, m, layout).astype(dtype))


def shifts_flow(shifts, h, w, layout="planar", dtype=np.float64):
    """Record k: the constant integer shift shifts[k] = (du, dv)."""
    u = np.stack([np.full((h, w), float(s[0])) for s in shifts])
    v = np.stack([np.full((h, w), float(s[1])) for s in shifts])
    return np.ascontiguousarray(join(u, v, None, layout).astype(dtype))


def smooth_flow(h=48, w=64, layout="planar", dtype=np.float64):
    """u = 1.5 sin(x / 8) cos(y / 10), v = cos(x / 9) sin(y / 7): the Jacobian norm stays below 0.4."""
    x, y = grid(h, w)
    u = 1.5 * np.sin(x / 8) * np.cos(y / 10)
    v = np.cos(x / 9) * np.sin(y / 7)
    return np.ascontiguousarray(join(u[None], v[None], None, layout).astype(dtype))


def step_flow(h=48, w=64, layout="planar", dtype=np.float64):
    """Two regions shifted +3 / -3 px along x, split at the middle column: (forward, backward) with
    the backward flow of each region its negated shift."""
    u = np.where(np.arange(w)[None, :] < w // 2, 3.0, -3.0) * np.ones((h, 1))
    z = np.zeros((h, w))
    fwd = np.ascontiguousarray(join(u[None], z[None], None, layout).astype(dtype))
    bwd = np.ascontiguousarray(join(-u[None], z[None], None, layout).astype(dtype))
    return fwd, bwd


def cons_case(K, h, w, seed, layout="planar", dtype=np.float64, bwd_layout=None, bwd_dtype=None, bwd_records=None):
    """(forward, backward) for the cross-check with pixels in every class where the frame has room:
    a wavy forward flow of a few pixels (some targets leave the frame), its 8-round inverse plus
    N(0, 0.45^2) noise (consistent and inconsistent pixels on either side of alpha2 = 0.5), one inf
    in the forward and one NaN in the backward flow (not finite)."""
    rng = np.random.default_rng(seed)
    x, y = grid(h, w)
    k = np.arange(K, dtype=np.float64)[:, None, None]
    u = 2.5 * np.sin(x / 5 + k) * np.cos(y / 6)
    v = 2.0 * np.cos(x / 7) * np.sin(y / 4 + k)
    fwd = join(u, v, None, "planar")
    bwd = invert(fwd, 8)[:bwd_records]
    bwd[:, :2] += 0.45 * rng.standard_normal(bwd[:, :2].shape)
    fwd[0, 0, h // 2, w // 2] = np.inf
    bwd[0, 1, h - 1, 0] = np.nan
    fu, fv, _ = split(fwd, "planar")
    bu, bv, _ = split(bwd, "planar")
    return (np.ascontiguousarray(join(fu, fv, None, layout).astype(dtype)),
            np.ascontiguousarray(join(bu, bv, None, layout if bwd_layout is None else bwd_layout)
                                 .astype(dtype if bwd_dtype is None else bwd_dtype)))


def inversion_residual(flow, B, layout="planar"):
    """max |F(p + B) + B| over the pixels whose p + B stays inside the frame."""
    u, v, _ = split(flow, layout)
    bu, bv, _ = split(B, layout)
    K, h, w = u.shape
    x, y = grid(h, w)
    worst = 0.0
    for k in range(K):
        px, py = x + bu[k], y + bv[k]
        inside = (px >= 0) & (px <= w - 1) & (py >= 0) & (py <= h - 1)
        ru, rv = S(u[k], px, py) + bu[k], S(v[k], px, py) + bv[k]
        worst = max(worst, np.abs(ru[inside]).max(), np.abs(rv[inside]).max())
    return worst
