"""Device-buffer interface on the GPU (include/foto.h, *_dev; foto/device.py): frames that are
already in device memory go in, the flow stays on the device.

Every comparison is against the host entry of this same build fed the values the descriptor
stands for, np.float64(pixel) / divisor, and is bit for bit (np.array_equal on the uint64 view):
the device entries share everything but the two uploads and the export with the host entries.
The one inexact quantity is the frame sum of normalize = 1, a fixed-order reduction in another
order than math.fsum: |S_dev - fsum(f)| <= n 2^-53 fsum(f) bounds any summation order of n
non-negative terms.  Device memory comes from foto.device.DeviceArray (foto_dev_malloc), so
only the torch test needs torch.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import PKG, REPO  # noqa: E402  (puts the package on sys.path)

from foto import _lib, evaluate, gn  # noqa: E402
from foto import device as D  # noqa: E402
from foto.bb import BBSolver  # noqa: E402
from foto.device import DeviceArray  # noqa: E402
from foto.synthetic import sinusoid_pair, textured_pair  # noqa: E402

ITS = 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def frames(w, h, seed=0):
    """(f0, f1) of textured_pair as (h, w) float64 arrays"""
    a, b = textured_pair(w, h, seed=seed)
    return a.reshape(h, w), b.reshape(h, w)


def run(s):
    s.iterate(ITS, stop_rules=False)
    return dict(crit=np.array(s.crit), cg=np.array(s.cg_its))


def host_solve(f0, f1, Nt, **opts):
    h, w = f0.shape
    with BBSolver(f0.ravel(), f1.ravel(), Nt, w, h, **opts) as s:
        r = run(s)
        r["u"], r["v"], r["m"] = s.flow()
    return r


def dev_solve(d0, d1, Nt, **opts):
    with BBSolver.from_device(d0, d1, Nt, **opts) as s:
        r = run(s)
        uvm = s.flow_device(dtype="float64", layout="planar").to_numpy()
        r["sums"] = s.sums
    r["u"], r["v"], r["m"] = (uvm[k].ravel() for k in range(3))
    return r


def assert_same_solve(got, ref):
    for k in ("u", "v", "m", "crit"):
        assert same(got[k], ref[k]), k
    assert np.array_equal(got["cg"], ref["cg"])


_host_cache = {}


def host_ref(w, h, Nt, seed=0, **opts):
    key = (w, h, Nt, seed, tuple(sorted(opts.items())))
    if key not in _host_cache:
        _host_cache[key] = host_solve(*frames(w, h, seed), Nt, **opts)
    return _host_cache[key]


# ------------------------------------------------------------------ 1. BB, float64 contiguous

@pytest.mark.parametrize("Nx,Ny,Nt,opts", [
    (37, 29, 5, dict(cg_mode=-1)),                      # auto: the stencil CG
    (40, 30, 6, dict(cg_mode=3)),                       # Gauss CG, two iterations in flight
    (40, 30, 6, dict(cg_mode=3, virtual_ranks=2)),      # two in-process shards: each gets its copy
])
def test_bb_float64_contiguous(Nx, Ny, Nt, opts):
    f0, f1 = frames(Nx, Ny)
    got = dev_solve(DeviceArray.from_numpy(f0), DeviceArray.from_numpy(f1), Nt, **opts)
    assert_same_solve(got, host_ref(Nx, Ny, Nt, **opts))
    assert got["sums"] == (1.0, 1.0)


# ------------------------------------------------------------------ 2. ingest variants

def _padded(f, pitch):
    buf = np.zeros((f.shape[0], pitch))
    buf[:, :f.shape[1]] = f
    return DeviceArray.from_numpy(buf)[:, :f.shape[1]]


def _channel(f, c=1):
    buf = np.full(f.shape + (3,), 7.0)
    buf[..., c] = f
    return DeviceArray.from_numpy(buf)[:, :, c]


def _transposed(f):
    return DeviceArray.from_numpy(np.ascontiguousarray(f.T)).T


def _offset(f):
    buf = np.zeros(f.size + 1)
    buf[1:] = f.ravel()
    d = DeviceArray.from_numpy(buf)[1:].reshape(f.shape)
    assert d.ptr % 16 == 8
    return d


VIEWS = {"row-padded (pitch 41)": lambda f: _padded(f, 41), "channel of [H][W][3]": _channel,
         "transposed": _transposed, "8- but not 16-byte aligned": _offset}


@pytest.mark.parametrize("view", list(VIEWS))
def test_ingest_float64_views(view):
    w, h, Nt = 37, 29, 5
    f0, f1 = frames(w, h)
    d0, d1 = VIEWS[view](f0), VIEWS[view](f1)
    assert d0.shape == (h, w) and np.array_equal(d0.to_numpy(), f0)
    assert_same_solve(dev_solve(d0, d1, Nt, cg_mode=-1), host_ref(w, h, Nt, cg_mode=-1))


def test_ingest_uint8():
    w, h, Nt = 37, 29, 5
    f0, f1 = frames(w, h)
    i0, i1 = (np.round(f * 255).astype(np.uint8) for f in (f0, f1))
    ref = host_solve(i0.astype(np.float64) / 255, i1.astype(np.float64) / 255, Nt, cg_mode=-1)
    assert_same_solve(dev_solve(DeviceArray.from_numpy(i0), DeviceArray.from_numpy(i1), Nt, cg_mode=-1), ref)
    # and through the scalar path: a row-padded view (pitch 41 is no multiple of 16)
    assert_same_solve(dev_solve(_pad_u8(i0), _pad_u8(i1), Nt, cg_mode=-1), ref)


def _pad_u8(i):
    buf = np.zeros((i.shape[0], 41), dtype=np.uint8)
    buf[:, :i.shape[1]] = i
    return DeviceArray.from_numpy(buf)[:, :i.shape[1]]


def test_ingest_float32():
    w, h, Nt = 37, 29, 5
    g0, g1 = (f.astype(np.float32) for f in frames(w, h))
    ref = host_solve(np.float64(g0) / 1.0, np.float64(g1) / 1.0, Nt, cg_mode=-1)
    assert_same_solve(dev_solve(DeviceArray.from_numpy(g0), DeviceArray.from_numpy(g1), Nt, cg_mode=-1), ref)


def test_ingest_2x2():
    f0, f1 = frames(2, 2)
    assert_same_solve(dev_solve(DeviceArray.from_numpy(f0), DeviceArray.from_numpy(f1), 5, cg_mode=-1),
                      host_solve(f0, f1, 5, cg_mode=-1))


def test_ingest_vector_path_with_tail():
    """Rows whose starts are all 16-byte aligned (pitch 48) with a width that is no multiple of
    the 16 / 4 / 2 pixels of one load: full chunks by the vector path, the row tail pixel by
    pixel."""
    w, h, Nt = 37, 29, 5
    f0, f1 = frames(w, h)
    for dt, div in ((np.uint8, 255.0), (np.float32, 1.0), (np.float64, 1.0)):
        g0, g1 = ((np.round(f * 255) if dt == np.uint8 else f).astype(dt) for f in (f0, f1))
        ref = host_solve(g0.astype(np.float64) / div, g1.astype(np.float64) / div, Nt, cg_mode=-1)

        def pad(g):
            buf = np.zeros((h, 48), dtype=dt)
            buf[:, :w] = g
            return DeviceArray.from_numpy(buf)[:, :w]
        assert_same_solve(dev_solve(pad(g0), pad(g1), Nt, cg_mode=-1), ref)


# ------------------------------------------------------------------ 3. normalize

def test_normalize():
    w, h, Nt = 37, 29, 5
    f0, f1 = frames(w, h)
    got = dev_solve(DeviceArray.from_numpy(f0), DeviceArray.from_numpy(f1), Nt, cg_mode=-1, normalize=True)
    n = w * h
    for S, f in zip(got["sums"], (f0, f1)):
        exact = math.fsum(f.ravel())
        err = abs(S - exact)
        print(f"sum: device {S!r}, fsum {exact!r}, |diff| {err:.3e}, bound {n * 2.0 ** -53 * exact:.3e}")
        assert err <= n * 2.0 ** -53 * exact
    ref = host_solve(f0 / got["sums"][0], f1 / got["sums"][1], Nt, cg_mode=-1)
    assert_same_solve(got, ref)


# ------------------------------------------------------------------ 4. export

def test_export_layouts(tmp_path):
    import utils   # the drop-in utils.saveFlo
    w, h, Nt = 37, 29, 5
    f0, f1 = frames(w, h)
    ref = host_ref(w, h, Nt, cg_mode=-1)
    with BBSolver.from_device(DeviceArray.from_numpy(f0), DeviceArray.from_numpy(f1), Nt, cg_mode=-1) as s:
        run(s)
        p32 = s.flow_device(dtype="float32", layout="planar")
        i32 = s.flow_device(dtype="float32", layout="interleaved")
        i64 = s.flow_device(dtype="float64", layout="interleaved")
        mine = DeviceArray((3, h, w), np.float32)          # a caller-owned target
        assert s.flow_device(out=mine, dtype="float32") is mine
    assert p32.shape == (3, h, w) and p32.dtype == np.float32 and i32.shape == (h, w, 2)
    host = np.stack([ref["u"], ref["v"], ref["m"]]).reshape(3, h, w)
    assert np.array_equal(p32.to_numpy().view(np.uint32), host.astype(np.float32).view(np.uint32))
    assert np.array_equal(mine.to_numpy().view(np.uint32), host.astype(np.float32).view(np.uint32))
    path = str(tmp_path / "ref.flo")
    utils.saveFlo(w, h, ref["u"], ref["v"], path)
    payload = open(path, "rb").read()[12:]
    assert i32.to_numpy().tobytes() == payload
    assert same(i64.to_numpy()[..., 0].ravel(), ref["u"]) and same(i64.to_numpy()[..., 1].ravel(), ref["v"])


# ------------------------------------------------------------------ 5. reset_device

@pytest.mark.parametrize("opts", [dict(cg_mode=-1), dict(cg_mode=3)])
def test_reset_device(opts):
    w, h, Nt = 40, 30, 6
    a0, a1 = frames(w, h, seed=0)
    b0, b1 = frames(w, h, seed=5)
    ref_a, ref_b = host_ref(w, h, Nt, seed=0, **opts), host_ref(w, h, Nt, seed=5, **opts)

    def flow64(s):
        uvm = s.flow_device(dtype="float64").to_numpy()
        return {"u": uvm[0].ravel(), "v": uvm[1].ravel(), "m": uvm[2].ravel()}
    with BBSolver.from_device(DeviceArray.from_numpy(a0), DeviceArray.from_numpy(a1), Nt, **opts) as s:
        s.iterate(ITS + 2, stop_rules=False)              # state to forget
        s.reset_device(DeviceArray.from_numpy(b0), DeviceArray.from_numpy(b1))
        got = run(s)
        got.update(flow64(s))
        assert_same_solve(got, ref_b)
        s.reset(a0.ravel(), a1.ravel())                   # and a host reset on the same context
        got = run(s)
        got["u"], got["v"], got["m"] = s.flow()
        assert_same_solve(got, ref_a)


# ------------------------------------------------------------------ 6. GN

def _gn_inputs(w, h, kind):
    pairs = [sinusoid_pair(w, h), textured_pair(w, h, seed=3)]
    out = []
    for f1, f2 in pairs:
        f1, f2 = f1.reshape(h, w), f2.reshape(h, w)
        if kind == "uint8":
            i1, i2 = (np.round(f * 255).astype(np.uint8) for f in (f1, f2))
            out.append(((i1.astype(np.float64) / 255, i2.astype(np.float64) / 255),
                        (DeviceArray.from_numpy(i1), DeviceArray.from_numpy(i2))))
        else:   # a strided float32 view: every other column of a padded buffer
            g1, g2 = f1.astype(np.float32), f2.astype(np.float32)

            def view(g):
                buf = np.zeros((h, 2 * w + 3), dtype=np.float32)
                buf[:, 1:2 * w:2] = g
                return DeviceArray.from_numpy(buf)[:, 1:2 * w:2]
            out.append(((np.float64(g1), np.float64(g2)), (view(g1), view(g2))))
    return out


@pytest.mark.parametrize("w,h", [(40, 30), (33, 21)])
@pytest.mark.parametrize("kind", ["uint8", "float32-strided"])
def test_gn_solve_device(w, h, kind):
    alpha, lam = 0.1, 0.2
    cases = _gn_inputs(w, h, kind)
    with gn.Plan(w, h, alpha, lam) as PH, gn.Plan(w, h, alpha, lam) as PD:   # each a fresh plan
        for (h1, h2), (d1, d2) in cases:   # the second, different pair on the same plans
            assert d1.shape == (h, w)
            u, v, m, info, its = PH.solve(h1.ravel(), h2.ravel())
            out, dinfo, dits = PD.solve_device(d1, d2, dtype="float64")
            got = out.to_numpy()
            assert (dinfo, dits) == (info, its) and info == 0
            for k, ref in enumerate((u, v, m)):
                assert same(got[k].ravel(), ref), "uvm"[k]
            assert PD.timing()["iterations"] == its


# ------------------------------------------------------------------ 7. evaluation

def test_evaluation_device():
    w, h = 37, 29
    n = w * h
    rng = np.random.default_rng(11)
    f1 = textured_pair(w, h)[0]
    u, v = rng.normal(0, 1.5, n), rng.normal(0, 1.5, n)
    m = rng.normal(0, 0.1, n)
    uG, vG = u + rng.normal(0, 0.3, n), v + rng.normal(0, 0.3, n)
    u[5] = 80.0            # an endpoint error > 50: ignored by EE
    uG[17] = np.nan        # a NaN angular error: ignored by AE
    I, IG = textured_pair(w, h, seed=2)
    dev = {k: DeviceArray.from_numpy(x) for k, x in dict(f1=f1, u=u, v=v, m=m, uG=uG, vG=vG, I=I, IG=IG).items()}
    for mm, dm in ((m, dev["m"]), (None, None)):
        ref = evaluate.warp(f1, u, v, w, h, mm)
        got = evaluate.warp_device(dev["f1"], dev["u"], dev["v"], w, h, dm)
        assert got.shape == (h, w) and same(got.to_numpy().ravel(), ref)
    ref = evaluate.flow_errors(u, v, uG, vG, w, h)
    got = evaluate.flow_errors_device(dev["u"], dev["v"], dev["uG"], dev["vG"], w, h)
    assert all(math.isfinite(x) for x in ref)
    assert same(np.array(got), np.array(ref))
    assert same(np.array([evaluate.intensity_error_device(dev["I"], dev["IG"], w, h)]),
                np.array([evaluate.intensity_error(I, IG, w, h)]))


# ------------------------------------------------------------------ 8. argument errors

def test_argument_errors_leave_context_usable():
    w, h, Nt = 37, 29, 5
    f0, f1 = frames(w, h)
    d0, d1 = DeviceArray.from_numpy(f0), DeviceArray.from_numpy(f1)
    L = _lib.lib()
    import ctypes
    with BBSolver.from_device(d0, d1, Nt, cg_mode=-1) as s:
        out = DeviceArray((3, h, w), np.float64)
        # flow before any iteration
        assert L.foto_bb_flow_dev(s._ctx, ctypes.c_void_p(out.ptr), _lib.FOTO_F64, 0, None) == _lib.FOTO_ERR_STATE
        run(s)
        # a descriptor of the wrong size: 29 x 37 frames for a 37 x 29 context
        with pytest.raises(ValueError):
            s.reset_device(d0.T, d1.T)
        small = DeviceArray.from_numpy(f0[:-1])        # h - 1 rows: the last row would be out of bounds
        ims = D.as_image(small)
        assert L.foto_bb_reset_dev(s._ctx, ctypes.byref(ims), ctypes.byref(ims), 0, None, None) == _lib.FOTO_ERR_ARG
        bad = D.as_image(d0)
        bad.dtype = 7
        good = D.as_image(d1)
        assert L.foto_bb_reset_dev(s._ctx, ctypes.byref(bad), ctypes.byref(good), 0, None, None) == _lib.FOTO_ERR_ARG
        assert L.foto_bb_reset_dev(s._ctx, ctypes.byref(good), ctypes.byref(bad), 0, None, None) == _lib.FOTO_ERR_ARG
        # an output dtype of FOTO_U8
        assert L.foto_bb_flow_dev(s._ctx, ctypes.c_void_p(out.ptr), _lib.FOTO_U8, 0, None) == _lib.FOTO_ERR_ARG
        assert L.foto_bb_flow_dev(s._ctx, ctypes.c_void_p(out.ptr), _lib.FOTO_F64, 2, None) == _lib.FOTO_ERR_ARG
        # the context is as it was: the flow of the three iterations, then a good reset and solve
        ref = host_ref(w, h, Nt, cg_mode=-1)
        uvm = s.flow_device(out=out, dtype="float64").to_numpy()
        assert same(uvm[0].ravel(), ref["u"]) and same(uvm[2].ravel(), ref["m"])
        s.reset_device(d0, d1)
        got = run(s)
        uvm = s.flow_device(dtype="float64").to_numpy()
        got["u"], got["v"], got["m"] = (uvm[k].ravel() for k in range(3))
        assert_same_solve(got, ref)
    with gn.Plan(w, h, 0.1, 0.2) as P:
        g0, g1 = D.as_image(d0), D.as_image(d1)
        o64 = DeviceArray((3, h, w), np.float64)
        its = ctypes.c_int(0)
        args = (ctypes.c_void_p(o64.ptr), _lib.FOTO_U8, 0, None, ctypes.byref(its))
        assert L.foto_gn_plan_solve_dev(P._p, ctypes.byref(g0), ctypes.byref(g1), *args) == _lib.FOTO_ERR_ARG
        assert L.foto_gn_plan_solve_dev(P._p, ctypes.byref(bad), ctypes.byref(g1), ctypes.c_void_p(o64.ptr),
                                        _lib.FOTO_F64, 0, None, ctypes.byref(its)) == _lib.FOTO_ERR_ARG
        u, v, m, info, n_its = gn.solve(f0.ravel(), f1.ravel(), w, h, 0.1, 0.2)
        out, dinfo, dits = P.solve_device(d0, d1, out=o64, dtype="float64")
        assert (dinfo, dits) == (info, n_its) and same(out.to_numpy()[0].ravel(), u)


# ------------------------------------------------------------------ 9. torch as producer

_TORCH_CHILD = r"""
import sys
sys.path[:0] = [{repo!r}, {pkg!r}]
import torch                      # first: libfoto then binds to torch's HIP runtime
import numpy as np
from foto import bb, gn, device
from foto.synthetic import textured_pair

w, h, Nt = 37, 29, 5
f0, f1 = (np.round(f.reshape(h, w) * 255).astype(np.uint8) for f in textured_pair(w, h))
r0, r1 = f0.astype(np.float64) / 255, f1.astype(np.float64) / 255
kw = dict(r=1.0, convergence_tol=0.0, reg_epsilon=1e-3, max_it=4)
ref = bb.solve(r0.ravel(), r1.ravel(), Nt, w, h, log=lambda s: None, **kw)
gref = gn.cached_plan(w, h, 0.1, 0.2).solve(r0.ravel(), r1.ravel())
assert len(device.runtime_check()) == 1

def same(t, ref):
    got = t.cpu().numpy()
    return all(np.array_equal(got[k].ravel().view(np.uint64), ref[k].view(np.uint64)) for k in range(3))

# plain: tensors of the default stream
t0, t1 = torch.from_numpy(f0).cuda(), torch.from_numpy(f1).cuda()
out = torch.as_tensor(device.bb_flow(t0, t1, Nt, dtype="float64", **kw), device="cuda")
assert out.shape == (3, h, w) and same(out, ref), "bb_flow"
out = torch.as_tensor(device.gn_flow(t0, t1, 0.1, 0.2, dtype="float64"), device="cuda")
assert same(out, gref), "gn_flow"

# ordering: inputs produced by torch ops on a side stream, handed over without a synchronise,
# and overwritten on that stream as soon as the call returns
side = torch.cuda.Stream()
base0, base1 = torch.from_numpy(f0.astype(np.int32)).cuda(), torch.from_numpy(f1.astype(np.int32)).cuda()
big = torch.ones(1 << 24, device="cuda")
torch.cuda.synchronize()
for name in ("bb", "gn"):
    with torch.cuda.stream(side):
        for _ in range(4):
            big = big * 1.0000001 + 0.0        # keeps the stream busy ahead of the producers
        x0 = ((base0 * 3 + 7 - 7) // 3).to(torch.uint8)
        x1 = ((base1 * 3 + 7 - 7) // 3).to(torch.uint8)
        if name == "bb":
            res = device.bb_flow(x0, x1, Nt, dtype="float64", stream=side, **kw)
        else:
            res = device.gn_flow(x0, x1, 0.1, 0.2, dtype="float64", stream=side)
        x0.fill_(255)
        x1.zero_()
        out = torch.as_tensor(res, device="cuda")
        ok = same(out, ref if name == "bb" else gref)     # (.cpu() waits on the side stream)
    assert ok, "ordering: " + name
torch.cuda.synchronize()
print("TORCH CHILD OK")
"""


def test_torch_producer():
    code = _TORCH_CHILD.format(repo=REPO, pkg=PKG)
    env = dict(os.environ)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0 and "TORCH CHILD OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
