"""Flow algebra on the device (include/foto.h, "flow algebra") against tests/chain_ref.py, the numpy
restatement of its definitions in the kernels' operation order.

Bar.  The operations are + - * sqrt, comparisons, floor and min / max, and the library is built with
-ffp-contract=off: float64 outputs equal the reference value for value (NaN where it is NaN), and
float32 outputs equal ``ref.astype(float32)`` the same way; masks and class counts are equal.  The
copy of K = 1 is compared on the bit patterns.  tests/test_chain_host.py shows on the numpy values
that the derived bounds used here hold and that no cross-check pixel sits within 1e-9 relative of
its threshold."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, REPO

import chain_ref as R
from foto import _lib, chain, evaluate
from foto import device as D
from chain_ref import CONS, SHIFTS

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
P, I = "planar", "interleaved"
COMBOS = [(d, l) for d in (F32, F64) for l in (P, I)]
# w, h, K, in dtype, in layout, out dtype, out layout: every combination at 37 x 29, one each elsewhere
CASES = [(37, 29, 2, di, li, do, lo) for di, li in COMBOS for do, lo in COMBOS] + [
    (2, 2, 2, F64, P, F64, P),       # every tap clamped
    (3, 2, 5, F32, I, F32, I),       # the smallest non-square clamped case
    (130, 18, 2, F32, P, F32, P),    # wider than one block row
    (64, 48, 5, F64, P, F32, I),     # several records chained
    (37, 29, 1, F32, P, F64, P),
    (37, 29, 5, F64, I, F64, P),
]


def _id(c):
    w, h, K, di, li, do, lo = c
    return f"{w}x{h}x{K}-{np.dtype(di).name}-{li}-to-{np.dtype(do).name}-{lo}"


IDS = [_id(c) for c in CASES]


def dev(a):
    return D.DeviceArray.from_numpy(a)


def same(got, want, dtype=None):
    want = want if dtype is None else want.astype(dtype)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------ 1. compose against the reference

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_compose_matches_the_reference(case):
    w, h, K, di, li, do, lo = case
    f = R.random_flow(K, h, w, li, di, seed=w + K)
    d = dev(f)
    ref = R.compose(f, li, lo)
    got = chain.compose(d, in_layout=li, dtype=do, layout=lo).to_numpy()
    same(got, ref, do)
    last = chain.compose(d, in_layout=li, dtype=do, layout=lo, last_only=True).to_numpy()
    same(last, ref[-1], do)                                  # `all` and `last_only` agree on the last record
    np.testing.assert_array_equal(d.to_numpy(), f)           # the input is read only
    if lo == P and li == P and K > 1:                        # the gain rule, restated on its own
        u, v, m = R.split(f, P)
        x, y = R.grid(h, w)
        g = (1.0 + ref[0, 2]) * (1.0 + R.S(m[1], x + ref[0, 0], y + ref[0, 1])) - 1.0
        same(got[1, 2], g, do)
    if lo == P and li == I:                                  # no m to compose: +0.0
        assert not np.any(got[:, 2]) and not np.any(np.signbit(got[:, 2]))


@pytest.mark.parametrize("layout", [P, I])
def test_compose_of_one_record_copies_the_bits(layout):
    f = R.random_flow(1, 29, 37, layout, F64, 5)
    f.reshape(-1).view(np.uint64)[[7, 400]] = [0x7ff8000000001234, 0xfff0000000000001]   # NaN payloads
    for last in (False, True):
        got = chain.compose(dev(f), in_layout=layout, last_only=last).to_numpy()
        assert np.array_equal(got.reshape(-1).view(np.uint64), f.reshape(-1).view(np.uint64))


# ------------------------------------------------------------------ 2. compose exactness

@pytest.mark.parametrize("dtype", [F32, F64])
def test_integer_shifts_compose_to_their_sum(dtype):
    h, w = 48, 64
    f = R.shifts_flow(SHIFTS, h, w, dtype=dtype)
    got = chain.compose(dev(f)).to_numpy()
    assert got.dtype == dtype
    same(got, R.compose(f), dtype)
    run = np.cumsum(np.array(SHIFTS, dtype=np.float64), axis=0)
    x, y = R.grid(h, w)
    inside = np.ones((h, w), bool)
    for k in range(len(SHIFTS)):
        inside &= (x + run[k, 0] >= 0) & (x + run[k, 0] <= w - 1) & (y + run[k, 1] >= 0) & (y + run[k, 1] <= h - 1)
        assert np.all(got[k, 0][inside] == run[k, 0]) and np.all(got[k, 1][inside] == run[k, 1])


# ------------------------------------------------------------------ 3. a NaN pocket stays local

def test_nan_pocket_stays_local():
    f = R.random_flow(3, 29, 37, P, F64, 6)
    f[1, 0, 14, 18] = np.nan
    ref = R.compose(f)
    got = chain.compose(dev(f)).to_numpy()
    bad = np.isnan(ref)
    assert not bad[0].any() and 0 < bad[1].sum() and bad.sum() < 200       # (known from the host test)
    assert np.array_equal(np.isnan(got), bad)
    same(got, ref)


# ------------------------------------------------------------------ 4. invert against the reference

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_invert_matches_the_reference(case):
    w, h, K, di, li, do, lo = case
    f = R.random_flow(K, h, w, li, di, seed=100 + w + K)
    got = chain.invert(dev(f), in_layout=li, iters=6, dtype=do, layout=lo).to_numpy()
    same(got, R.invert(f, 6, li, lo), do)
    if lo == P:
        assert not np.any(got[:, 2]) and not np.any(np.signbit(got[:, 2]))


@pytest.mark.parametrize("iters", [1, 6, 16])
def test_invert_of_the_smooth_flow(iters):
    F = R.smooth_flow()
    B = chain.invert(dev(F), iters=iters).to_numpy()
    same(B, R.invert(F, iters))
    if iters == 16:   # |J F| < 0.4, |F| < 2: 0.4^16 * 2 < 1e-6 (derived; numpy meets it in the host test)
        assert R.inversion_residual(F, B) <= 1e-6


# ------------------------------------------------------------------ 5. consistency against the reference

def _consistency(f, b, lf, lb, err_dtype, **kw):
    valid, table, err = chain.consistency(dev(f), dev(b), layout=lf, bwd_layout=lb, err=err_dtype, **kw)
    rv, rt, re, _, margin = R.consistency(f, b, lf, lb, **kw)
    assert margin.min() > 1e-9, "a numpy value within 1e-9 relative of its threshold"   # (the precondition)
    valid, table, err = valid.to_numpy(), table.to_numpy(), err.to_numpy()
    same(valid, rv)
    same(table, rt)
    same(err, re, err_dtype)
    assert np.all(table.sum(axis=1) == rv.shape[1] * rv.shape[2])
    return valid, table, err


@pytest.mark.parametrize("df,lf,db,lb", [(a, b, c, d) for a, b in COMBOS for c, d in COMBOS])
def test_consistency_every_combination(df, lf, db, lb):
    w, h, K, seed = CONS[2]
    f, b = R.cons_case(K, h, w, seed, layout=lf, dtype=df, bwd_layout=lb, bwd_dtype=db)
    _, table, _ = _consistency(f, b, lf, lb, "float32" if df == F32 else "float64")
    assert np.all(table.sum(axis=0) > 0)     # every class occurs


@pytest.mark.parametrize("w,h,K,seed", CONS)
@pytest.mark.parametrize("bwd_records", [None, 1])
def test_consistency_shapes_and_broadcast(w, h, K, seed, bwd_records):
    f, b = R.cons_case(K, h, w, seed, bwd_records=bwd_records)
    assert b.shape[0] == (K if bwd_records is None else 1)
    _, table, err = _consistency(f, b, P, P, "float64")
    assert table[0, 3] >= 1 and np.isnan(err).sum() == table[:, 3].sum()
    # other thresholds are arguments, not constants
    _consistency(f, b, P, P, "float64", alpha1=0.0, alpha2=0.125)


def test_consistency_of_a_flow_and_its_inverse():
    F = R.smooth_flow()
    dF = dev(F)
    valid, table = chain.consistency(dF, chain.invert(dF, iters=16))
    valid, table = valid.to_numpy(), table.to_numpy()
    x, y = R.grid(48, 64)
    qx, qy = x + F[0, 0], y + F[0, 1]
    inside = (qx >= 0) & (qx <= 63) & (qy >= 0) & (qy <= 47)
    assert np.array_equal(valid[0] == 1, inside)             # class 0 everywhere the target stays in frame
    assert table[0, 0] == inside.sum() and table[0, 2] == (~inside).sum() and table[0, 1] == table[0, 3] == 0


def test_consistency_marks_the_band_of_a_discontinuity():
    fwd, bwd = R.step_flow()
    valid, table, _ = _consistency(fwd, bwd, P, P, "float64")
    cls1 = R.consistency(fwd, bwd)[3][0] == 1
    assert np.array_equal(valid[0] == 0, cls1) and table[0, 1] == cls1.sum() == 6 * 48
    assert sorted(set(np.nonzero(valid[0] == 0)[1])) == [29, 30, 31, 32, 33, 34]


def test_consistency_of_infinite_flows():
    f, b = R.cons_case(1, 29, 37, 21)
    f[0, :2, 3, 4:9] = [[np.inf] * 5, [-np.inf] * 5]
    b[0, 0, 20, 20] = np.inf
    valid, table, err = _consistency(f, b, P, P, "float64")
    assert not valid[0, 3, 4:9].any() and np.isnan(err[0, 3, 4:9]).all() and table[0, 3] >= 6


# ------------------------------------------------------------------ 6. the mask plugs in

def test_the_mask_plugs_into_score_flow():
    w, h, K, seed = CONS[2]
    f, b = R.cons_case(1, h, w, seed, dtype=F32)
    df = dev(f[0])
    valid, table = chain.consistency(df, dev(b[0]))
    assert valid.shape == (h, w) and table.shape == (4,)
    gt = dev(np.zeros((h, w, 2), F32))
    s = evaluate.score_flow(df, gt, mask=valid)
    assert s.n == table.to_numpy()[0] == np.count_nonzero(valid.to_numpy()) > 0


# ------------------------------------------------------------------ 7. argument errors

class View:
    def __init__(self, shape, typestr, ptr):
        self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(ptr, False), version=3, strides=None)


def test_argument_errors_leave_the_outputs_untouched():
    L = _lib.lib()
    w, h, K = 37, 29, 3
    f = R.random_flow(K, h, w, P, F32, 9)
    d, d2 = dev(f), dev(f[:2])
    out = dev(np.full((K, 3, h, w), 7.25, F32))
    valid = dev(np.full((K, h, w), 9, np.uint8))
    table = dev(np.full((K, 4), 7.25))
    fl = _lib.Flow()
    fl.data, fl.dtype, fl.layout, fl.records = d.ptr, _lib.FOTO_F32, 0, K
    f2 = _lib.Flow()
    f2.data, f2.dtype, f2.layout, f2.records = d2.ptr, _lib.FOTO_F32, 0, 2
    host = _lib.Flow()
    host.data, host.dtype, host.layout, host.records = f.ctypes.data, _lib.FOTO_F32, 0, K
    o, F4 = ctypes.c_void_p(out.ptr), _lib.FOTO_F32
    # an output over its input
    assert L.foto_flow_compose_dev(ctypes.byref(fl), w, h, 0, ctypes.c_void_p(d.ptr), F4, 0, None) == _lib.FOTO_ERR_ARG
    with pytest.raises(_lib.FotoError):
        chain.invert(d, out=View((K, 3, h, w), "<f4", d.ptr))
    assert L.foto_flow_consistency_dev(ctypes.byref(fl), ctypes.byref(fl), w, h, 0.01, 0.5, ctypes.c_void_p(d.ptr), None, 0,
                                       ctypes.c_void_p(table.ptr), None) == _lib.FOTO_ERR_ARG
    # a host pointer where device memory is required
    assert L.foto_flow_compose_dev(ctypes.byref(host), w, h, 0, o, F4, 0, None) == _lib.FOTO_ERR_ARG
    assert L.foto_last_error()
    # a misaligned out
    assert L.foto_flow_invert_dev(ctypes.byref(fl), w, h, 6, ctypes.c_void_p(out.ptr + 2), F4, 0, None) == _lib.FOTO_ERR_ARG
    # 2 backward records against 3
    assert L.foto_flow_consistency_dev(ctypes.byref(fl), ctypes.byref(f2), w, h, 0.01, 0.5, ctypes.c_void_p(valid.ptr), None,
                                       0, ctypes.c_void_p(table.ptr), None) == _lib.FOTO_ERR_ARG
    assert np.all(out.to_numpy() == 7.25) and np.all(valid.to_numpy() == 9) and np.all(table.to_numpy() == 7.25)
    np.testing.assert_array_equal(d.to_numpy(), f)


# ------------------------------------------------------------------ 8. bb_sequence

def test_bb_sequence_records_are_the_pair_flows():
    w, h, Nt = 32, 24, 4
    x, y = R.grid(h, w)
    frames = [0.2 + 0.7 * np.exp(-((x - 12 - 2.5 * k) ** 2 + (y - 10 - 1.5 * k) ** 2) / (2 * 4.0 ** 2)) for k in range(3)]
    dfr = [dev(f) for f in frames]
    kw = dict(r=1.0, convergence_tol=0.01, reg_epsilon=1e-2, max_it=6, dtype="float64")
    seq = D.bb_sequence(dfr, Nt, **kw)
    assert seq.shape == (2, 3, h, w)
    rec = seq.to_numpy()
    for k in range(2):
        pair = D.bb_flow(dfr[k], dfr[k + 1], Nt, **kw).to_numpy()
        assert np.array_equal(rec[k].view(np.uint64), pair.view(np.uint64))
    assert np.abs(rec[:, :2]).max() > 0.1                     # the frames do move
    same(chain.compose(seq).to_numpy(), R.compose(rec))
    stacked = D.bb_sequence(dev(np.stack(frames)), Nt, layout=I, **kw)      # one (K + 1, h, w) array; interleaved
    same(stacked.to_numpy(), np.ascontiguousarray(np.moveaxis(rec[:, :2], 1, -1)))


def test_numpy_arrays_are_uploaded_and_downloaded():
    f = R.random_flow(3, 18, 20, I, F32, 3)
    got = chain.compose(f, in_layout=I, layout=P, dtype="float64", last_only=True)
    assert isinstance(got, np.ndarray)
    same(got, R.compose(f, I, P, last_only=True)[0])
    B = chain.invert(f[0], in_layout=I)
    same(B, R.invert(f[:1], 6, I)[0], F32)
    valid, table, err = chain.consistency(f[0], B, layout=I, err=True)
    rv, rt, re, _, _ = R.consistency(f[:1], B[None], I)
    same(valid, rv[0]), same(table, rt[0]), same(err, re[0])


# ------------------------------------------------------------------ 9. stream order with torch

_TORCH_CHILD = r"""
import sys
sys.path[:0] = [{repo!r}, {pkg!r}, {tests!r}]
import torch                      # first: libfoto then binds to torch's HIP runtime
import numpy as np
import chain_ref as R
from foto import chain

w, h, K = 37, 29, 3
f = R.random_flow(K, h, w, "planar", np.float64, 31)
want_c = R.compose(2.0 * f)
want_b = R.invert(2.0 * f, 6)
want_v, want_t, _, _, _ = R.consistency(2.0 * f, want_b)
src = torch.from_numpy(f).cuda()
side = torch.cuda.Stream()
big = torch.ones(1 << 24, device="cuda")
torch.cuda.synchronize()
with torch.cuda.stream(side):
    a = torch.zeros_like(src)
    comp = torch.full((K, 3, h, w), -1.0, dtype=torch.float64, device="cuda")
    back = torch.full((K, 3, h, w), -1.0, dtype=torch.float64, device="cuda")
    valid = torch.full((K, h, w), 9, dtype=torch.uint8, device="cuda")
    table = torch.full((K, 4), -1.0, dtype=torch.float64, device="cuda")
    for _ in range(4):
        big = big * 1.0000001 + 0.0        # keeps the stream busy ahead of the producer
    a.copy_(2.0 * src)                     # the flow is produced by a kernel on this stream
    assert chain.compose(a, out=comp, stream=side) is comp
    assert chain.invert(a, out=back, stream=side) is back
    v, t = chain.consistency(a, back, out=valid, table_out=table, stream=side)
    assert v is valid and t is table
    a.fill_(0)                             # the input may be overwritten as soon as the call returns
    got_c = (comp + 1.0).cpu().numpy()     # consumers on the same stream, no host sync between
    got_b = (back + 1.0).cpu().numpy()
    got_v = (valid + 1).cpu().numpy()
    got_t = (table + 1.0).cpu().numpy()
np.testing.assert_array_equal(got_c, want_c + 1.0)
np.testing.assert_array_equal(got_b, want_b + 1.0)
np.testing.assert_array_equal(got_v, want_v + 1)
np.testing.assert_array_equal(got_t, want_t + 1.0)
torch.cuda.synchronize()
print("TORCH CHILD OK")
"""


def test_torch_stream_order():
    if importlib.util.find_spec("torch") is None:
        pytest.skip("torch is not installed")
    code = _TORCH_CHILD.format(repo=REPO, pkg=PKG, tests=os.path.join(REPO, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, env=dict(os.environ))
    assert r.returncode == 0 and "TORCH CHILD OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
