"""The flow algebra's three kernels (foto_flow_compose_dev, foto_flow_invert_dev,
foto_flow_consistency_dev: k_compose, k_invert, k_consistency) timed with HIP events on the shape of
a flow path, beside their traffic-model times at the stream rate foto_stream_probe measures in the
same process on the same device (DESIGN.md 3.14 has the model and the numbers).

The buffer: R records of w x h, float32 planar (flow_path_device's output at the bench grid: 31 x
640 x 480).  Two fillings: "smooth", a wavy flow of about a pixel per record (what a transport path
holds), and "random", N(0, 2^2) px per pixel (every gather lands somewhere else: the worst case).
compose writes all records; invert runs 6 rounds; consistency checks the buffer against its inverse
and writes the mask, the float32 error and the table.

Events are torch.cuda.Event (HIP events) on a side stream that is handed to the calls as their
stream; every call is timed on its own, WARM warm-up calls, then the median of CALLS.  The timed
calls are the C entries through ctypes with the pointers worked out beforehand.
usage: python tools/chain_time.py [--w 640 --h 480 --records 31] [--warm 20 --calls 100]"""
import argparse
import ctypes
import os
import sys

import torch  # first: libfoto then binds to torch's HIP runtime
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "optical-flow-optimal-transport_amd"))
from foto import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--w", type=int, default=640)
ap.add_argument("--h", type=int, default=480)
ap.add_argument("--records", type=int, default=31)
ap.add_argument("--warm", type=int, default=20)
ap.add_argument("--calls", type=int, default=100)
A = ap.parse_args()
w, h, R = A.w, A.h, A.records
n = w * h
side = torch.cuda.Stream()
L, P = _lib.lib(), ctypes.c_void_p
F32 = _lib.FOTO_F32


def median_us(fn):
    for _ in range(A.warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(A.calls)]
    for a, b in ev:
        a.record(side)
        fn()
        b.record(side)
    side.synchronize()
    return float(np.median([1e3 * a.elapsed_time(b) for a, b in ev]))


def fill(kind):
    jj, ii = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    if kind == "smooth":
        k = np.arange(R, dtype=np.float64)[:, None, None]
        u = 1.2 * np.sin(ii / 40 + 0.3 * k) * np.cos(jj / 50)
        v = 0.9 * np.cos(ii / 45) * np.sin(jj / 35 + 0.2 * k)
        m = 0.01 * np.sin(ii / 30) * np.ones_like(k)
    else:
        rng = np.random.default_rng(0)
        u, v = 2.0 * rng.standard_normal((2, R, h, w))
        m = 0.01 * rng.standard_normal((R, h, w))
    return torch.from_numpy(np.stack([u, v, m], axis=1).astype(np.float32)).cuda()


# the stream rate of this device: foto_stream_probe reads and writes two n-double vectors (32 B per element)
pn = R * 3 * n // 2 * 2
us = (ctypes.c_double * 2)()
_lib.check(L.foto_stream_probe(pn, 20, us))
rate = 32.0 * pn / (min(us[0], us[1]) * 1e-6)   # bytes per second
print(f"device: {torch.cuda.get_device_name(0)}; {R} records of {w} x {h}, float32 planar; {A.warm} warm-ups, median of "
      f"{A.calls} calls; stream rate {rate / 1e9:.0f} GB/s (foto_stream_probe over {pn} doubles: plain {us[0]:.1f} us, "
      f"write-through {us[1]:.1f} us)")

# the traffic model, bytes per pixel and record (float32 planar in and out): every input element once, every output once
MODEL = {"compose all": 3 * 4 + 3 * 4,          # u, v, m in; u, v, m out
         "invert(6)": 2 * 4 + 3 * 4,            # u, v in; u, v, m out
         "consistency": 2 * 4 + 2 * 4 + 1 + 4}  # F and B (u, v) in; mask and float32 error out

for kind in ("smooth", "random"):
    with torch.cuda.stream(side):
        flow = fill(kind)
        out = torch.empty_like(flow)
        back = torch.empty_like(flow)
        valid = torch.empty((R, h, w), dtype=torch.uint8, device="cuda")
        err = torch.empty((R, h, w), dtype=torch.float32, device="cuda")
        table = torch.empty((R, 4), dtype=torch.float64, device="cuda")
        side.synchronize()
        st = P(side.cuda_stream)
        fl = _lib.Flow()
        fl.data, fl.dtype, fl.layout, fl.records = flow.data_ptr(), F32, 0, R
        bk = _lib.Flow()
        bk.data, bk.dtype, bk.layout, bk.records = back.data_ptr(), F32, 0, R
        calls = {
            "compose all": lambda: _lib.check(L.foto_flow_compose_dev(ctypes.byref(fl), w, h, 0, P(out.data_ptr()), F32, 0, st)),
            "invert(6)": lambda: _lib.check(L.foto_flow_invert_dev(ctypes.byref(fl), w, h, 6, P(back.data_ptr()), F32, 0, st)),
            "consistency": lambda: _lib.check(L.foto_flow_consistency_dev(
                ctypes.byref(fl), ctypes.byref(bk), w, h, 0.01, 0.5, P(valid.data_ptr()), P(err.data_ptr()), F32,
                P(table.data_ptr()), st)),
        }
        for name, fn in calls.items():
            t = median_us(fn)
            model = MODEL[name] * n * R / rate * 1e6
            print(f"{kind:6s} {name:12s} {t:8.1f} us; model {MODEL[name]} B per pixel and record = {model:6.1f} us at the "
                  f"stream rate; ratio {t / model:.2f}")
        side.synchronize()
        counts = table.cpu().numpy().sum(axis=0)
        print(f"{kind:6s} class counts over all records (0, 1, 2, 3): {[int(c) for c in counts]}")
