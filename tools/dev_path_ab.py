"""Device-buffer path against the host path of the same build, same process, same GPU.

(a) GN 640x480, a fresh (different) pair per call: host Plan.solve against Plan.solve_device,
    host wall time per call and foto_gn_plan_timing's device times.
(b) BB 640x480x16: reset + flow (host arrays) against reset_device + flow_device, after the same
    outer iterations (untimed) -- the staging around a solve, not the solve.
(c) the main.py evaluation sequence -- warp, IE, EE / AE -- host entries against the *_dev ones.

Synthetic inputs; median (and min) of N calls after 3 warm-ups.  The device variants' frames and
flows are made resident before the timed region (that is the case the interface is for); the
host variants include their uploads and downloads (that is what they cost a caller).
usage: python tools/dev_path_ab.py [--n 20] [--w 640 --h 480 --nt 16]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "optical-flow-optimal-transport_amd"))
from foto import evaluate, gn  # noqa: E402
from foto.bb import BBSolver  # noqa: E402
from foto.device import DeviceArray  # noqa: E402
from foto.synthetic import textured_pair  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=20)
ap.add_argument("--w", type=int, default=640)
ap.add_argument("--h", type=int, default=480)
ap.add_argument("--nt", type=int, default=16)
ap.add_argument("--its", type=int, default=2)
A = ap.parse_args()
w, h, N, WARM = A.w, A.h, A.n, 3


def med(xs):
    return f"median {1e3 * statistics.median(xs):.3f} ms, min {1e3 * min(xs):.3f} ms (n = {len(xs)})"


def timed(fn, reps):
    out = []
    for k in range(reps):
        t = time.perf_counter()
        fn(k)
        out.append(time.perf_counter() - t)
    return out


pairs = [textured_pair(w, h, seed=k, dx=1.0 + 0.1 * k, dy=0.5) for k in range(N + WARM)]
pairs8 = [tuple(np.round(f.reshape(h, w) * 255).astype(np.uint8) for f in p) for p in pairs]
hpairs8 = [tuple(f.astype(np.float64).ravel() / 255 for f in p) for p in pairs8]
dpairs8 = [tuple(DeviceArray.from_numpy(f) for f in p) for p in pairs8]

# ------------------------------------------------------------------ (a) GN fresh pairs
print(f"(a) GN {w}x{h}, alpha 0.1, lambda 0.2, a different pair per call (uint8 frames / 255)")
for name in ("host", "device"):
    with gn.Plan(w, h, 0.1, 0.2) as P:
        dev_t = []
        out = DeviceArray((3, h, w), np.float32)

        def call(k):
            if name == "host":
                P.solve(*hpairs8[k])
            else:
                P.solve_device(*dpairs8[k], out=out, dtype="float32")
            dev_t.append(P.timing())
        timed(call, WARM)
        del dev_t[:]
        ts = timed(lambda k: call(k + WARM), N)
        setup = statistics.median(t["ms_setup"] for t in dev_t)
        pcg = statistics.median(t["ms_pcg"] for t in dev_t)
        its = statistics.median(t["iterations"] for t in dev_t)
        print(f"  {name:6s} wall per call: {med(ts)}; device: setup {setup:.3f} ms, PCG {pcg:.3f} ms, {its:.0f} its")
print("  (the device call returns with the export enqueued; its wall time includes the PCG's host waits)")

# ------------------------------------------------------------------ (b) BB reset + flow
print(f"(b) BB {w}x{h}x{A.nt}: new pair in + flow out around {A.its} outer iterations (iterations untimed)")
f0, f1 = pairs[0]
with BBSolver(f0, f1, A.nt, w, h) as s:
    dpairs = [tuple(DeviceArray.from_numpy(f.reshape(h, w)) for f in p) for p in pairs]
    out = DeviceArray((3, h, w), np.float32)
    for name in ("host", "device"):
        t_in, t_out = [], []
        for k in range(N + WARM):
            t = time.perf_counter()
            if name == "host":
                s.reset(*pairs[k])
            else:
                s.reset_device(*dpairs[k])
            t_in.append(time.perf_counter() - t)
            s.iterate(A.its, stop_rules=False)
            s.sync()
            t = time.perf_counter()
            if name == "host":
                s.flow()
            else:
                s.flow_device(out=out)
            t_out.append(time.perf_counter() - t)
        print(f"  {name:6s} reset: {med(t_in[WARM:])}")
        print(f"  {name:6s} flow:  {med(t_out[WARM:])}")

# ------------------------------------------------------------------ (c) evaluation sequence
print(f"(c) evaluation {w}x{h}: warp + IE + EE/AE (main.py's sequence)")
n = w * h
rng = np.random.default_rng(0)
u, v, m = rng.normal(0, 1, n), rng.normal(0, 1, n), rng.normal(0, 0.05, n)
uG, vG = u + rng.normal(0, 0.2, n), v + rng.normal(0, 0.2, n)
f1, f2 = pairs[0]
dev = {k: DeviceArray.from_numpy(x) for k, x in dict(f1=f1, f2=f2, u=u, v=v, m=m, uG=uG, vG=vG).items()}
dw = DeviceArray((h, w), np.float64)


def host_eval(_):
    fw = evaluate.warp(f1, u, v, w, h, m)
    return evaluate.intensity_error(fw, f2, w, h), evaluate.flow_errors(u, v, uG, vG, w, h)


def dev_eval(_):
    evaluate.warp_device(dev["f1"], dev["u"], dev["v"], w, h, dev["m"], out=dw)
    return evaluate.intensity_error_device(dw, dev["f2"], w, h), \
        evaluate.flow_errors_device(dev["u"], dev["v"], dev["uG"], dev["vG"], w, h)


assert host_eval(0) == dev_eval(0)
for name, fn in (("host", host_eval), ("device", dev_eval)):
    timed(fn, WARM)
    print(f"  {name:6s} {med(timed(fn, N))}")
