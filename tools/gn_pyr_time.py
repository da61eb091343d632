"""Coarse-to-fine GN against the single solve, timed at 640x480 on the bench's GN pair (the config-3
stand-in: sinusoid pair, alpha 0.1, lambda 0.2): Plan.solve_device, Pyramid(levels=1, warps=1) and
Pyramid(levels=4, warps=3), each a reused object solving the same device frames over and over.

Events are torch.cuda.Event on a side stream that is handed to the calls as their stream (the *_dev
stream contract orders the library's stream inside the pair); a measurement is the time of REPS
back-to-back solves between two events, divided by REPS.  Every run is printed; the median is the
figure, the spread of the runs the noise.  The solves wait on the host for the PCG's stop flag, so
the figure is the time of a solve as a caller sees it.  The pyramid's own report (device events per
level, and around its own steps between the solves) gives the share of the new kernels.
usage: python tools/gn_pyr_time.py [--w 640 --h 480] [--reps 10 --runs 7] [--levels 4 --warps 3]"""
import argparse
import json
import os
import sys

import torch  # first: libfoto then binds to torch's HIP runtime
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "optical-flow-optimal-transport_amd"))
from foto import gn  # noqa: E402
from foto.device import DeviceArray  # noqa: E402
from foto.synthetic import sinusoid_pair  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--w", type=int, default=640)
ap.add_argument("--h", type=int, default=480)
ap.add_argument("--alpha", type=float, default=0.1)
ap.add_argument("--lam", type=float, default=0.2)
ap.add_argument("--levels", type=int, default=4)
ap.add_argument("--warps", type=int, default=3)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--runs", type=int, default=7)
A = ap.parse_args()
w, h = A.w, A.h
side = torch.cuda.Stream()
f1, f2 = sinusoid_pair(w, h)
d1, d2 = DeviceArray.from_numpy(f1.reshape(h, w)), DeviceArray.from_numpy(f2.reshape(h, w))
out = DeviceArray((3, h, w), np.float32)
print(f"device: {torch.cuda.get_device_name(0)}; {w}x{h} sinusoid pair, alpha {A.alpha}, lambda {A.lam}; "
      f"{A.reps} solves per measurement, {A.runs} runs")


def timed(solve):
    solve()
    solve()   # (the second solve runs with the first one's iteration predictions, like the rest)
    ms = []
    for _ in range(A.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        for _ in range(A.reps):
            solve()
        e1.record(side)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / A.reps)
    return ms


res = {"size": [w, h], "reps": A.reps, "runs": A.runs}
with torch.cuda.stream(side):
    with gn.Plan(w, h, A.alpha, A.lam) as P:
        ms = timed(lambda: P.solve_device(d1, d2, out=out, stream=side))
        tm = P.timing()
        res["plan"] = {"ms": ms, "median": float(np.median(ms)), "pcg_its": tm["iterations"]}
    for name, (L, W) in (("pyr_1x1", (1, 1)), (f"pyr_{A.levels}x{A.warps}", (A.levels, A.warps))):
        with gn.Pyramid(w, h, A.alpha, A.lam, levels=L, warps=W) as Q:
            ms = timed(lambda: Q.solve_device(d1, d2, out=out, stream=side))
            _, info, st = Q.solve_device(d1, d2, out=out, stream=side, stats=True)
            dev = sum(st["ms_level"])
            res[name] = {"ms": ms, "median": float(np.median(ms)), "info": info, "sizes": st["sizes"],
                         "pcg_its": st["iterations"], "ms_level": st["ms_level"], "ms_levels_sum": dev,
                         "ms_new": st["ms_new"], "new_share": st["ms_new"] / dev}
    side.synchronize()

base = res["plan"]["median"]
for name, r in res.items():
    if not isinstance(r, dict):
        continue
    m = r["ms"]
    print(f"{name}: ms per solve by run: " + ", ".join(f"{t:.3f}" for t in m))
    print(f"{name}: median {r['median']:.3f} ms, min {min(m):.3f}, max {max(m):.3f} "
          f"(spread {100 * (max(m) - min(m)) / r['median']:.1f} % of the median); "
          f"{r['median'] / base:.3f} x Plan.solve_device; PCG its {r['pcg_its']}")
    if "ms_new" in r:
        print(f"{name}: levels {r['sizes']}, device ms per level {['%.3f' % t for t in r['ms_level']]} "
              f"(sum {r['ms_levels_sum']:.3f}); own steps between the solves (restrict, prolong, warp, "
              f"flow copies) {r['ms_new']:.3f} ms = {100 * r['new_share']:.1f} % of the levels' device time")
print("JSON " + json.dumps(res))
del P, Q   # (the lambdas above keep them reachable until module teardown otherwise)
