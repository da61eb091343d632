"""TV-L1 at its defaults against the GN pyramid (levels 4, warps 3), timed at 640x480 on the bench's
GN pair (sinusoid pair; GN at alpha 0.1, lambda 0.2): each a reused object solving the same device
frames over and over, tools/gn_pyr_time.py's method -- torch.cuda.Event on a side stream handed to
the calls as their stream, REPS back-to-back solves between two events, every run printed, the
median the figure.  One TV-L1 solver per --per-launch value: 1 is a launch per inner iteration, K > 1
the LDS tile kernel with K iterations per launch; all give the same bits.  The TV-L1 solve never
waits on the host (all counts are fixed); the GN pyramid waits for every PCG's stop flag.  The
solver's own report gives the launches and the device time per level, from which the time per inner
iteration (a level's device time over its warps * iters iterations; the warps' coefficient launches
and the prolongation are inside it) follows.
usage: python tools/tvl1_time.py [--w 640 --h 480] [--reps 10 --runs 7] [--per-launch 1 3 5 6] [--only-tvl1]"""
import argparse
import json
import os
import sys

import torch  # first: libfoto then binds to torch's HIP runtime
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "optical-flow-optimal-transport_amd"))
from foto import gn, tvl1  # noqa: E402
from foto.device import DeviceArray  # noqa: E402
from foto.synthetic import sinusoid_pair  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--w", type=int, default=640)
ap.add_argument("--h", type=int, default=480)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--only-tvl1", action="store_true", help="the TV-L1 solves alone (for a kernel trace)")
ap.add_argument("--per-launch", type=int, nargs="+", default=[1, 3, 5, 6],
                help="inner iterations per kernel launch, one timed solver each (1: a launch per iteration)")
A = ap.parse_args()
w, h = A.w, A.h
side = torch.cuda.Stream()
f1, f2 = sinusoid_pair(w, h)
d1, d2 = DeviceArray.from_numpy(f1.reshape(h, w)), DeviceArray.from_numpy(f2.reshape(h, w))
out = DeviceArray((3, h, w), np.float32)
print(f"device: {torch.cuda.get_device_name(0)}; {w}x{h} sinusoid pair; {A.reps} solves per measurement, {A.runs} runs")


def timed(solve):
    solve()
    solve()
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
    for per in A.per_launch:
        with tvl1.TVL1(w, h, per_launch=per) as T:
            ms = timed(lambda: T.solve_device(d1, d2, out=out, stream=side))
            _, st = T.solve_device(d1, d2, out=out, stream=side, stats=True)
            o = T.opts
            its = o["warps"] * o["iters"]
            res[f"tvl1_x{per}"] = {"ms": ms, "median": float(np.median(ms)), "opts": o, "sizes": st["sizes"],
                                   "launches": st["launches"], "ms_level": st["ms_level"],
                                   "ms_levels_sum": sum(st["ms_level"]),
                                   "us_per_iteration": [1e3 * t / its for t in st["ms_level"]]}
    if not A.only_tvl1:
        with gn.Pyramid(w, h, 0.1, 0.2, levels=4, warps=3) as Q:
            ms = timed(lambda: Q.solve_device(d1, d2, out=out, stream=side))
            _, info, st = Q.solve_device(d1, d2, out=out, stream=side, stats=True)
            res["gn_pyr_4x3"] = {"ms": ms, "median": float(np.median(ms)), "info": info, "sizes": st["sizes"],
                                 "pcg_its": st["iterations"], "ms_level": st["ms_level"],
                                 "ms_levels_sum": sum(st["ms_level"])}
    side.synchronize()

for name, r in res.items():
    if not isinstance(r, dict):
        continue
    m = r["ms"]
    print(f"{name}: ms per solve by run: " + ", ".join(f"{t:.3f}" for t in m))
    print(f"{name}: median {r['median']:.3f} ms, min {min(m):.3f}, max {max(m):.3f} "
          f"(spread {100 * (max(m) - min(m)) / r['median']:.1f} % of the median)")
    print(f"{name}: levels {r['sizes']}, device ms per level {['%.3f' % t for t in r['ms_level']]} "
          f"(sum {r['ms_levels_sum']:.3f})")
    if "launches" in r:
        print(f"{name}: launches per level {r['launches']}; us per inner iteration by level "
              f"{['%.2f' % t for t in r['us_per_iteration']]}")
if "gn_pyr_4x3" in res:
    for per in A.per_launch:
        print(f"tvl1_x{per} / gn_pyr_4x3: {res[f'tvl1_x{per}']['median'] / res['gn_pyr_4x3']['median']:.3f}")
print("JSON " + json.dumps(res))
del T   # (the lambdas above keep the solvers reachable until module teardown otherwise)
if not A.only_tvl1:
    del Q
