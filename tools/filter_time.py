"""The workload behind the kernel times of DESIGN.md 3.15 (profiles/filter_kernel_times.txt):
foto_flow_median_dev (k_median<R>) on one 640 x 480 record, float32 interleaved, a uint8 guide,
Gaussian tables, one round, at R = 2 and R = 7 -- WARM + CALLS calls each.  Run under `rocprofv3
--kernel-trace --stats -- python tools/filter_time.py`: the kernels of the two radii are two template
instances, so the statistics list them apart.  The flow is a wavy field of a few pixels plus N(0,
0.25^2) px of noise, what a solver returns before it is filtered; the guide two grey levels in
stripes plus noise.  For context only it also prints the wall time of scipy.ndimage.median_filter
(the unweighted median, on the CPU) on the same field.
usage: python tools/filter_time.py [--w 640 --h 480] [--warm 3 --calls 10] [--radii 2 7] [--no-scipy]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "optical-flow-optimal-transport_amd"))
from foto import device as D  # noqa: E402
from foto import filter as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--w", type=int, default=640)
ap.add_argument("--h", type=int, default=480)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--radii", type=int, nargs="+", default=[2, 7])
ap.add_argument("--no-scipy", action="store_true")
A = ap.parse_args()
w, h = A.w, A.h

rng = np.random.default_rng(0)
jj, ii = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
u = 3.0 * np.sin(ii / 40) * np.cos(jj / 50) + 0.25 * rng.standard_normal((h, w))
v = 2.0 * np.cos(ii / 45) * np.sin(jj / 35) + 0.25 * rng.standard_normal((h, w))
flow = np.ascontiguousarray(np.stack([u, v], axis=-1).astype(np.float32))
guide = np.clip(np.where((ii + jj) % 64 < 32, 70, 170) + rng.integers(-25, 26, (h, w)), 0, 255).astype(np.uint8)

d, g = D.DeviceArray.from_numpy(flow), D.DeviceArray.from_numpy(guide)
out = D.DeviceArray((h, w, 2), np.float32)
valid, table = D.DeviceArray((h, w), np.uint8), D.DeviceArray((4,), np.float64)
for R in A.radii:
    sp, rg = F.tables(R, sigma_s=float(R), sigma_r=0.08)
    t0 = time.perf_counter()
    for _ in range(A.warm + A.calls):
        F.median(d, in_layout="interleaved", guide=g, radius=R, spatial=sp, range=rg, out=out, valid_out=valid, table_out=table)
    counts = table.to_numpy()          # (the download waits for the last call)
    dt = (time.perf_counter() - t0) / (A.warm + A.calls)
    moved = np.count_nonzero(out.to_numpy() != flow)
    print(f"R = {R}: {A.warm + A.calls} calls of {w} x {h}, {1e6 * dt:.0f} us per call of host wall time (launch included); "
          f"counts {[int(c) for c in counts]}; {moved} of {2 * w * h} values changed")

if not A.no_scipy:
    import scipy.ndimage as ndi
    for R in A.radii:
        t0 = time.perf_counter()
        ndi.median_filter(flow[..., 0], size=2 * R + 1)
        ndi.median_filter(flow[..., 1], size=2 * R + 1)
        print(f"scipy.ndimage.median_filter, size {2 * R + 1}, u and v on the CPU: {1e3 * (time.perf_counter() - t0):.1f} ms")
