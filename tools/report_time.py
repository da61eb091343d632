"""The transport report (foto_bb_report_dev, one k_report launch on a one-shard context) timed with
HIP events at the bench grid, after ten outer iterations.

Algorithmic bytes: one read of rho, m1, m2 and phi, 32 B per voxel (the rho0 / rhoT planes and the
partials are noise next to them); the stencil neighbours are L1 / L2 hits, as in k_rhs, which moves
56 B per voxel with the same stencils.

Events are torch.cuda.Event on a side stream that is handed to the calls as their stream (the *_dev
stream contract orders the library's stream inside the pair); a measurement is the time of REPS
back-to-back calls between two events, divided by REPS; every run is printed, the best and the
median are reported.  The timed call is the C entry through ctypes with the pointer worked out
beforehand: the Python wrapper validates its argument on every call (runtime_check reads
/proc/self/maps), which would be all a stream-side measurement of it sees.  The host entry
(BBSolver.report: launch, one 64 Nt-byte copy, a synchronise) is timed with the host clock.
usage: python tools/report_time.py [--w 640 --h 480 --nt 32 --its 10] [--reps 20 --runs 7]"""
import argparse
import ctypes
import os
import sys
import time

import torch  # first: libfoto then binds to torch's HIP runtime
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "optical-flow-optimal-transport_amd"))
from foto import _lib, ops  # noqa: E402
from foto.bb import BBSolver  # noqa: E402
from foto.synthetic import textured_pair  # noqa: E402

HBM_PEAK_TBS = 8.0   # MI355X, vendor figure

ap = argparse.ArgumentParser()
ap.add_argument("--w", type=int, default=640)
ap.add_argument("--h", type=int, default=480)
ap.add_argument("--nt", type=int, default=32)
ap.add_argument("--its", type=int, default=10)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--check", action="store_true", help="compare with foto_report_from_state on the downloaded state")
A = ap.parse_args()
w, h, Nt = A.w, A.h, A.nt
side = torch.cuda.Stream()

f0, f1 = textured_pair(w, h, seed=0)
print(f"device: {torch.cuda.get_device_name(0)}; grid {w}x{h}x{Nt}, {A.its} outer iterations; "
      f"{A.reps} calls per measurement, {A.runs} runs")
with BBSolver(f0, f1, Nt, w, h) as s:
    s.iterate(A.its, stop_rules=False)
    s.sync()
    out = torch.empty((Nt, 8), dtype=torch.float64, device="cuda")
    with torch.cuda.stream(side):
        s.report_device(out=out, stream=side)
        side.synchronize()
        rep = s.report()
        same = np.array_equal(out.cpu().numpy().view(np.uint64), rep.table.view(np.uint64))
        print(f"report_device == report bit for bit: {same}; crit {rep.crit!r} (callback: {s.crit[-1]!r})")
        print(repr(rep))
        if A.check:
            ref = ops.report_from_state(s.state()[0], s.phi(), f0, f1, Nt, w, h)
            print(f"report == report_from_state(state) bit for bit: {np.array_equal(ref.view(np.uint64), rep.table.view(np.uint64))}")
        L, P = s._L, ctypes.c_void_p
        a = (s._ctx, P(out.data_ptr()), P(side.cuda_stream))
        call = lambda: _lib.check(L.foto_bb_report_dev(*a), L)   # noqa: E731
        call()
        call()
        us = []
        for _ in range(A.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            for _ in range(A.reps):
                call()
            e1.record(side)
            e1.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / A.reps)
    nbytes = 32.0 * Nt * w * h
    best, med = min(us), float(np.median(us))
    print("foto_bb_report_dev, us per call by run: " + ", ".join(f"{t:.1f}" for t in us))
    for name, t in (("best", best), ("median", med)):
        tbs = nbytes / t / 1e6
        print(f"{name}: {t:.1f} us per call; algorithmic {nbytes / 1e6:.1f} MB -> {tbs:.2f} TB/s, "
              f"{100 * tbs / HBM_PEAK_TBS:.0f} % of the {HBM_PEAK_TBS:g} TB/s HBM peak")
    host = []
    for _ in range(A.runs):
        t0 = time.perf_counter()
        for _ in range(A.reps):
            s.report()
        host.append(1e6 * (time.perf_counter() - t0) / A.reps)
    print(f"BBSolver.report (host entry, launch + copy + synchronise), host clock: best {min(host):.1f} us, "
          f"median {float(np.median(host)):.1f} us per call")
    t0 = time.perf_counter()
    s.iterate(20, stop_rules=False)
    s.sync()
    print(f"for orientation: one outer iteration {1e6 * (time.perf_counter() - t0) / 20:.1f} us (20 iterations, host clock)")
