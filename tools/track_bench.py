"""Point tracking (BBSolver.track_device, one k_track launch) timed with HIP events.

Dense:  M = Nx * Ny pixel centres, all steps, float32 -- against flow_path_device(layout=
        "interleaved", dtype="float32") of the same context, which produces the same numbers with
        two launches per step (k_traj + k_flow_record) and the positions through memory between
        them; the step itself, 12 loads, is the one function both kernels call.  The two results
        are compared bit for bit before anything is timed.
Sparse: M = 1 (what a call costs before its points do), M = 1024 and M = 10^6 random in-frame
        points, and the 10^6 sorted by the pixel they start in; all steps and last-only,
        microseconds per call; at 10^6 the effective bytes as well: per step one 8 B / point
        write plus the phi plane touched, and the points read once.

Events are torch.cuda.Event on a side stream that is handed to the calls as their stream (the
*_dev stream contract orders the library's stream inside the pair); a measurement is the time of
REPS back-to-back calls between two events, divided by REPS, best of RUNS.  The timed calls are
the C entries (foto_bb_track_dev, foto_bb_flow_path_dev) through ctypes with the pointers worked
out beforehand: the Python wrappers validate their arguments on every call (runtime_check reads
/proc/self/maps, about half a millisecond with torch loaded), which would be all a stream-side
measurement of them sees.
usage: python tools/track_bench.py [--w 640 --h 480 --nt 32 --its 3] [--reps 20 --runs 7]"""
import argparse
import ctypes
import os
import sys

import torch  # first: libfoto then binds to torch's HIP runtime
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "optical-flow-optimal-transport_amd"))
from foto import _lib  # noqa: E402
from foto.bb import BBSolver  # noqa: E402
from foto.synthetic import textured_pair  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--w", type=int, default=640)
ap.add_argument("--h", type=int, default=480)
ap.add_argument("--nt", type=int, default=32)
ap.add_argument("--its", type=int, default=3)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--runs", type=int, default=7)
A = ap.parse_args()
w, h, Nt = A.w, A.h, A.nt
side = torch.cuda.Stream()


def best_us(fn):
    """microseconds per call: REPS calls between two events on the side stream, best of RUNS"""
    fn()
    fn()
    best = float("inf")
    for _ in range(A.runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(side)
        for _ in range(A.reps):
            fn()
        b.record(side)
        b.synchronize()
        best = min(best, 1e3 * a.elapsed_time(b) / A.reps)
    return best


f0, f1 = textured_pair(w, h, seed=0)
print(f"device: {torch.cuda.get_device_name(0)}; grid {w}x{h}x{Nt}, {A.its} outer iterations; "
      f"{A.reps} calls per measurement, best of {A.runs}")
with BBSolver(f0, f1, Nt, w, h) as s:
    s.iterate(A.its, stop_rules=False)
    s.sync()
    nxy = w * h
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    centres = torch.from_numpy(np.stack([ii.ravel(), jj.ravel()], axis=1).astype(np.float32)).cuda()
    rec = torch.empty((Nt - 1, nxy, 2), dtype=torch.float32, device="cuda")
    path = torch.empty((Nt - 1, h, w, 2), dtype=torch.float32, device="cuda")
    with torch.cuda.stream(side):
        s.track_device(centres, out=rec, stream=side)
        s.flow_path_device(out=path, layout="interleaved", stream=side)
        side.synchronize()
        same = torch.equal(rec.view(torch.int32), path.view(Nt - 1, nxy, 2).view(torch.int32))
        print(f"dense: track_device == flow_path_device(interleaved) bit for bit: {same}")
        L, P, st, F32 = s._L, ctypes.c_void_p, ctypes.c_void_p(side.cuda_stream), _lib.FOTO_F32

        def c_track(pts, M, all_steps, out):
            a = (s._ctx, P(pts.data_ptr()), F32, M, all_steps, P(out.data_ptr()), F32, st)
            return lambda: _lib.check(L.foto_bb_track_dev(*a), L)

        b = (s._ctx, P(path.data_ptr()), F32, 1, st)
        t_path = best_us(lambda: _lib.check(L.foto_bb_flow_path_dev(*b), L))
        t_trk = best_us(c_track(centres, nxy, 1, rec))
        print(f"dense M = {nxy} float32 all steps: flow_path_device {t_path:.1f} us, track_device {t_trk:.1f} us, "
              f"ratio track / path {t_trk / t_path:.3f}")
        del rec, path
        rng = np.random.default_rng(1)
        # M = 1: what a call costs before its points do (two pointer look-ups, the two event pairs
        # of the stream contract, one launch of Nt - 1 dependent steps)
        for M, order in ((1, "random"), (1024, "random"), (10 ** 6, "random"), (10 ** 6, "sorted by pixel")):
            p = np.stack([rng.uniform(0, w - 1, M), rng.uniform(0, h - 1, M)], axis=1).astype(np.float32)
            if order != "random":
                p = p[np.lexsort((p[:, 0].astype(np.int64), p[:, 1].astype(np.int64)))]
            pts = torch.from_numpy(p).cuda()
            for all_steps in (True, False):
                R = Nt - 1 if all_steps else 1
                out = torch.empty((R, M, 2), dtype=torch.float32, device="cuda")
                t = best_us(c_track(pts, M, 1 if all_steps else 0, out))
                line = f"sparse M = {M} ({order}) float32 {'all steps' if all_steps else 'last only'}: {t:.1f} us"
                if M >= 10 ** 6:
                    nbytes = 8 * M + R * 8 * M + (Nt - 1) * 8 * nxy
                    line += f", effective {nbytes / 1e6:.1f} MB, {nbytes / t / 1e6:.3f} TB/s"
                print(line)
