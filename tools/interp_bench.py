"""Maps and in-betweens (foto_bb_maps_dev, foto_bb_interp_dev: k_maps, k_interp) timed with HIP
events, beside k_track's time per trajectory step on the same device as the yardstick.

Cases: 1 time (the middle, s = (Nt-1)/2) and 8 times (evenly spaced interior), inv_iters 6; maps
in float32; in-betweens of uint8 frames with 1 and 3 interleaved channels into uint8.  Every chain
is serial: a time s = n + theta costs Nt-1-n forward steps and inv_iters (n + [theta > 0]) rounds of
the inverse step, each one velocity sample (the twelve phi taps of traj_vel); the samples per pixel
of a call are printed, and the time per sample and pixel beside k_track's per step and point.

Events are torch.cuda.Event on a side stream that is handed to the calls as their stream; a
measurement is the time of REPS back-to-back calls between two events, divided by REPS, best of
RUNS.  The timed calls are the C entries through ctypes with the pointers worked out beforehand
(tools/track_bench.py has the reason).
usage: python tools/interp_bench.py [--w 640 --h 480 --nt 32 --its 3] [--reps 20 --runs 7]"""
import argparse
import ctypes
import os
import sys

import torch  # first: libfoto then binds to torch's HIP runtime
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "optical-flow-optimal-transport_amd"))
from foto import _lib  # noqa: E402
from foto import device as D  # noqa: E402
from foto.bb import BBSolver  # noqa: E402
from foto.synthetic import textured_pair  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--w", type=int, default=640)
ap.add_argument("--h", type=int, default=480)
ap.add_argument("--nt", type=int, default=32)
ap.add_argument("--its", type=int, default=3)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--inv-iters", type=int, default=6)
A = ap.parse_args()
w, h, Nt, IT = A.w, A.h, A.nt, A.inv_iters
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


def samples(T):
    """velocity samples per pixel of a call at the times T"""
    n = np.floor(T).astype(int)
    return int(np.sum((Nt - 1 - n) + IT * (n + (T > n))))


f0, f1 = textured_pair(w, h, seed=0)
print(f"device: {torch.cuda.get_device_name(0)}; grid {w}x{h}x{Nt}, {A.its} outer iterations, inv_iters {IT}; "
      f"{A.reps} calls per measurement, best of {A.runs}")
rng = np.random.default_rng(2)
with BBSolver(f0, f1, Nt, w, h) as s:
    s.iterate(A.its, stop_rules=False)
    s.sync()
    nxy = w * h
    L, P, st = s._L, ctypes.c_void_p, ctypes.c_void_p(side.cuda_stream)
    U8, F32 = _lib.FOTO_U8, _lib.FOTO_F32
    with torch.cuda.stream(side):
        jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        centres = torch.from_numpy(np.stack([ii.ravel(), jj.ravel()], axis=1).astype(np.float32)).cuda()
        rec = torch.empty((Nt - 1, nxy, 2), dtype=torch.float32, device="cuda")
        a = (s._ctx, P(centres.data_ptr()), F32, nxy, 1, P(rec.data_ptr()), F32, st)
        t_trk = best_us(lambda: _lib.check(L.foto_bb_track_dev(*a), L))
        per_step = 1e3 * t_trk / (Nt - 1) / nxy
        print(f"yardstick k_track, {nxy} pixel centres, all {Nt - 1} steps, float32: {t_trk:.1f} us, "
              f"{per_step:.4f} ns per step and point")
        del rec
        for K in (1, 8):
            T = np.array([0.5 * (Nt - 1)]) if K == 1 else np.linspace(0.0, Nt - 1.0, K + 2)[1:-1]
            ns = samples(T)
            out = torch.empty((K, 4, h, w), dtype=torch.float32, device="cuda")
            b = (s._ctx, _lib.dptr(T), K, IT, P(out.data_ptr()), F32, st)
            t = best_us(lambda: _lib.check(L.foto_bb_maps_dev(*b), L))
            print(f"maps_dev, {K} time(s), float32: {t:.1f} us; {ns} velocity samples per pixel, "
                  f"{1e3 * t / ns / nxy:.4f} ns per sample and pixel ({1e3 * t / ns / nxy / per_step:.2f} x k_track's step)")
            for C in (1, 3):
                shape = (h, w) if C == 1 else (h, w, C)
                c0 = torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8)).cuda()
                c1 = torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8)).cuda()
                i0, i1, C_, sc0, sc1, _, _ = D.interp_frames(c0, c1)
                img = torch.empty((K,) + shape, dtype=torch.uint8, device="cuda")
                c = (s._ctx, ctypes.byref(i0), ctypes.byref(i1), C_, sc0, sc1, _lib.dptr(T), K, IT, P(img.data_ptr()), U8, st)
                t = best_us(lambda: _lib.check(L.foto_bb_interp_dev(*c), L))
                print(f"interp_dev, {K} time(s), {C} channel(s), uint8 -> uint8: {t:.1f} us; "
                      f"{1e3 * t / ns / nxy:.4f} ns per sample and pixel")
                ends = torch.empty((2,) + shape, dtype=torch.uint8, device="cuda")
                s.interpolate(c0, c1, [0.0, Nt - 1.0], out=ends, stream=side)
                side.synchronize()
                print(f"    ends give the frames back: {bool(torch.equal(ends[0], c0) and torch.equal(ends[1], c1))}")
