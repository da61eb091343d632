"""The global-motion fit at a user's sizes, for a kernel trace and for HIP-event times:

    rocprofv3 --kernel-trace --stats -d OUT -o motion -- python tools/motion_profile.py --trace
    python tools/motion_profile.py

An affine model with 0.05 px of noise and 30 % of the correspondences displaced by up to 15 px, H =
256 hypotheses, the defaults otherwise: fit_flow on a 640 x 480 float32 flow at stride 1 (M =
307200) and fit on M = 2000 float32 tracks.  Without --trace each call is timed with HIP events
(torch.cuda.Event on the null stream, which every call joins) around REPS calls after a warm-up.
FOTO_LIB selects another build of the library (an A/B of the scoring kernel's shape).
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "optical-flow-optimal-transport_amd"), os.path.join(REPO, "tests")]

W, H, M_SPARSE, REPS = 640, 480, 2000, 50


def main():
    trace = "--trace" in sys.argv[1:]
    import torch   # (before the first foto call: one HIP runtime per process)
    import motion_ref as R
    from foto import device as D
    from foto import motion

    rng = np.random.default_rng(1)
    mt = R.true_matrix("affine", W, H, rng)
    u, v = R.field_uv(mt, W, H)
    bad = rng.random((H, W)) < 0.3
    u = u + rng.normal(0, 0.05, u.shape) + bad * rng.uniform(-15, 15, u.shape)
    v = v + rng.normal(0, 0.05, v.shape) + bad * rng.uniform(-15, 15, v.shape)
    flow = D.DeviceArray.from_numpy(np.stack([u, v, np.zeros_like(u)]).astype(np.float32))
    p, d, _, _, _ = R.synthetic("affine", W, H, M_SPARSE, 0.3, seed=2)
    pts, disp = (D.DeviceArray.from_numpy(a.astype(np.float32)) for a in (p, d))
    table = motion.samples(256, 0)
    calls = [(f"fit_flow {W}x{H} stride 1 (M = {W * H})", lambda: motion.fit_flow(flow, stride=1, samples=table)),
             (f"fit M = {M_SPARSE}", lambda: motion.fit(pts, disp, W, H, samples=table))]
    print(f"affine, H = {len(table)}, rounds {motion.DEFAULTS['rounds']}, library {os.environ.get('FOTO_LIB', 'default')}")
    for name, fn in calls:
        for _ in range(3):
            fit = fn()
        torch.cuda.synchronize()
        print(f"{name}: (inliers, valid, winner, status) = {fit.counts()}, rms {fit.rms():.4f}")
        if trace:
            for _ in range(REPS):
                fn()
            torch.cuda.synchronize()
            continue
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        torch.cuda.synchronize()
        print(f"{name:44s} {a.elapsed_time(b) / REPS * 1e3:9.1f} us per call (HIP events around {REPS} calls)")
    if not trace:
        n = W * H
        print("counts from the shapes:")
        print(f"  k_motion_score: reads {32 * n} B of the list once and {72 * len(table)} B of models per block; "
              f"{len(table)} x {n} evaluations of 21 flops = {21 * len(table) * n / 1e9:.2f} Gflop")
        print(f"  k_motion_accum (affine): reads {32 * n} B, 27 sums of {n} terms")


if __name__ == "__main__":
    main()
