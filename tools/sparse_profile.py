"""The sparse tracking entries at a user's size, for a kernel trace and for HIP-event times:

    rocprofv3 --kernel-trace --stats -d OUT -o sparse -- python tools/sparse_profile.py --trace
    python tools/sparse_profile.py

640x480 frames of foto.synthetic.textured_pair, the detector's and the tracker's defaults:
corners(max_count = 4096), set_frames, and track of the corners found and of M = 4096 points (the
corners, then a regular grid of further points: the defaults find fewer than 4096 corners on this
texture).  Without --trace every entry is timed with HIP events (torch.cuda.Event on the null
stream, which every call joins) around REPS calls after a warm-up, and the bytes and operations
each kernel must move / do are printed beside the times.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "optical-flow-optimal-transport_amd")]

W, H, M, REPS = 640, 480, 4096, 100


def main():
    trace = "--trace" in sys.argv[1:]
    import torch   # (before the first foto call: one HIP runtime per process)
    from foto import device as D
    from foto import sparse
    from foto.gn import pyramid_sizes
    from foto.synthetic import textured_pair

    f0, f1 = (D.DeviceArray.from_numpy(f.reshape(H, W)) for f in textured_pair(W, H))
    pts = D.DeviceArray((M, 2), np.float32)
    _, count = sparse.corners(f0, M, out=pts)
    host = pts.to_numpy()
    gx, gy = np.meshgrid(np.linspace(16, W - 17, 64), np.linspace(16, H - 17, 64))
    host[count:] = np.column_stack([gx.ravel(), gy.ravel()])[:M - count].astype(np.float32)
    full = D.DeviceArray.from_numpy(host)
    found = pts[:count]
    lk = sparse.LK(W, H).set_frames(f0, f1)
    sizes = [tuple(s) for s in pyramid_sizes(W, H, sparse.LK_DEFAULTS["levels"], sparse.LK_DEFAULTS["min_size"])]
    out = {n: (D.DeviceArray((n, 2), np.float32), D.DeviceArray((n,), np.uint8)) for n in (count, M)}

    def track(p):
        n = p.shape[0]
        return lambda: lk.track_raw(p, out=out[n][0], status=out[n][1], err=False)

    cnt = D.DeviceArray((4,), np.uint8)
    calls = [("corners(max_count=4096)", lambda: sparse.corners(f0, M, out=pts, wait=False, count_out=cnt)),
             ("set_frames", lambda: lk.set_frames(f0, f1)),
             (f"track M={count} (the corners)", track(found)),
             (f"track M={M}", track(full))]
    print(f"{W}x{H} textured_pair, defaults: {count} corners; pyramid {sizes}; {REPS} calls each")
    for name, fn in calls:
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
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
        print(f"{name:32s} {a.elapsed_time(b) / REPS * 1e3:9.1f} us per call (HIP events around {REPS} calls)")
    if trace:
        return
    n = W * H
    r = sparse.LK_DEFAULTS["radius"]
    win, iters = (2 * r + 1) ** 2, sparse.LK_DEFAULTS["iters"]
    c = sparse.CORNER_DEFAULTS["window"]
    print("counts from the shapes:")
    print(f"  k_corner_response: reads {8 * n} B, writes {8 * n} B; {3 * 2 * (2 * c + 1)} adds + 3 products + 1 sqrt per "
          f"pixel = {n * (6 * (2 * c + 1) + 12) / 1e6:.1f} Mflop")
    print(f"  k_corner_mark: reads {8 * n} B (+ the 11 x 11 window of the pixels over the threshold), writes {n} B")
    taps = sum(20 * win + iters * 4 * win for _ in sizes) + 4 * win
    print(f"  k_lk_track: per point {len(sizes)} levels x ({20 * win} template taps + {iters} x {4 * win} search taps) "
          f"+ {4 * win} = {taps} loads of 8 B from {sum(2 * 8 * a * b for a, b in sizes)} B of pyramids (cache-resident); "
          f"M = {M}: {taps * M * 8 / 1e6:.0f} MB of loads, {M * len(sizes) * (iters * 2 + 3)} wave sums")


if __name__ == "__main__":
    main()
