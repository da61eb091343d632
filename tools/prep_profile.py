"""The frame-preparation kernels at a user's size, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d OUT -o prep -- python tools/prep_profile.py

Lanczos 1280x960 -> 640x480 for uint8 and float64 through both routes of the horizontal pass, the
640x480 pair normalisation and frame difference, REPS times each after a warm-up; then the same
calls timed on the host clock around a device synchronise, and PIL's Image.resize on this box's CPU
for context.  The bytes each pass must move are printed beside the times.
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "optical-flow-optimal-transport_amd")]

from foto import device as D  # noqa: E402
from foto import prep  # noqa: E402

W, H, OW, OH, REPS = 1280, 960, 640, 480, 50


def sync():
    D.DeviceArray.from_numpy(np.zeros(1)).to_numpy()   # a blocking copy on the null stream, which every call joins


def timed(fn):
    fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(REPS):
        fn()
    sync()
    return (time.perf_counter() - t0) / REPS * 1e6


def main():
    rng = np.random.default_rng(0)
    print(f"Lanczos {W}x{H} -> {OW}x{OH}, {REPS} calls each; bytes a pass must move: read its input once, write its output")
    for dtype in (np.uint8, np.float64):
        item = np.dtype(dtype).itemsize
        a = rng.integers(0, 256, (H, W)).astype(dtype)
        d = D.DeviceArray.from_numpy(a)
        out = D.DeviceArray((OH, OW), dtype)
        hb, vb = (W * H + OW * H) * item, (OW * H + OW * OH) * item
        for route in ("lds", "direct"):
            us = timed(lambda: prep.resize(d, (OW, OH), "lanczos", route=route, out=out))
            print(f"resize {np.dtype(dtype).name:8s} route {route:6s}: {us:8.1f} us per call (host clock, both passes); "
                  f"horizontal pass {hb} B, vertical pass {vb} B")
    f0 = D.DeviceArray.from_numpy(rng.integers(0, 256, (OH, OW), dtype=np.uint8))
    f1 = D.DeviceArray.from_numpy(rng.integers(0, 256, (OH, OW), dtype=np.uint8))
    o0, o1 = D.DeviceArray((OH, OW), np.uint8), D.DeviceArray((OH, OW), np.uint8)
    print(f"normalize_pair uint8 {OW}x{OH}: {timed(lambda: prep.normalize_pair(f0, f1, out0=o0, out1=o1)):8.1f} us per call "
          "(host clock; the call allocates, waits for its statistics and frees)")
    print(f"difference     uint8 {OW}x{OH}: {timed(lambda: prep.difference(f0, f1, out=o0)):8.1f} us per call (host clock)")
    try:
        import PIL
        from PIL import Image
    except ImportError:
        print("PIL: not installed")
        return
    for mode, dtype in (("L", np.uint8), ("F", np.float32)):
        im = Image.fromarray(rng.integers(0, 256, (H, W)).astype(dtype), mode)
        best = min(_pil(im) for _ in range(5))
        print(f"PIL {PIL.__version__} mode {mode} Image.resize LANCZOS on this CPU: "
              f"{best * 1e6:8.1f} us (best of 5)")


def _pil(im):
    from PIL import Image
    t0 = time.perf_counter()
    im.resize((OW, OH), Image.LANCZOS)
    return time.perf_counter() - t0


if __name__ == "__main__":
    main()
