"""The workloads of profiles/match_kernel_times.txt, for a run under `rocprofv3 --kernel-trace --stats`:
describe at 640 x 480 with 4096 points (K = 1 and K = 32), match at 4096 x 4096 and 16384 x 16384 on
random descriptors, gate off and gate on.  One workload per process (describe1, describe32, match4096,
match16384 on the command line), since the sizes share kernel names; REPS runs after one warm-up."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "optical-flow-optimal-transport_amd"))

from foto import match  # noqa: E402
from foto.device import DeviceArray  # noqa: E402
from foto.synthetic import textured_pair  # noqa: E402

REPS = 10


def main(what):
    rng = np.random.default_rng(0)
    w, h = 640, 480
    frame = DeviceArray.from_numpy(textured_pair(w, h, 0, 0, 0)[0].reshape(h, w))
    pts = DeviceArray.from_numpy(np.column_stack([rng.uniform(15, w - 16, 4096), rng.uniform(15, h - 16, 4096)])
                                 .astype(np.float32))
    if what.startswith("describe"):
        for _ in range(REPS + 1):
            out = match.describe(frame, pts, orientations=int(what[8:]))
        print(what, "described", int((out[1].to_numpy() == 0).sum()))
        return
    for n in (int(what[5:]),):
        sets = []
        for _ in range(2):
            d = DeviceArray.from_numpy(rng.integers(0, 2 ** 64, size=(n, 4), dtype=np.uint64))
            s = DeviceArray.from_numpy(np.zeros(n, np.uint8))
            p = DeviceArray.from_numpy(np.column_stack([rng.uniform(0, w, n), rng.uniform(0, h, n)]).astype(np.float32))
            sets.append((d, s, p))
        for gate in (0.0, 50.0):
            for _ in range(REPS + 1):
                out = match.match(*sets[0], *sets[1], max_disp=gate)
        print(n, "matched", int((out[2].to_numpy() == 0).sum()))


if __name__ == "__main__":
    main(sys.argv[1])
