"""The entropic-transport solver at a user's size, for a kernel trace, for HIP-event times and for
the cross-check against the Benamou-Brenier solver:

    rocprofv3 --kernel-trace --stats -d OUT -o sk --output-format csv -- python tools/sinkhorn_profile.py --trace --radius 16
    python tools/sinkhorn_profile.py            # wall time of a 100-iteration solve, both forms, R = 16 and 32
    python tools/sinkhorn_profile.py --bb       # BB's w2 beside w2, w2_debiased and the analytic value

640 x 480 frames (a translating Gaussian on a floor of 0.01), eps = 2.  Both forms of the
half-iteration run in one process: FOTO_SK_FUSED is read when a context is made.  --trace runs 100
iterations of each form at one radius (the kernel names tell the forms apart; the radii need a run
each).  Without it the solve is timed with HIP events (torch.cuda.Event on the null stream, which
every call joins) around REPS solves after a warm-up.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "optical-flow-optimal-transport_amd"), os.path.join(REPO, "tests")]

W, H, ITERS, REPS, EPS = 640, 480, 100, 40, 2.0


def contexts(radius):
    """(two-pass, fused) contexts with the frames set."""
    from foto import device as D
    from foto import sinkhorn
    from foto.synthetic import translating_gaussian
    f0, f1 = (D.DeviceArray.from_numpy(f.reshape(H, W) + 0.01) for f in translating_gaussian(W, H))
    out = []
    for fused in ("0", "1"):
        os.environ["FOTO_SK_FUSED"] = fused
        out.append(sinkhorn.Sinkhorn(W, H, EPS, radius).set_frames(f0, f1))
    del os.environ["FOTO_SK_FUSED"]
    return out


def trace(radius):
    import torch
    for s in contexts(radius):
        s.iterate(ITERS)
        s.flow()
        s.info_device()
    torch.cuda.synchronize()
    print(f"traced: {W} x {H}, R = {radius}, {ITERS} iterations of each form, one flow and one record each")


def wall():
    import torch
    for radius in (16, 32):
        two, fused = contexts(radius)
        for name, s in (("two-pass", two), ("fused", fused)):
            s.iterate(ITERS)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(REPS):
                s.iterate(ITERS)
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b) / REPS
            print(f"{W} x {H} R = {radius:2d} {name:8s}: {ms * 1e3:9.1f} us per {ITERS}-iteration solve, "
                  f"{ms * 1e3 / (2 * ITERS):7.2f} us per half-iteration (HIP events around {REPS} solves)")
        same = all(np.array_equal(x.to_numpy(), y.to_numpy()) for x, y in zip(two.scalings(), fused.scalings()))
        print(f"  the two forms give the same bits after {fused.info().iterations} iterations: {same}")


def bb():
    """The 64 x 48 translating Gaussian (a 6.4 px shift) with the reference run's BB parameters."""
    import torch  # noqa: F401  (before the first foto call: one HIP runtime per process)
    from foto import sinkhorn
    from foto.bb import BBSolver
    from foto.synthetic import translating_gaussian
    Nx, Ny, Nt = 64, 48, 16
    rho0, rhoT = translating_gaussian(Nx, Ny)
    mass = float(rho0.sum())
    with BBSolver(rho0, rhoT, Nt, Nx, Ny, r=1.0, reg_epsilon=1e-2, device=0) as s:
        s.iterate(200, 0.01, True)
        rep = s.report()
        u, v, m = s.flow()
        outer, crit = len(s.crit), s.crit[-1]
    bb_mean = (float((rho0 * u).sum() / mass), float((rho0 * v).sum() / mass))
    with sinkhorn.Sinkhorn(Nx, Ny, EPS, 16) as k:
        k.set_frames(rho0, rhoT).iterate(100)
        info = k.info()
        fl = k.flow(dtype="float64").to_numpy()
    d = sinkhorn.divergence(rho0.reshape(Ny, Nx), rhoT.reshape(Ny, Nx), eps=EPS, radius=16, iters=100)
    sk_mean = (float((rho0 * fl[0].ravel()).sum() / mass), float((rho0 * fl[1].ravel()).sum() / mass))
    r = np.sqrt(mass)
    print(f"64 x 48 translating Gaussian, mass {mass!r} (frame 1: {float(rhoT.sum())!r})")
    print(f"BB: Nt = {Nt}, r = 1, reg_epsilon = 1e-2, {outer} outer iterations, crit {crit:.3e}")
    print(f"Sinkhorn: eps = {EPS}, R = 16, 100 iterations, marginal error / mass {info.marginal_error / mass:.3e}")
    print("quantity                          value        / sqrt(mass)")
    for name, val in (("analytic 6.4 sqrt(mass)", 6.4 * r), ("BB report().w2", rep.w2), ("BB report().w2_dual", rep.w2_dual),
                      ("Sinkhorn w2 (sharp cost)", info.w2), ("Sinkhorn w2_debiased", d.w2_debiased)):
        print(f"{name:30s} {val:12.6f} {val / r:12.6f}")
    print(f"mass-weighted mean flow (u, v):  BB ({bb_mean[0]:.6f}, {bb_mean[1]:.6f})   "
          f"Sinkhorn ({sk_mean[0]:.6f}, {sk_mean[1]:.6f})   gap in u {bb_mean[0] - sk_mean[0]:.6f} px")


def main():
    args = sys.argv[1:]
    import torch  # noqa: F401  (before the first foto call: one HIP runtime per process)
    if "--trace" in args:
        trace(int(args[args.index("--radius") + 1]) if "--radius" in args else 16)
    elif "--bb" in args:
        bb()
    else:
        wall()


if __name__ == "__main__":
    main()
