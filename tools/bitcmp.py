#!/usr/bin/env python3
"""Bit-identity of two library builds on the bench grid: run as
    FOTO_LIB=a.so python tools/bitcmp.py save A.npz [Nt Nx Ny iters sharded_W cg_mode]
    FOTO_LIB=b.so python tools/bitcmp.py save B.npz ...
    python tools/bitcmp.py cmp A.npz B.npz
Saved: the BB solve (CG counts, crit, phi, flows), the flow outputs and the transport report of
the solved context, and a GN solve of an Nx x Ny pair with the multigrid and the block-Jacobi PCG."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "optical-flow-optimal-transport_amd"))
if sys.argv[1] == "cmp":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    same = sorted(a.files) == sorted(b.files) and all(np.array_equal(a[k], b[k]) for k in a.files)
    print("bit-identical" if same else "DIFFERENT",
          {k: float(np.max(np.abs(a[k].astype(np.float64) - b[k]))) for k in a.files if k in b.files})
    sys.exit(0 if same else 1)
from foto import evaluate, gn, render  # noqa: E402
from foto.bb import BBSolver  # noqa: E402
from foto.device import DeviceArray  # noqa: E402
from foto.synthetic import sinusoid_pair, translating_gaussian  # noqa: E402
Nt, Nx, Ny, iters, vr, cg_mode = (int(v) for v in (sys.argv[3:9] + ["32", "640", "480", "6", "1", "3"][len(sys.argv[3:9]):]))
rho0, rhoT = translating_gaussian(Nx, Ny)
with BBSolver(rho0, rhoT, Nt, Nx, Ny, r=1.0, reg_epsilon=1e-2, cg_mode=cg_mode, virtual_ranks=vr) as s:
    s.iterate(iters, 0.0, stop_rules=False)
    out = dict(cg=np.array(s.cg_its), crit=np.array(s.crit), phi=s.phi())
    # the flow outputs of the solved context (finite flows, finite starts in and around the frame)
    u, v, m = s.flow()
    assert all(np.isfinite(x).all() for x in (u, v, m))
    out.update(u=u, v=v, m=m)
    out["report"] = s.report().table
    out["path_f32_interleaved"] = s.flow_path_device(dtype="float32", layout="interleaved").to_numpy()
    out["path_f64_planar"] = s.flow_path_device(dtype="float64", layout="planar").to_numpy()
    rng = np.random.default_rng(7)
    pts = np.stack([rng.uniform(-3, Nx + 2, 4096), rng.uniform(-3, Ny + 2, 4096)], axis=1)
    out["track_f64"] = s.track_device(DeviceArray.from_numpy(pts), dtype="float64").to_numpy()
    out["track_f32"] = s.track_device(DeviceArray.from_numpy(pts.astype(np.float32)), dtype="float32").to_numpy()
    frame = rng.uniform(0, 1, Nx * Ny)
    out["warp_m"] = evaluate.warp(frame, u, v, Nx, Ny, m)
    out["warp"] = evaluate.warp(frame, u, v, Nx, Ny)
    src, fl = DeviceArray.from_numpy(frame.reshape(Ny, Nx)), s.flow_device(dtype="float64")
    out["render_u8"] = render.reconstruct(src, fl, dtype="uint8").to_numpy()
    out["render_f64"] = render.reconstruct(src, fl, dtype="float64").to_numpy()
# GN: the multigrid PCG (default), then the block-Jacobi PCG, whose three reductions per
# iteration are the plain last-block sums
f1, f2 = sinusoid_pair(Nx, Ny)
for mg in ("1", "0"):
    os.environ["FOTO_GN_MG"] = mg
    gu, gv, gm, info, its = gn.solve(f1, f2, Nx, Ny, 0.1, 0.2)
    out.update({f"gn_mg{mg}_u": gu, f"gn_mg{mg}_v": gv, f"gn_mg{mg}_m": gm, f"gn_mg{mg}_its": np.array([info, its])})
os.environ.pop("FOTO_GN_MG")
# GN, every launch structure: the three forms of test_gn_round5_forms_bit_identical and the
# block-Jacobi PCG, at the bench size and at 71x77 (three levels with odd extents, k_mg_ltail
# directly under the level-0 legs); a plan per call, as that test
FORMS = {"sep": dict(FOTO_GN_SETUP_FUSE="0", FOTO_GN_RECOMP="0", FOTO_GN_FOLD="0", FOTO_MG_LTAIL="0"),
         "fold": dict(FOTO_GN_SETUP_FUSE="1", FOTO_GN_RECOMP="1", FOTO_GN_FOLD="1", FOTO_MG_LTAIL="0"),
         "ltail": dict(FOTO_GN_SETUP_FUSE="1", FOTO_GN_RECOMP="1", FOTO_GN_FOLD="1", FOTO_MG_LTAIL="1"),
         "bj": dict(FOTO_GN_MG="0")}
for w, h in ((640, 480), (71, 77)):
    f1, f2 = sinusoid_pair(w, h)
    for key, env in FORMS.items():
        env = dict(env, FOTO_GN_PLAN_CACHE="0")
        os.environ.update(env)
        gu, gv, gm, info, its = gn.solve(f1, f2, w, h, 0.1, 0.2)
        for k in env:
            os.environ.pop(k)
        out.update({f"gn_{w}x{h}_{key}_uvm": np.stack([gu, gv, gm]), f"gn_{w}x{h}_{key}_its": np.array([info, its])})
np.savez(sys.argv[2], **out)
