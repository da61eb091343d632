"""The spectral plan's fallback paths, selected by their knobs.

FOTO_TCOL=0 (t axis by dct_pass with separate INIT / x^ passes), FOTO_RING=0 (register-fed s-step
pass), FOTO_DCT_FFT=0 (GEMM kernels on every axis) and FOTO_GQ_CGTAB=0 (k_gq_cg, then k_gq_qtab)
otherwise run only where a grid happens to fall outside the fast path (odd Nt, odd Nx).  Every
one of them goes through the plan's shared transform chain and pass loop, so each is pinned here
to the bars of the default path: the reference's golden C1 run for a single shard
(test_gpu_parity.py::test_bb_deferred_cg), the single-shard solve for two shards
(test_gpu_parity.py::test_bb_virtual_ranks_match_single).  The knobs are read when the context
is built, so they are set before the BBSolver is."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

foto = pytest.importorskip("foto")
from foto.bb import BBSolver  # noqa: E402

SINGLE = [
    (2, {"FOTO_TCOL": "0"}),
    (2, {"FOTO_RING": "0"}),
    (2, {"FOTO_DCT_FFT": "0"}),
    (2, {"FOTO_TCOL": "0", "FOTO_RING": "0", "FOTO_DCT_FFT": "0"}),
    (3, {"FOTO_GQ_CGTAB": "0"}),
    (3, {"FOTO_TCOL": "0"}),
    (3, {"FOTO_DCT_FFT": "0"}),
]

SHARDED = [
    (2, {"FOTO_RING": "0"}),   # no late plan: cg_plan runs after every pass
    (2, {"FOTO_TCOL": "0"}),   # cg_begin launches the INIT pass
    (3, {"FOTO_TCOL": "0"}),   # inv_t goes through k_gq_xhat + dct_pass
]


def _id(case):
    mode, env = case
    return f"mode{mode}-" + "-".join(f"{k[5:]}={v}" for k, v in env.items())


@pytest.mark.parametrize("case", SINGLE, ids=_id)
def test_bb_c1_fallback_path(gold, monkeypatch, case):
    """C1 (64x64x8) with the stop rules on: 46 outer iterations, CG counts within one of the
    golden's, crit to 1e-5 relative, flow to 1e-5 px."""
    mode, env = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = gold("bb_c1.npz")
    Nt, Ny, Nx = (int(v) for v in d["shape"])
    r, tol, eps, max_it = d["params"]
    with BBSolver(d["rho0"], d["rhoT"], Nt, Nx, Ny, r=r, reg_epsilon=eps, cg_mode=mode) as s:
        s.iterate(int(max_it), tol, True)
        crit, its, (u, v, m) = np.array(s.crit), np.array(s.cg_its), s.flow()
    n = min(len(crit), len(d["crit"]))
    print(f"C1 {_id(case)}: outer {len(crit)}, cg its diff max {np.max(np.abs(its[:n] - d['cg_its'][:n]))}, "
          f"crit rel {np.max(np.abs(crit[:n] - d['crit'][:n]) / d['crit'][:n]):.2e}, "
          f"flow {max(np.abs(a - b).max() for a, b in ((u, d['u']), (v, d['v']), (m, d['m']))):.2e} px")
    assert len(crit) == len(d["crit"]) == 46
    assert np.max(np.abs(its - d["cg_its"])) <= 1
    np.testing.assert_allclose(crit, d["crit"], rtol=1e-5, atol=0)
    for a, b in ((u, d["u"]), (v, d["v"]), (m, d["m"])):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-5)


@pytest.mark.parametrize("case", SHARDED, ids=_id)
def test_bb_two_shards_fallback_path(gold, monkeypatch, case):
    """Two in-process shards reproduce the single-shard solve with the same knob."""
    mode, env = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = gold("bb_tex.npz")
    Nt, Ny, Nx = (int(s) for s in d["shape"])
    r, tol, eps, max_it = d["params"]
    res = []
    for vr in (1, 2):
        with BBSolver(d["rho0"], d["rhoT"], Nt, Nx, Ny, r=r, reg_epsilon=eps, virtual_ranks=vr, cg_mode=mode) as s:
            s.iterate(int(max_it), tol, True)
            res.append((np.array(s.crit), np.array(s.cg_its), s.phi(), s.flow()))
    (c1, k1, p1, f1), (c2, k2, p2, f2) = res
    assert len(c1) == len(c2)
    print(f"two shards {_id(case)}: outer {len(c1)}, cg its diff max {np.max(np.abs(k1 - k2))}, "
          f"crit rel {np.max(np.abs(c2 - c1) / np.abs(c1)):.2e}, phi {np.abs(p2 - p1).max() / np.abs(p1).max():.2e}, "
          f"flow {max(np.abs(a - b).max() for a, b in zip(f1, f2)):.2e}")
    assert np.max(np.abs(k1 - k2)) <= 1
    np.testing.assert_allclose(c2, c1, rtol=1e-6)
    np.testing.assert_allclose(p2, p1, rtol=0, atol=1e-6 * np.abs(p1).max())
    for a, b in zip(f1, f2):
        np.testing.assert_allclose(b, a, rtol=0, atol=1e-6)
