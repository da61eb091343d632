"""The plane march of k_prox_rhs (csrc/foto_kernels.hip, prox_rhs_body).

An iteration p of a chunk [l0, l1) runs stepB on plane p and F on plane p - 1.  The STEADY planes
[ps, pe] of a chunk run a copy of the iteration with every plane condition folded away (all loads
issued, four stores per own voxel, no boundary term), the first of them ahead of a loop of pairs
that alternates two register sets of mu; the planes before and after run the general iteration,
which skips the ring voxels and the w_x, w_y images on the planes l0 - 1 and l1.

1. The schedule, restated in Python (no GPU): every plane of every chunk is visited once and in
   order, and a steady plane satisfies what its folded conditions assume.
2. The fused kernel against k_prox + k_rhs (FOTO_FUSE_PR=0) with the spectral s-step CG, bit for
   bit, at the plane counts, chunk lengths and tile shapes where the march changes path.
"""
import numpy as np
import pytest

from foto.bb import BBSolver
from foto.synthetic import textured_pair, translating_gaussian

gpu = pytest.mark.gpu

PR_TCH = 16   # the default chunk (Tuning::pr_tch)


def chunk_schedule(Nt, tch, t0=0, nloc=None):
    """Per chunk the (plane, kind) list of prox_rhs_body's march, kind 'g' (general) or 's' (steady),
    with the chunk's (l0, l1, pz): the loop bounds of the kernel restated (EDGE = false)."""
    nloc = Nt if nloc is None else nloc
    tch = min(tch, nloc)
    out = []
    for ch in range(-(-nloc // tch)):
        l0, l1 = ch * tch, min(nloc, ch * tch + tch)
        pa, pz = max(l0 - 1, -t0), min(l1, Nt - 1 - t0)
        ps, pe = max(l0 + 1, 2 - t0), min(pz - 2, Nt - 4 - t0)
        p, seq = pa, []
        for part in range(2):
            last = min(ps - 1, l1) if part == 0 else l1
            while p <= last:
                seq.append((p, "g"))
                p += 1
            if part == 0 and p <= pe:
                seq.append((p, "s"))
                p += 1
                while p + 1 <= pe:
                    seq += [(p, "s"), (p + 1, "s")]
                    p += 2
        out.append((seq, (l0, l1, pa, pz)))
    return out


def _check_schedule(Nt, tch, t0=0, nloc=None):
    kinds = []
    for seq, (l0, l1, pa, pz) in chunk_schedule(Nt, tch, t0, nloc):
        assert [p for p, _ in seq] == list(range(pa, l1 + 1))          # once each, in order
        for p, kind in seq:
            if kind != "s":
                continue
            assert l0 <= p - 1 and p < l1                              # mu'(p) and F(p - 1) are stored
            assert 1 <= t0 + p - 1 <= Nt - 2                           # F(p - 1) has no boundary term
            assert 0 < t0 + p < Nt - 1                                 # stepB's t neighbours exist
            assert p + 1 <= pz                                         # mu(p + 1) is loaded
            assert p + 3 <= pz + 1 and 0 <= t0 + p + 3 < Nt            # phi(p + 3) is in the grid
        kinds.append("".join(k for _, k in seq))
    return kinds


def test_schedule_visits_every_plane_once_and_steady_planes_fold():
    for Nt in range(2, 70):
        for tch in (1, 2, 3, 4, 5, 8, 16, 32, 64):
            _check_schedule(Nt, tch)
    for t0 in (1, 3, 7):                       # recomputed-edge shards: planes below 0 are the halo's
        for nloc in range(1, 20):
            for Nt in range(t0 + nloc, t0 + nloc + 5):
                for tch in (1, 2, 3, 16):
                    _check_schedule(Nt, tch, t0, nloc)


def test_schedule_claims():
    """What the GPU cases below say they reach."""
    assert _check_schedule(32, PR_TCH) == ["gg" + 13 * "s" + "gg", "gg" + 11 * "s" + "ggggg"]   # the bench grid
    assert _check_schedule(2, PR_TCH) == ["ggg"] and _check_schedule(5, PR_TCH) == ["gggggg"]   # no steady plane
    assert _check_schedule(6, PR_TCH) == ["ggsgggg"]                                            # the first alone
    assert _check_schedule(17, PR_TCH) == ["gg" + 11 * "s" + "gggg", "ggg"]                     # ... and five pairs
    assert _check_schedule(33, PR_TCH)[2] == "ggg"                                              # a one-plane chunk
    assert all("s" not in k for t in (1, 2, 3) for k in _check_schedule(7, t))
    assert _check_schedule(9, PR_TCH) == ["ggsssggggg"]          # planes 2..5 could be steady: the fourth is general


# ---------------------------------------------------------------- fused against separate

R, EPS = 1.0, 1e-2
_PR_ENV = ("FOTO_FUSE_PR", "FOTO_PR_TCH", "FOTO_PR_EDGE")


def _setenv(monkeypatch, env):
    for k in _PR_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _run(rho0, rhoT, Nt, Ny, Nx):
    """Three outer iterations one at a time, then two in one call (cg_mode 2)."""
    with BBSolver(rho0, rhoT, Nt, Nx, Ny, r=R, reg_epsilon=EPS, cg_mode=2) as s:
        for _ in range(3):
            s.iterate(1, 0.0, False)
        mu3, q3 = s.state()
        phi3 = s.phi()
        s.iterate(2, 0.0, False)
        mu, q = s.state()
        return np.array(s.crit), list(s.cg_its), (mu3, q3, phi3, mu, q, s.phi()) + tuple(s.flow())


MARCH_CASES = [
    # Nt, Ny, Nx, input, FOTO_PR_TCH
    (2, 18, 130, "tex", None),     # fewer planes than the phi ring has slots
    (3, 18, 130, "tex", None),
    (5, 18, 130, "tex", None),     # the longest march with no steady plane
    (6, 18, 130, "tex", None),     # one steady plane: the one ahead of the loop of pairs
    (9, 18, 130, "tex", None),     # pairs, and a steady-able plane left to the general iteration
    (17, 18, 130, "tex", None),    # a seam at plane 16
    (33, 18, 130, "tex", None),    # a last chunk of one plane
    (7, 18, 130, "tex", "1"),      # chunks that are all head and tail
    (7, 18, 130, "tex", "2"),
    (7, 18, 130, "tex", "3"),
    (3, 18, 131, "tex", None),     # odd Nx
    (4, 19, 133, "tex", None),
    (4, 27, 195, "tex", None),     # interior tiles adjoining in x and y, plus a 3 x 3 remainder tile
    (9, 27, 195, "tex", None),     # ... with steady planes: the bounded tiles' copy of them too
    (3, 18, 130, "gauss", None),   # vacuum: the mu_t >= 0 clamp
]


def _march_id(c):
    Nt, Ny, Nx, kind, tch = c
    return f"{Nt}x{Ny}x{Nx}-{kind}" + (f"-tch{tch}" if tch else "")


@gpu
@pytest.mark.parametrize("case", MARCH_CASES, ids=_march_id)
def test_march_matches_separate_kernels(monkeypatch, case):
    """mu, q, phi and the flow after three single iterations and after two more: exactly equal;
    CG counts equal; crit to 1e-13 relative (its sums are grouped differently)."""
    Nt, Ny, Nx, kind, tch = case
    rho0, rhoT = translating_gaussian(Nx, Ny) if kind == "gauss" else textured_pair(Nx, Ny, seed=3, dx=1.5, dy=0.5)
    _setenv(monkeypatch, {"FOTO_FUSE_PR": "0"})
    sep = _run(rho0, rhoT, Nt, Ny, Nx)
    _setenv(monkeypatch, {"FOTO_FUSE_PR": "1", **({"FOTO_PR_TCH": tch} if tch else {})})
    fused = _run(rho0, rhoT, Nt, Ny, Nx)
    assert sep[1] == fused[1]
    np.testing.assert_allclose(fused[0], sep[0], rtol=1e-13, atol=0)
    for name, x, y in zip(("mu@3", "q@3", "phi@3", "mu", "q", "phi", "u", "v", "m"), sep[2], fused[2]):
        bad = np.flatnonzero(x != y)
        assert np.array_equal(x, y), f"{name}: {bad.size} values differ, first flat indices {bad[:5]}"
