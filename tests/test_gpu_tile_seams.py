"""The tiled Benamou-Brenier kernels (csrc/foto_kernels.hip) at tile seams and on interior tiles.

Three tiled families carry the outer iteration: the stencil march (64 x 4 tiles: k_apply_A, the
Laplacian, the stencil-CG kernels), k_rhs (64 x 1 tiles, chunks of 8 planes) and the fused
k_prox_rhs (64 x 8 tiles plus rings, chunks of FOTO_PR_TCH = 16 planes), whose INTERIOR
instantiation -- the march without bound tests -- runs on every tile with x0 >= 2, x0 + 66 <= Nx,
y0 >= 2, y0 + 10 <= Ny: 130 x 18 is the smallest plane that has one.  All three map blocks to
tiles through xcd_tile, a bijection only if its per / rem arithmetic is right for the block
count mod 8.  The goldens stop at Nx <= 64 (one tile column); the grids here are the smallest
with x seams, chunk seams, interior tiles and every kind of block count.

1. Exact stencils.  With integer-coded inputs (phi, w in [-2^20, 2^20); mu, q in [-2^16, 2^16);
   rho0, rhoT in [0, 2^16); r = 2, eps = 1/4) every intermediate of grad_st, div_st, the
   Laplacian, A and the RHS is a multiple of 1/2 below 2^25 in magnitude: exact in float64 in
   any operation order, so the kernels must equal the oracle bit for bit and a wrong neighbour
   cannot hide in rounding.  test_exactness_precondition (no GPU) proves that against an int64
   restatement for these very inputs.
2. k_prox_rhs against k_prox + k_rhs (FOTO_FUSE_PR=0), bit for bit, on grids with 0, 1 and 4
   interior tiles, single-shard and on time-slab shards (k_prox_rhs<EDGE> with INTERIOR).
3. The same fused runs against code the fused kernel does not share: q and mu against
   ops.stepB on ops.grad_st (pinned exactly at these widths by 1.), and the next phi -- the only
   place the never-stored F of the fused kernel shows -- against the oracle's own RHS and CG.
"""
import numpy as np
import pytest

from oracle import foto_oracle as O

from foto import ops  # noqa: E402  (importing the package does not load the library)
from foto.bb import BBSolver  # noqa: E402
from foto.synthetic import textured_pair, translating_gaussian  # noqa: E402

gpu = pytest.mark.gpu

TX, TY = 64, 4          # march tile (foto_internal.h)
PR_X, PR_Y = 64, 8      # k_prox_rhs tile


def march_blocks(Nx, Ny):
    return -(-Nx // TX) * -(-Ny // TY)


def interior_tiles(Nx, Ny):
    """Tiles of k_prox_rhs that take its INTERIOR body: the 64 x 8 tile at (x0, y0) plus its
    two-voxel phi ring lies inside the plane (the predicate in k_prox_rhs, foto_kernels.hip)."""
    return sum(1 for y0 in range(0, Ny, PR_Y) for x0 in range(0, Nx, PR_X)
               if x0 >= 2 and x0 + PR_X + 2 <= Nx and y0 >= 2 and y0 + PR_Y + 2 <= Ny)


# (Nt, Ny, Nx): what the grid adds
SEAM_GRIDS = [
    (2, 2, 65),      # a 1-wide last tile
    (3, 5, 64),      # exactly one tile column, two tile rows
    (3, 5, 66),
    (2, 9, 129),     # 9 march blocks: xcd_tile remainder 1
    (3, 18, 130),    # 15 blocks: remainder 7
    (4, 13, 200),    # 16 blocks: a multiple of 8
    (9, 4, 127),     # one k_rhs chunk seam at plane 8, a 1-plane last chunk
    (17, 3, 70),     # two chunk seams
]
R_EXACT, EPS_EXACT = 2.0, 0.25


def _seam_id(g):
    Nt, Ny, Nx = g
    return f"{Nt}x{Ny}x{Nx}-blocks{march_blocks(Nx, Ny)}"


def integer_inputs(Nt, Ny, Nx):
    """The integer-coded fields of a grid, as int64 (the float64 copies are exact)."""
    rng = np.random.default_rng(1000003 * Nt + 1009 * Ny + Nx)
    N, nxy = Nt * Ny * Nx, Ny * Nx
    return dict(phi=rng.integers(-2 ** 20, 2 ** 20, N), w=rng.integers(-2 ** 20, 2 ** 20, 3 * N),
                mu=rng.integers(-2 ** 16, 2 ** 16, 3 * N), q=rng.integers(-2 ** 16, 2 ** 16, 3 * N),
                rho0=rng.integers(0, 2 ** 16, nxy), rhoT=rng.integers(0, 2 ** 16, nxy))


def oracle_results(Nt, Ny, Nx):
    d = {k: v.astype(np.float64) for k, v in integer_inputs(Nt, Ny, Nx).items()}
    return dict(grad=O.grad_st(d["phi"], Nt, Ny, Nx), div=O.div_st(d["w"], Nt, Ny, Nx),
                lap=O.apply_laplacian_st(d["phi"], Nt, Ny, Nx),
                A=O.apply_A(d["phi"], R_EXACT, EPS_EXACT, Nt, Ny, Nx),
                rhs=O.bb_rhs(d["mu"], d["q"], d["rho0"], d["rhoT"], R_EXACT, Nt, Ny, Nx))


# ---- int64 restatement, in units of 1/2 (every function returns twice the operator's value)

def _d1_x2(z, axis):
    z = np.moveaxis(z, axis, 0)
    out = np.empty_like(z)
    out[1:-1] = z[2:] - z[:-2]
    out[0] = 2 * (z[1] - z[0])
    out[-1] = 2 * (z[-1] - z[-2])
    return np.moveaxis(out, 0, axis)


def _lap1(z, axis):
    z = np.moveaxis(z, axis, 0)
    out = np.empty_like(z)
    out[1:-1] = z[:-2] - 2 * z[1:-1] + z[2:]
    out[0] = z[1] - z[0]
    out[-1] = z[-2] - z[-1]
    return np.moveaxis(out, 0, axis)


def _div_x2(w, Nt, Ny, Nx):
    wt, wx, wy = w.reshape(3, Nt, Ny, Nx)
    return _d1_x2(wt, 0) + _d1_x2(wx, 2) + _d1_x2(wy, 1)


def int64_results_x2(Nt, Ny, Nx):
    d = integer_inputs(Nt, Ny, Nx)
    assert all(v.dtype == np.int64 for v in d.values())
    P = d["phi"].reshape(Nt, Ny, Nx)
    lap = _lap1(P, 0) + _lap1(P, 1) + _lap1(P, 2)
    r = int(R_EXACT)
    assert r == R_EXACT and 2 * R_EXACT * EPS_EXACT == 1.0
    F2 = _div_x2(d["mu"] - r * d["q"], Nt, Ny, Nx)
    mut, qt = d["mu"][:Nt * Ny * Nx].reshape(Nt, Ny, Nx), d["q"][:Nt * Ny * Nx].reshape(Nt, Ny, Nx)
    F2[0] -= 2 * (d["rho0"].reshape(Ny, Nx) - mut[0] + r * qt[0])
    F2[-1] += 2 * (d["rhoT"].reshape(Ny, Nx) - mut[-1] + r * qt[-1])
    return dict(grad=np.concatenate([_d1_x2(P, 0).ravel(), _d1_x2(P, 2).ravel(), _d1_x2(P, 1).ravel()]),
                div=_div_x2(d["w"], Nt, Ny, Nx).ravel(), lap=2 * lap.ravel(),
                A=(-2 * r * lap + P).ravel(),          # 2 (-r L + r eps I), 2 r eps = 1
                rhs=F2.ravel())


@pytest.mark.parametrize("grid", SEAM_GRIDS, ids=_seam_id)
def test_exactness_precondition(grid):
    """The oracle on the integer-coded inputs is exact: twice its float64 result equals the int64
    restatement, and nothing comes near 2^53.  So the array_equal assertions of
    test_exact_stencils cannot be excused by rounding or operation order."""
    want = int64_results_x2(*grid)
    got = oracle_results(*grid)
    for k in ("grad", "div", "lap", "A", "rhs"):
        assert np.abs(want[k]).max() < 2 ** 40, k
        assert np.array_equal(2.0 * got[k], want[k].astype(np.float64)), k
        assert np.any(want[k] % 2 != 0) or k == "lap"   # half-integers do occur


def test_grid_claims():
    """What the docstrings and ids claim of the grids: interior-tile counts of k_prox_rhs, the
    march block counts and the xcd_tile remainders they reach."""
    assert [interior_tiles(Nx, Ny) for Ny, Nx in ((18, 130), (17, 130), (18, 129), (27, 195))] == [1, 0, 0, 4]
    assert interior_tiles(129, 17) == 0 and interior_tiles(64, 64) == 0 and interior_tiles(640, 480) > 0
    counts = [march_blocks(Nx, Ny) for _, Ny, Nx in SEAM_GRIDS]
    assert counts == [2, 2, 4, 9, 15, 16, 2, 2]
    assert {c % 8 for c in counts} >= {0, 1, 7} and min(counts) < 8
    assert 195 % PR_X == 3 and 27 % PR_Y == 3       # the last tile of 195 x 27 is 3 wide, 3 high


# ---------------------------------------------------------------- 1. exact stencils

@gpu
@pytest.mark.parametrize("grid", SEAM_GRIDS, ids=_seam_id)
def test_exact_stencils(grid):
    """grad_st, div_st, the Laplacian and A (the march) and the RHS (k_rhs) equal the oracle bit
    for bit on the integer-coded inputs: every voxel, so every tile seam, chunk seam and block
    of xcd_tile's map (a skipped tile leaves its voxels unwritten, a doubled one leaves another's)."""
    Nt, Ny, Nx = grid
    d = {k: v.astype(np.float64) for k, v in integer_inputs(Nt, Ny, Nx).items()}
    ref = oracle_results(Nt, Ny, Nx)
    got = dict(grad=ops.grad_st(d["phi"], Nt, Nx, Ny), div=ops.div_st(d["w"], Nt, Nx, Ny),
               lap=ops.laplacian_st(d["phi"], Nt, Nx, Ny),
               A=ops.apply_A(d["phi"], Nt, Nx, Ny, R_EXACT, EPS_EXACT),
               rhs=ops.bb_rhs(d["mu"], d["q"], d["rho0"], d["rhoT"], R_EXACT, Nt, Nx, Ny))
    for k in ("grad", "div", "lap", "A", "rhs"):
        bad = np.flatnonzero(got[k] != ref[k])
        n = Nt * Ny * Nx
        where = [(int(i // n), int(i % n // (Ny * Nx)), int(i % (Ny * Nx) // Nx), int(i % Nx)) for i in bad[:5]]
        assert np.array_equal(got[k], ref[k]), f"{k}: {bad.size} voxels differ, first (field, t, y, x) {where}"


@gpu
def test_stencil_cg_across_seams():
    """Five iterations of the stencil CG (its march kernels k_cg_dir / k_cg_upd) on 130 x 18 x 3,
    15 blocks, against the oracle's CG on the assembled matrix, at test_cg's 5-iteration bar."""
    Nt, Ny, Nx, r, eps = 3, 18, 130, 1.0, 1e-2
    b = np.random.default_rng(130).standard_normal(Nt * Ny * Nx)
    x, info, its = ops.cg(b, Nt, Nx, Ny, r, eps, 1e-6, 5, 0)
    ref, info_o, its_o = O.cg(O.assemble_A(r, eps, Nt, Ny, Nx).dot, b, 1e-6, 5)
    assert (info, its) == (info_o, its_o) == (5, 5)
    print(f"stencil CG 5 its: max|x - ref| / max|ref| = {np.abs(x - ref).max() / np.abs(ref).max():.2e}")
    np.testing.assert_allclose(x, ref, rtol=0, atol=1e-10 * np.abs(ref).max())


# ---------------------------------------------------------------- 2. fused against separate

R, EPS = 1.0, 1e-2
_PR_ENV = ("FOTO_FUSE_PR", "FOTO_PR_TCH", "FOTO_PR_EDGE")


def _pair(kind, Nx, Ny):
    return translating_gaussian(Nx, Ny) if kind == "gauss" else textured_pair(Nx, Ny, seed=3, dx=1.5, dy=0.5)


def _setenv(monkeypatch, env):
    for k in _PR_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _run(rho0, rhoT, Nt, Ny, Nx, mode, vr=1):
    """Three outer iterations one at a time, then two in one call."""
    with BBSolver(rho0, rhoT, Nt, Nx, Ny, r=R, reg_epsilon=EPS, cg_mode=mode, virtual_ranks=vr) as s:
        for _ in range(3):
            s.iterate(1, 0.0, False)
        mu3, q3 = s.state()
        phi3 = s.phi()
        s.iterate(2, 0.0, False)
        mu, q = s.state()
        return np.array(s.crit), list(s.cg_its), (mu3, q3, phi3, mu, q, s.phi()) + tuple(s.flow())


def _compare(sep, fused, exact, crit_rtol):
    assert sep[1] == fused[1]                      # CG counts
    np.testing.assert_allclose(fused[0], sep[0], rtol=crit_rtol, atol=0)
    names = ("mu@3", "q@3", "phi@3", "mu", "q", "phi", "u", "v", "m")
    for name, x, y in zip(names, sep[2], fused[2]):
        if exact:
            bad = np.flatnonzero(x != y)
            assert np.array_equal(x, y), f"{name}: {bad.size} values differ, first flat indices {bad[:5]}"
        else:
            np.testing.assert_allclose(y, x, rtol=0, atol=1e-10 * max(np.abs(x).max(), 1e-300), err_msg=name)


FUSED_CASES = [
    # Nt, Ny, Nx, input, FOTO_PR_TCH
    (3, 18, 130, "tex", None),     # exactly one interior tile
    (3, 17, 130, "tex", None),     # none: the y edge of the predicate
    (3, 18, 129, "tex", None),     # none: the x edge
    (4, 27, 195, "tex", None),     # four interior tiles adjoining in x and y; a 3 x 3 last tile
    (2, 18, 130, "tex", None),     # the smallest Nt
    (17, 18, 130, "tex", None),    # the default 16-plane chunk: a seam at plane 16 in an interior tile
    (3, 18, 130, "tex", "1"),      # a chunk seam at every plane
    (3, 18, 130, "gauss", None),   # vacuum: the mu_t >= 0 clamp
]


def _fused_id(c):
    Nt, Ny, Nx, kind, tch = c
    return f"{Nt}x{Ny}x{Nx}-{kind}-interior{interior_tiles(Nx, Ny)}" + (f"-tch{tch}" if tch else "")


@gpu
@pytest.mark.parametrize("case", FUSED_CASES, ids=_fused_id)
def test_fused_matches_separate_with_interior_tiles(monkeypatch, case):
    """k_prox_rhs (tile, ring, INTERIOR and bounded bodies side by side) against k_prox + k_rhs
    with the spectral s-step CG: b.b comes from b^, so every iterate is bit-identical; only the
    crit sums are grouped differently (1e-13)."""
    Nt, Ny, Nx, kind, tch = case
    rho0, rhoT = _pair(kind, Nx, Ny)
    _setenv(monkeypatch, {"FOTO_FUSE_PR": "0"})
    sep = _run(rho0, rhoT, Nt, Ny, Nx, 2)
    _setenv(monkeypatch, {"FOTO_FUSE_PR": "1", **({"FOTO_PR_TCH": tch} if tch else {})})
    fused = _run(rho0, rhoT, Nt, Ny, Nx, 2)
    _compare(sep, fused, True, 1e-13)


@gpu
@pytest.mark.parametrize("mode", [0, 3])
@pytest.mark.parametrize("grid", [(3, 18, 130), (4, 27, 195)], ids=lambda g: "x".join(map(str, g)))
def test_fused_matches_separate_other_modes(monkeypatch, grid, mode):
    """The same with the stencil CG and the Gauss-compressed CG, at the bars these modes have in
    test_bb_fused_prox_rhs_matches_separate (F.F is summed in another order: CG rounding only)."""
    Nt, Ny, Nx = grid
    rho0, rhoT = _pair("tex", Nx, Ny)
    _setenv(monkeypatch, {"FOTO_FUSE_PR": "0"})
    sep = _run(rho0, rhoT, Nt, Ny, Nx, mode)
    _setenv(monkeypatch, {"FOTO_FUSE_PR": "1"})
    fused = _run(rho0, rhoT, Nt, Ny, Nx, mode)
    _compare(sep, fused, False, 1e-10)


@gpu
@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("vr", [2, 3, 5])
def test_fused_sharded_with_interior_tile(monkeypatch, vr, mode):
    """130 x 18 x 6 on vr time slabs: k_prox_rhs<EDGE=true> (deferred edges, the default) and the
    recomputed edges (FOTO_PR_EDGE=0), each with the INTERIOR body on the middle tile, against
    the separate kernels at test_bb_fused_prox_rhs_sharded's bars: CG counts equal, mu, q, phi
    and the flow bit-identical, crit to 1e-13 relative."""
    Nt, Ny, Nx = 6, 18, 130
    rho0, rhoT = _pair("tex", Nx, Ny)
    out = []
    for env in ({"FOTO_FUSE_PR": "0"}, {"FOTO_FUSE_PR": "1"}, {"FOTO_FUSE_PR": "1", "FOTO_PR_EDGE": "0"}):
        _setenv(monkeypatch, env)
        with BBSolver(rho0, rhoT, Nt, Nx, Ny, r=R, reg_epsilon=EPS, cg_mode=mode, virtual_ranks=vr) as s:
            s.iterate(4, 0.0, False)
            out.append((s.state(), s.phi(), list(s.cg_its), np.array(s.crit), s.flow()))
    _setenv(monkeypatch, {})
    (mu0, q0), p0, its0, crit0, f0 = out[0]
    for (mu1, q1), p1, its1, crit1, f1 in out[1:]:
        assert its0 == its1
        np.testing.assert_allclose(crit1, crit0, rtol=1e-13, atol=0)
        for x, y in ((mu0, mu1), (q0, q1), (p0, p1)) + tuple(zip(f0, f1)):
            assert np.array_equal(x, y)


# ---------------------------------------------------------------- 3. fused against independent code

@gpu
@pytest.mark.parametrize("grid", [(3, 18, 130), (4, 27, 195)],
                         ids=lambda g: "x".join(map(str, g)) + f"-interior{interior_tiles(g[2], g[1])}")
def test_fused_against_independent_references(monkeypatch, grid):
    """Bit-identity to the separate kernels says nothing of code the two share.  After each of
    three single fused iterations (mode 2): q and mu by test_inlined_sites_compute_stepB's
    recipe -- q == stepB(g + mu_prev / r), mu == mu_prev + r (g - q) with the t block clamped at
    0, g = ops.grad_st(phi) (exact at these widths: test_exact_stencils) -- and the NEXT phi
    against the oracle's own step from that (mu, q): O.bb_rhs and O.cg on the assembled matrix,
    at test_cg's bars (CG count +-1, 5e-8 max|phi|).  F of the fused kernel is never stored;
    phi is where its ring voxels show: one wrong F entry at a tile edge moves phi by orders more
    than that bar.  The first phi comes from k_rhs on the initial state, not from the fused
    kernel: its figures are printed, and q and mu after it are held to the recipe like the rest.
    Measured on an MI355X: the three phi that follow a fused F have the oracle's CG count and
    are within 8.3e-15 max|phi| of it on both grids.  The first phi: 2.1e-8 at equal counts on
    195 x 27 x 4; on 130 x 18 x 3 the kernel stops at 196 iterations where the oracle stops at
    195, one CG step at the rtol threshold, 2.1e-7 (4.5e-8 against the oracle's iterate 196)."""
    Nt, Ny, Nx = grid
    N = Nt * Ny * Nx
    rho0, rhoT = _pair("tex", Nx, Ny)
    A = O.assemble_A(R, EPS, Nt, Ny, Nx)
    _setenv(monkeypatch, {"FOTO_FUSE_PR": "1"})
    phi_bad = []
    with BBSolver(rho0, rhoT, Nt, Nx, Ny, r=R, reg_epsilon=EPS, cg_mode=2) as s:
        mu_prev, q_prev = s.state()
        for it in range(4):   # the fourth only for the phi that the third iteration's F gives
            want_phi, info, its = O.solve_step(mu_prev, q_prev, rho0, rhoT, R, A.dot, Nt, Ny, Nx)
            s.iterate(1, 0.0, False)
            phi, k = s.phi(), s.cg_its[-1]
            top = np.abs(want_phi).max()
            err = np.abs(phi - want_phi).max() / top
            # (for the record only: the oracle's iterate after the kernel's own count)
            same = O.cg(A.dot, O.bb_rhs(mu_prev, q_prev, rho0, rhoT, R, Nt, Ny, Nx), 0.0, k)[0]
            print(f"{grid} it {it}: CG {k} (oracle {its}), max|phi - oracle| / max|phi| = {err:.2e}"
                  f" ({np.abs(phi - same).max() / top:.2e} against the oracle's iterate {k})")
            assert info == 0 and s.cg_info[-1] == 0
            if it > 0 and not (abs(k - its) <= 1 and err <= 5e-8):
                phi_bad.append((it, k, its, err))
            mu, q = s.state()
            g = ops.grad_st(phi, Nt, Nx, Ny)
            assert np.array_equal(q, ops.stepB(g + (1.0 / R) * mu_prev, N)), (it, "q")
            mu_want = mu_prev + R * (g - q)
            mu_want[:N] = np.maximum(mu_want[:N], 0)
            assert np.array_equal(mu, mu_want), (it, "mu")
            mu_prev, q_prev = mu, q
    assert not phi_bad, f"(iteration, CG count, oracle's, max|phi - oracle| / max|phi|): {phi_bad}"
