"""project_K (csrc/foto_kernels.hip), the projection onto K = {a + |b|^2/2 <= 0}, against the
exact projection, and its five inlined sites against k_stepB.

Yardstick.  oracle/projk_exact.py computes the projection from its optimality conditions in
80-digit decimal; it shares no closed form with the kernel or with foto_oracle.stepB (the
float64 restatement of the reference).  With err_i = max_k |q - q_exact| and s_i = max(1,
|p_i|_inf), a regime's envelope is E_ref = max(2^-52, max over oracle-finite points of
err_i^oracle / s_i), formed at test time from the oracle alone.  The kernel must stay within
F * E_ref * s_i at EVERY point, F = 4: cbrt_pair is within 2-3 ulp of the rounded cube root
where the reference's pow is within one, and c - (a+1)/(3c) passes that through linearly.
tests/test_projk_exact_host.py checks the premises (reference residual, a second construction,
E_ref <= 2e-15 everywhere) on the CPU.

Regimes (oracle/projk_cases.py): N(0, 3^2); uniform scales 1e-12 ... 1e50 (1e50: cbrt_pair's
exponent split at e ~ 250); per-component mixed scales 10^U(-6, 6); points delta (1 + rho^2)
outside the boundary, delta down to 1e-13; points exactly on the boundary (bit-identical
output); the axis rho = 0 under all signs of the zeros; and the seam between the Cardano and the
trigonometric branch, 32 (a+1)^3 + 108 rho^2 = 0, 0 / 1 / 2 / 4 ulps and 1e-9 / 1e-3 relative to
either side.  Inputs from 1e100 upward are out of scope: the reference's own a^3 overflows.

The seam.  The reference's closed forms are NaN on 8-13 % of the points placed on the seam
(acos argument an ulp above 1; the expanded Cardano polynomial an ulp below 0).  Without the two
selects in project_K / proj_trig_z the kernel's are too -- on an MI355X 50 / 36 of the 301
axis-aligned / rotated points on the seam (34 / 26 of them where the oracle is finite), 25 / 24
one ulp above, 2 / 9 one ulp below, 1 / 5 two ulps above, none from four ulps -- and
test_envelope fails on those eight regimes.  With them every seam point is finite and inside
the envelope.

Measured on an MI355X, max over points of err_i / (E_ref s_i), bar F = 4:
  N(0, 3^2): 2.17 (M = 1999), 0.53 (M = 1), 2.41 (M = 255), 3.03 (M = 257; E_ref of 257 points
  is 3.1e-16, of 1999 points 4.8e-16); scales 1e-12 ... 1e50: 0.82 ... 1.26 (1e50: 1.00);
  mixed: 1.08; near the boundary: 1.37 / 1.89 / 1.80 (delta 1e-3 / 1e-8 / 1e-13); boundary: 0
  (identity); axis: 0.83; seam, all 22 regimes: 0.73 ... 2.80 (on the seam itself 1.66
  axis-aligned, 2.42 rotated).  E_ref is 2.8e-16 ... 8.1e-16 throughout.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

foto = pytest.importorskip("foto")
from foto import ops  # noqa: E402
from foto.bb import BBSolver  # noqa: E402
from foto.synthetic import textured_pair, translating_gaussian  # noqa: E402
from oracle import foto_oracle as O  # noqa: E402
from oracle import projk_cases as C  # noqa: E402
from oracle import projk_exact as X  # noqa: E402

F_BAR = 4.0
U = 2.0 ** -52
NAMES = sorted(C.regimes())


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _point_finite(q, M):
    return np.isfinite(np.asarray(q).reshape(3, M)).all(axis=0)


@pytest.mark.parametrize("name", NAMES)
def test_envelope(name):
    p, M, hi, lo, ins, _, qo = C.exact(name)
    q = ops.stepB(p, M)
    s = C.scale_of(p, M)
    # inside K: the input's bits, signed zeros included
    k = np.tile(ins, 3)
    assert np.array_equal(_bits(q)[k], _bits(p)[k])
    # the envelope, from the oracle alone
    fin_o = _point_finite(qo, M)
    err_o = X.point_error(qo, hi, lo, M)
    E_ref = max(U, float(np.max(err_o[fin_o] / s[fin_o])))
    err = X.point_error(q, hi, lo, M)
    nan = int(np.isnan(err).sum())
    ratio = float(np.max(np.where(np.isnan(err), np.inf, err) / (E_ref * s)))
    print(f"{name}: M {M}, inside {int(ins.sum())}, E_ref {E_ref:.3e}, oracle non-finite {int((~fin_o).sum())}, "
          f"kernel non-finite {nan}, kernel max err / (E_ref s) = {ratio:.3f}")
    assert nan == 0, f"{nan} non-finite outputs, {int((np.isnan(err) & fin_o).sum())} of them where the oracle is finite"
    assert ratio <= F_BAR
    # feasibility
    qa, q1, q2 = q[:M], q[M:2 * M], q[2 * M:]
    assert np.all(qa + 0.5 * (q1 * q1 + q2 * q2) <= 8 * U * np.maximum(1.0, np.abs(qa)))


def test_axis_signs_of_zero():
    """rho = 0, a > 0: p projects onto the apex (the values are test_envelope[axis]'s).  The
    reference forms rH (cos, sin)(atan2(b2, b1)) with atan2(+-0, +0) = +-0 and atan2(+-0, -0) =
    +-pi, and rH = sqrt2 (c - (a+1)/(3c)) is a rounding residue of either sign, or a zero.  So
    q1 = +-rH with b1's sign, and q2 = rH sin(.) has the sign of rH times b2's: a zero for b1 = +0;
    for b1 = -0 the reference's rH sin(+-pi) is rH * +-1.2e-16 where the kernel returns the zero
    of that sign.  rH's own sign hangs on the cube root's last bit, so the kernel is held to
    these relations, which the oracle is shown to satisfy, and to the oracle's bits of sign on
    every zero where both round rH to the same side."""
    p, M, _, _, _, _, qo = C.exact("axis")
    q = ops.stepB(p, M)
    b1, b2 = p[M:2 * M], p[2 * M:]
    for who, v in (("oracle", qo), ("kernel", q)):
        va, v1, v2 = v[:M], v[M:2 * M], v[2 * M:]
        rH_neg = np.signbit(v1) ^ np.signbit(b1)
        assert np.array_equal(np.signbit(v2), rH_neg ^ np.signbit(b2)), who
        assert np.all(v2[~np.signbit(b1)] == 0.0), who
        assert np.all(np.signbit(va)), who            # q_a = -(z^2): negative or -0, never +0
    assert np.all(q[2 * M:] == 0.0)
    same = np.tile(np.signbit(q[M:2 * M]) == np.signbit(qo[M:2 * M]), 3)
    zero = same & (qo == 0.0) & (q == 0.0)
    print(f"axis: rH rounds to the oracle's side on {int(same.sum()) // 3} of {M} points, {int(zero.sum())} common zeros")
    assert np.array_equal(np.signbit(q[zero]), np.signbit(qo[zero]))


def test_nonfinite_inputs():
    """NaN, +Inf, -Inf in single components: the set of points with a non-finite output is the
    oracle's, every other point keeps its bits, and (-Inf, b1, b2) -- inside K -- comes back
    as it is."""
    p0, M = C.regimes()["normal3"]
    clean = ops.stepB(p0, M)
    p = p0.copy()
    bad = {}
    vals = (np.nan, np.inf, -np.inf)
    for j, (comp, v) in enumerate((c, v) for c in range(3) for v in vals):
        for i in (3 + 17 * j, 256 + 5 * j, M - 1 - 31 * j):   # first block, a block edge, the tail
            p[comp * M + i] = v
            bad[i] = (comp, v)
    q = ops.stepB(p, M)
    with np.errstate(all="ignore"):
        qo = O.stepB(p, M)
    assert np.array_equal(_point_finite(q, M), _point_finite(qo, M))
    touched = np.zeros(M, dtype=bool)
    touched[list(bad)] = True
    keep = np.tile(~touched, 3)
    assert np.array_equal(_bits(q)[keep], _bits(clean)[keep])
    assert _point_finite(q, M)[~touched].all()
    for i, (comp, v) in bad.items():
        assert not _point_finite(q, M)[i]
        if comp == 0 and v == -np.inf:
            assert np.array_equal(_bits(q[i::M]), _bits(p[i::M]))


# ---------------------------------------------------------------- the inlined sites

def _grid(name, gold):
    if name == "2x2x2-gauss":
        return (2, 2, 2, 1.0, 1e-2) + translating_gaussian(2, 2)
    if name == "7x5x3-tex":
        return (7, 5, 3, 1.0, 1e-2) + textured_pair(7, 5)
    if name == "24x18x5-tex":
        d = gold("bb_tex.npz")
        Nt, Ny, Nx = (int(v) for v in d["shape"])
        r, _, eps, _ = d["params"]
        return Nx, Ny, Nt, float(r), float(eps), d["rho0"], d["rhoT"]
    return (40, 30, 20, 1.0, 1e-2) + translating_gaussian(40, 30)


CONTEXTS = {
    "separate": ({"FOTO_FUSE_PR": "0"}, 1),               # k_prox stores q
    "fused": ({}, 1),                                      # k_prox_rhs tile + ring; q by k_q_from_phi
    "fused-tch1": ({"FOTO_PR_TCH": "1"}, 1),               # a chunk seam at every plane
    "one-in-flight": ({"FOTO_PIPE": "0"}, 1),
    "sharded": ({}, 3),                                    # deferred slab edges: k_wt_pre
}
SITES = [(g, c) for g in ("2x2x2-gauss", "7x5x3-tex", "24x18x5-tex", "40x30x20-gauss") for c in CONTEXTS
         if c != "sharded" or g in ("24x18x5-tex", "40x30x20-gauss")]


@pytest.mark.parametrize("grid,ctx", SITES)
def test_inlined_sites_compute_stepB(gold, monkeypatch, grid, ctx):
    """project_K is inlined in k_stepB, k_prox, k_q_from_phi, k_prox_rhs (tile and ring) and
    k_wt_pre.  Three outer iterations, one at a time, in five contexts that reach them: after each,
    with g = grad_st(phi) and the mu before it, q must have the bits of k_stepB on g + (1/r) mu
    and mu those of mu + r (g - q) (t block clamped at 0) -- the kernels' operation order, no
    contraction (the file header of test_gpu_parity.py).  The criterion is checked apart from
    the CG: crit against sqrt(num / (den + 1e-10)) with num, den the exactly rounded sums
    (math.fsum) of the same voxel terms; every term is >= 0, so any summation order is within
    (N - 1) u, and the bar is (N + 16) 2^-52 relative.  (q of k_prox_rhs's ring voxels and of
    k_wt_pre's planes reaches only the next right-hand side F, hence the next phi: that those
    have the separate kernels' bits is test_gpu_parity.py's test_bb_fused_prox_rhs_*.)"""
    for k in ("FOTO_FUSE_PR", "FOTO_PR_TCH", "FOTO_PR_EDGE", "FOTO_PIPE"):
        monkeypatch.delenv(k, raising=False)
    env, vr = CONTEXTS[ctx]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    Nx, Ny, Nt, r, eps, rho0, rhoT = _grid(grid, gold)
    N = Nt * Nx * Ny
    with BBSolver(rho0, rhoT, Nt, Nx, Ny, r=r, reg_epsilon=eps, cg_mode=2, virtual_ranks=vr) as s:
        mu_prev, _ = s.state()
        for it in range(3):
            s.iterate(1, 0.0, False)
            phi = s.phi()
            mu, q = s.state()
            g = ops.grad_st(phi, Nt, Nx, Ny)
            assert np.array_equal(q, ops.stepB(g + (1.0 / r) * mu_prev, N)), (it, "q")
            mu_want = mu_prev + r * (g - q)
            mu_want[:N] = np.maximum(mu_want[:N], 0)
            assert np.array_equal(mu, mu_want), (it, "mu")
            gg = g[N:2 * N] * g[N:2 * N] + g[2 * N:] * g[2 * N:]
            num = math.fsum(mu[:N] * np.abs(g[:N] + 0.5 * gg))
            den = math.fsum(mu[:N] * gg)
            want = math.sqrt(num / (den + 1e-10))
            assert abs(s.crit[-1] - want) <= (N + 16) * U * want, (it, s.crit[-1], want)
            mu_prev = mu
