"""The premises of tests/test_gpu_projk.py, checked without a GPU.

That test holds the HIP project_K to a multiple of the float64 oracle's own error against an
exact projection (oracle/projk_exact.py, 80-digit decimal).  Here, on every input regime of
oracle/projk_cases.py:

  * the exact reference passes its own check (cubic residual <= 1e-45 of the largest term);
  * a second construction of it (bisection on the Lagrange multiplier instead of Newton on the
    cubic) agrees to 1e-40;
  * the oracle's envelope E = max_i err_i / max(1, |p_i|_inf) is finite and <= 2e-15 (measured
    3e-16 ... 8e-16: a sanity cap, not a tuned bar);
  * on the branch seam 32 (a+1)^3 + 108 rho^2 = 0 the oracle -- the reference's closed forms --
    is NaN on some points (acos argument rounding above 1, the Cardano polynomial rounding
    below 0) and finite on most: measured finite on 87 % (axis-aligned) and 92 % (rotated) of
    the points placed on the seam to the nearest double, 90 % one ulp above, all from four ulps.
"""
from decimal import Decimal

import numpy as np
import pytest

from oracle import projk_cases as C
from oracle import projk_exact as X

NAMES = sorted(C.regimes())


@pytest.mark.parametrize("name", NAMES)
def test_exact_reference_residual(name):
    p, M, hi, lo, ins, res, _ = C.exact(name)
    assert np.all(res <= float(X.RESIDUAL_BAR))
    # inside K the reference is the identity, bit for bit
    k = np.tile(ins, 3)
    assert np.array_equal(hi[k].view(np.uint64), p[k].view(np.uint64)) and not np.any(lo[k])
    # the result lies on the boundary of K (outside points) to double-double accuracy
    o = ~ins
    qa, q1, q2 = hi[:M][o], hi[M:2 * M][o], hi[2 * M:][o]
    assert np.all(np.abs(qa + 0.5 * (q1 * q1 + q2 * q2)) <= 4 * 2.0 ** -52 * np.maximum(np.abs(qa), 1e-300))


@pytest.mark.parametrize("name", NAMES)
def test_two_constructions_agree(name):
    p, M, hi, lo, ins, _, _ = C.exact(name)
    s = C.scale_of(p, M)
    idx = np.unique(np.concatenate([np.arange(0, M, max(M // 24, 1)), [M - 1]]))
    for i in idx:
        a, b1, b2 = float(p[i]), float(p[M + i]), float(p[2 * M + i])
        q, _ = X.project_point(a, b1, b2)
        qb = X.project_point_bisect(a, b1, b2)
        d = max(abs(u - v) for u, v in zip(q, qb))
        assert d <= Decimal("1e-40") * Decimal(float(s[i])), (name, i, d)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_envelope(name):
    p, M, hi, lo, _, _, qo = C.exact(name)
    err = X.point_error(qo, hi, lo, M)
    fin = np.isfinite(qo.reshape(3, M)).all(axis=0)
    if not name.startswith("seam_"):
        assert fin.all()
    E = float(np.max(err[fin] / C.scale_of(p, M)[fin]))
    print(f"{name}: oracle envelope {E:.3e}, finite on {fin.sum()} of {M}")
    assert np.isfinite(E) and E <= 2e-15


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("seam_")])
def test_oracle_seam_defect(name):
    """The reference's defect, pinned: NaN on some points placed on the seam, finite on at
    least three quarters of every seam set."""
    _, M, _, _, _, _, qo = C.exact(name)
    fin = np.isfinite(qo.reshape(3, M)).all(axis=0)
    assert fin.mean() >= 0.75
    if name.endswith("_+0ulp"):
        assert not fin.all()
