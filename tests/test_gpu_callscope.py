"""The one-shot entries share one kind of call scope (csrc/foto_devmem.h): a pooled stream, device
blocks freed on exit.  One pass over them in an order that hands the same pooled stream from one
kind of entry to the next -- foto_dct, foto_grad_st, foto_gn_solve_prior with and without a prior,
foto_warp, foto_flow_errors, foto_pyr_down, foto_stream_probe, foto_dct again -- at the smallest
shapes that still cross a block edge, then the same pass again: the second pass equals the first
bit for bit (nothing of an earlier call, its stream or its freed blocks leaks into a later one),
and the first equals the references the operators' own tests use, at their bars:
scipy.fft 1e-13 (test_dct_axis), the oracle's grad_st 1e-13 (test_gpu_parity), the restatement's
increment solve 1e-7 and its restriction bit for bit (test_gpu_gn_pyr), the oracle's warp bit for
bit and its EE / AE at 1e-13 relative (test_dropin)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import PKG  # noqa: E402,F401  (puts the package on sys.path)

import gn_pyr_ref as R  # noqa: E402
from foto import _lib, evaluate, gn, ops  # noqa: E402
from foto.synthetic import textured_pair  # noqa: E402
from oracle import foto_oracle as O  # noqa: E402

NT, NY, NX = 5, 7, 6      # grid (Nt x Ny x Nx)
W, H = 13, 9              # image
DCT_SHAPES = [(3, 64, 1), (2, 6, 5)]   # (outer, n, inner): an FFT length, a GEMM length on a strided axis
PROBE_N, PROBE_REPS = 4096, 2


def _inputs():
    rng = np.random.default_rng(1309)
    n = W * H
    f1, f2 = textured_pair(W, H, seed=5, dx=1.2, dy=-0.7, smooth=3)
    prior = (rng.uniform(-0.8, 0.8, n), rng.uniform(-0.8, 0.8, n), rng.uniform(-0.05, 0.05, n))
    return dict(
        dct=[rng.uniform(-1, 1, s) for s in DCT_SHAPES],
        phi=rng.standard_normal(NT * NY * NX),
        f1=f1, f2=f2, prior=prior, g=R.warp(f2, *prior, W, H),
        frame=rng.uniform(0, 1, n),
        u=rng.uniform(-3, 3, n), v=rng.uniform(-3, 3, n), m=rng.uniform(-0.3, 0.3, n),
        uG=rng.uniform(-3, 3, n), vG=rng.uniform(-3, 3, n),
    )


def _dcts(x, out, tag):
    for a, (outer, n, inner) in zip(x["dct"], DCT_SHAPES):
        for inv in (False, True):
            out[f"{tag}_{n}_{int(inv)}"] = ops.dct(a, n, inner, inverse=inv)


def _one_pass(x):
    out = {}
    _dcts(x, out, "dct_a")
    out["grad_st"] = ops.grad_st(x["phi"], NT, NX, NY)
    for key, prior in (("inc", x["prior"]), ("plain", None)):
        u, v, m, info, its = gn.solve_prior(x["f1"], x["g"] if prior else x["f2"], W, H, R.ALPHA, R.LAM, prior)
        assert info == 0 and its > 0
        out[f"solve_{key}"] = np.stack([u, v, m])
        out[f"solve_{key}_its"] = np.array([its])
    out["warp"] = evaluate.warp(x["frame"], x["u"], x["v"], W, H, x["m"])
    out["errors"] = np.array(evaluate.flow_errors(x["u"], x["v"], x["uG"], x["vG"], W, H))
    out["down"] = np.concatenate(gn.pyr_down(x["f1"], x["f2"], W, H))
    us = (ctypes.c_double * 2)()
    _lib.check(_lib.lib().foto_stream_probe(PROBE_N, PROBE_REPS, us))
    assert all(np.isfinite(t) and t > 0 for t in us), list(us)   # (a timing: not compared between the passes)
    _dcts(x, out, "dct_b")
    return out


def test_interleaved_one_shot_entries():
    import scipy.fft as sfft
    x = _inputs()
    first = _one_pass(x)
    second = _one_pass(x)
    assert sorted(first) == sorted(second)
    for k in first:
        assert np.array_equal(first[k].view(np.uint64), second[k].view(np.uint64)), k

    for a, (outer, n, inner) in zip(x["dct"], DCT_SHAPES):
        for inv in (False, True):
            ref = sfft.dct(a, type=3 if inv else 2, norm="ortho", axis=1).ravel()
            for tag in ("dct_a", "dct_b"):
                err = np.abs(first[f"{tag}_{n}_{int(inv)}"] - ref).max()
                print(f"{tag} {(outer, n, inner)} inverse={inv}: max abs diff {err:.3e}")
                assert err <= 1e-13
    np.testing.assert_allclose(first["grad_st"], O.grad_st(x["phi"], NT, NY, NX), rtol=0, atol=1e-13)
    refs = {"inc": R.solve_inc(x["f1"], x["g"], W, H, R.ALPHA, R.LAM, x["prior"]),
            "plain": R.solve_inc(x["f1"], x["f2"], W, H, R.ALPHA, R.LAM, None)}
    for key, ref in refs.items():
        for a, b, name in zip(first[f"solve_{key}"], ref, "uvm"):
            print(f"solve_prior {key} {name}: max abs diff {np.abs(a - b).max():.3e}")
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-7)
    assert np.array_equal(first["warp"], O.apply_opticalflow(x["frame"], x["u"], x["v"], W, H, x["m"]))
    want = np.array(O.EE(W, H, x["u"], x["v"], x["uG"], x["vG"]) + O.AE(W, H, x["u"], x["v"], x["uG"], x["vG"]))
    np.testing.assert_allclose(first["errors"], want, rtol=1e-13)
    assert np.array_equal(first["down"], np.concatenate([R.down(x["f1"], W, H), R.down(x["f2"], W, H)]))
