// Spectral CG for the stepA Poisson solve (benamou_brenier.py:85) -- gfx950.
//
// A = -r L_st + r eps I with the Neumann lap1d stencils of operators.py:95-110 is
// diagonalised exactly by the orthonormal DCT-II along each axis:
//     A = C^T diag(lam) C,  C = Ct (x) Cy (x) Cx,
//     lam(kt,ky,kx) = r eps + r (mu_t[kt] + mu_y[ky] + mu_x[kx]),  mu_n[k] = 2 - 2 cos(pi k / n).
// CG is basis-invariant: running scipy's CG recurrence on (diag(lam), C b) produces C x_k
// for the same x_k, the same residual norms, hence the same stopping iteration (up to
// rounding).  In that basis every CG iteration is pointwise, so one pass per iteration
// (Chronopoulos-Gear form: p.Ap from r.Ar, one fused reduction) reads and writes only r
// and p; x is recovered at the end as x = C^T ((b^ - r^) / lam).  The two vectors
// (2 x 78.6 MB at 640x480x32) stay resident in the 256 MiB Infinity Cache.
//
// This unit holds the CG variants in that basis (one step per pass, the s-step passes and
// their plan wave, the Gauss-compressed CG of foto_gauss.inc), the t-axis column kernels
// fused with them, and the host plan (SpectralPlan) that launches it all.  The per-axis
// DCT passes (GEMM, FFT and the fused (x, t) form) are in foto_dct.hip.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "foto_dct.h"
#include "foto_devmem.h"
#include "foto_devutil.h"
#include "foto_reduce.h"
#include "foto_spectral.h"

namespace foto {

// ============================================================================ CG in the eigenbasis

// The spectral box a shard owns: all kt, rows ky in [y0, y0 + nyl), all kx; laid out
// [kt][ky - y0][kx] (single shard: the whole grid, y0 = 0, nyl = Ny).
struct SpecTab {
    const double* mt;   // mu_t[kt]
    const double* my;   // mu_y[ky]
    const double* mx;   // mu_x[kx]
    double r, reps;     // r, r * eps
    int Nt, Ny, Nx;
    int y0, nyl;
};

__device__ __forceinline__ double spec_lam(const SpecTab& T, double rowmu, int kx) {
    return T.reps + T.r * (rowmu + T.mx[kx]);
}

// tile = 4 rows x 128 columns; thread (tx, ty) owns columns 2tx, 2tx+1 of row ty.
// f(i, lam0, lam1, n2): elements i and i+1 (n2 = number valid: 1 or 2).  With Nx even,
// i is even and both elements are 16-B aligned (one dwordx4 per lane).
template <class F>
__device__ __forceinline__ void spec_for_each(const SpecTab& T, F f) {
    const int rows = T.Nt * T.nyl;
    const int ntx = (T.Nx + 127) / 128;
    const int ntiles = ntx * ((rows + 3) / 4);
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int row = (t / ntx) * 4 + ty;
        const int kx = (t % ntx) * 128 + 2 * tx;
        if (row >= rows || kx >= T.Nx) continue;
        const int kt = row / T.nyl, ky = T.y0 + (row - kt * T.nyl);
        const double rowmu = T.mt[kt] + T.my[ky];
        const int64_t i = (int64_t)row * T.Nx + kx;
        const int n2 = (kx + 1 < T.Nx) ? 2 : 1;
        f(i, spec_lam(T, rowmu, kx), n2 == 2 ? spec_lam(T, rowmu, kx + 1) : 1.0, n2);
    }
}

template <bool VEC>
__device__ __forceinline__ void ld2(const double* p, int64_t i, int n2, double& a, double& b) {
    if (VEC && n2 == 2) {
        const dbl2 v = *reinterpret_cast<const dbl2*>(p + i);
        a = v[0];
        b = v[1];
    } else {
        a = p[i];
        b = (n2 == 2) ? p[i + 1] : 0.0;
    }
}

template <bool VEC>
__device__ __forceinline__ void st2(double* p, int64_t i, int n2, double a, double b) {
    if (VEC && n2 == 2) {
        *reinterpret_cast<dbl2*>(p + i) = dbl2{a, b};
    } else {
        p[i] = a;
        if (n2 == 2) p[i + 1] = b;
    }
}

// r^ = b^; partials (r.r, r.lam.r) -> gath[0..1]
template <bool VEC>
__global__ __launch_bounds__(NT) void k_spec_init(SpecTab T, const double* __restrict__ bh, double* __restrict__ rh,
                                                  RedBuf rb, double* gath) {
    double a0 = 0.0, a1 = 0.0;
    spec_for_each(T, [&](int64_t i, double l0, double l1, int n2) {
        double b0, b1;
        ld2<VEC>(bh, i, n2, b0, b1);
        st2<VEC>(rh, i, n2, b0, b1);
        a0 += b0 * b0;
        a1 += l0 * (b0 * b0);
        if (n2 == 2) {
            a0 += b1 * b1;
            a1 += l1 * (b1 * b1);
        }
    });
    double v[2] = {a0, a1}, tot[2];
    if (grid_reduce_last<2>(v, rb, tot) && threadIdx.x == 0) { gath[0] = tot[0]; gath[1] = tot[1]; }
}

// One CG iteration k (Chronopoulos-Gear): given rho_k = r.r and m_k = r.lam.r (gathered),
//   stop if ||r_k|| < atol (scipy's top-of-loop test); beta = rho_k / rho_{k-1};
//   p.Ap = m_k - beta rho_k / alpha_{k-1} (k > 0), = m_0 (k = 0); alpha = rho_k / p.Ap;
//   p = beta p + r;  r = r - alpha (lam p);  partials (r.r, r.lam.r) of r_{k+1}.
template <bool VEC>
__global__ __launch_bounds__(NT) void k_spec_cg(SpecTab T, int k, double* __restrict__ rh, double* __restrict__ ph,
                                                CGScal* S, RedBuf rb, double* gath, double rtol) {
    if (S->done) return;
    const double rho = gath[0], mk = gath[1];
    double atol, beta = 0.0, pap;
    if (k == 0) {
        atol = fmax(0.0, rtol * sqrt(rho));
        if (rho == 0.0) {
            if (blockIdx.x == 0 && threadIdx.x == 0) { S->done = 1; S->iters = 0; }
            return;
        }
        pap = mk;
    } else {
        atol = S->atol;
        beta = rho / S->rho;
        pap = mk - beta * rho / S->pap;   // S->pap holds alpha_{k-1}
    }
    if (sqrt(rho) < atol) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { S->done = 1; S->iters = k; }
        return;
    }
    const double alpha = rho / pap;
    double a0 = 0.0, a1 = 0.0;
    spec_for_each(T, [&](int64_t i, double l0, double l1, int n2) {
        double r0, r1, p0 = 0.0, p1 = 0.0;
        ld2<VEC>(rh, i, n2, r0, r1);
        if (k > 0) ld2<VEC>(ph, i, n2, p0, p1);
        p0 = (k == 0) ? r0 : beta * p0 + r0;
        p1 = (k == 0) ? r1 : beta * p1 + r1;
        const double n0 = r0 - alpha * (l0 * p0);
        const double n1 = r1 - alpha * (l1 * p1);
        st2<VEC>(ph, i, n2, p0, p1);
        st2<VEC>(rh, i, n2, n0, n1);
        a0 += n0 * n0;
        a1 += l0 * (n0 * n0);
        if (n2 == 2) {
            a0 += n1 * n1;
            a1 += l1 * (n1 * n1);
        }
    });
    double v[2] = {a0, a1}, tot[2];
    if (grid_reduce_last<2>(v, rb, tot) && threadIdx.x == 0) {
        S->rho = rho;
        S->pap = alpha;
        if (k == 0) { S->atol = atol; S->bb = rho; }
        gath[0] = tot[0];
        gath[1] = tot[1];
    }
}

// x^ = (b^ - r^) / lam
template <bool VEC>
__global__ __launch_bounds__(NT) void k_spec_xhat(SpecTab T, const double* __restrict__ bh,
                                                  const double* __restrict__ rh, double* __restrict__ xh) {
    spec_for_each(T, [&](int64_t i, double l0, double l1, int n2) {
        double b0, b1, r0, r1;
        ld2<VEC>(bh, i, n2, b0, b1);
        ld2<VEC>(rh, i, n2, r0, r1);
        st2<VEC>(xh, i, n2, (b0 - r0) / l0, (b1 - r1) / l1);
    });
}

// ============================================================================ s-step CG in the eigenbasis
//
// One pass = up to SMAX CG iterations.  State between passes: r = r_k, q = p_{k-1}.  The
// pass applies the planned steps pointwise (p = beta q + r; r -= alpha lam p; q = p --
// scipy's per-element recurrence) with scalars prepared by the previous pass, then
// accumulates the Chebyshev moments of the NEW state,
//     M^rr_m = sum T_m(x) r^2,  M^rq_m = sum T_m(x) r q,  M^qq_m = sum T_m(x) q^2,
//     x = (lam - c0) / c1 in [-1, 1],  m = 0 .. 2 SMAX - 1,
// from which one wavefront of the last block plans the next pass: r_{k+i} = A_i(lam) r +
// B_i(lam) q with Chebyshev-coefficient polynomials, inner products through the Gram matrix
// (M_{a+c} + M_{|a-c|}) / 2.  Step i > 0 is taken only while its two Gram-form inner
// products (rho_{k+i} and p.Ap) are well conditioned: sum |terms| / |result| <= S_CLIM
// (3e4, i.e. ~3e-12 relative rounding; DESIGN.md 3.1.1 has the sweep).  Early in a solve
// the residual measure is a few dominant low-frequency components, the Chebyshev-Krylov basis is nearly degenerate and
// passes take 1-2 steps; later ones take SMAX.  A fixed s >= 3 loses digits in the first
// passes (measured: alpha off by 1e-4 at s = 3, k = 0).  tests/test_sstep_plan.py checks
// the planning rule (numpy restatement) against the golden solves: the same CG counts as
// scipy; at 640x480x32, 24 passes for 147 iterations (s = 2: 74).

constexpr int SMAX = 8;              // max CG steps per pass
constexpr int NMOM = 2 * SMAX;       // moments per family: degrees 0 .. 2 SMAX - 1
constexpr int NACC = 3 * NMOM;       // rr, rq, qq
constexpr int NCO = SMAX + 1;        // Chebyshev coefficients per part (degree <= SMAX)
constexpr int NG = 2 * NCO;          // combined (r part, q part) coefficient index
constexpr double S_CLIM = 3e4;       // cancellation limit of a Gram-form inner product
static_assert(NG <= 64, "coefficients live one per lane");
static_assert(NG % 2 == 0, "pairs of coefficients (r part, q part)");

struct SStep {
    int k;        // iterations applied so far
    int nsteps;   // steps the next pass applies (0 .. SMAX)
    int fin;      // after applying nsteps the solve is finished
    int conv;     // ... because the stop test passed (else: maxiter reached)
    int done;     // 1 converged, 2 maxiter reached (host polls this)
    int iters;    // iterations at finish
    int passes;   // plans made in this solve
    int flags;    // bit 0: no interval adaptation (A/B runs, FOTO_SADAPT=0)
    int pend;     // the moments in gath await their plan (made at the start of the next pass)
    int pad_;
    double a[SMAX], b[SMAX];
    double rho_prev;   // rho_{k-1}
    double atol;
    double c0, c1;     // Chebyshev interval of the next pass's moments: lam in [c0 - c1, c0 + c1]
    double gc0, gc1;   // the whole spectrum's interval (fixed)
    double ic0, ic1;   // interval of the next solve's INIT moments (set by each INIT plan)
};

// Interval adaptation: the Chebyshev-Krylov basis is well conditioned when [c0 - c1, c0 + c1]
// spans where the residual measure sum r^2 delta(lam) has its weight.  Early in a solve that
// weight sits at low frequencies and the full-spectrum basis is nearly degenerate (passes of
// 1-2 steps); so the plan sets the next pass's interval to [lmin, min(lmax, mean + S_KAPPA sd)]
// of the measure of the state it just received (from M_0..M_2 of the rr family).  Elements
// above the interval get |x| > 1 (large T_m); the cancellation rule keeps every planned step
// accurate regardless.  Measured (numpy restatement, tests/test_sstep_plan.py): at the bench
// grid 24 -> 22 passes on the first outer iteration, 33 -> 28 at 160x120x32; no change in
// CG counts or iterates.
constexpr double S_KAPPA = 2.0;
constexpr int S_PROJ = (NMOM - 3) / 2;   // projected interval after n <= S_PROJ steps (2n + 2 < NMOM)

// Plan helpers.  Coefficient vectors are distributed one entry per lane: lane j < NG holds
// index j of (r part | q part), lanes >= NG hold 0; lane j also holds row j of the Gram
// matrix H.  Cross-lane traffic stays in registers: V broadcast by v_readlane into SGPRs, the
// |terms| sums by FMA with |.| operand modifiers, lane sums by a DPP row_shr tree (lanes 15 and
// 31 hold the row totals), neighbours for lam U by DPP wave shifts -- no LDS round trip.

// sum over lanes 0 .. 31 (lanes >= NG hold 0), uniform result: the row tree, then rows 0 and 1
__device__ __forceinline__ double dpp_sum32(double v) {
    dpp_row_sums(v);
    return dbl_readlane(v, 15) + dbl_readlane(v, 31);
}

// <U, V> = sum_j U_j (H V)_j and whether its cancellation ratio sum |terms| / |<U, V>| is
// within S_CLIM (*cratio = 1, else infinity; tested as sum|terms| <= S_CLIM |<U, V>|).
// nc: V's coefficients of degree >= nc are zero in both parts (step i of a plan: R has degree
// i, lam Pn degree i + 1); with the step loop unrolled nc is a constant and the zero columns
// cost nothing (about half the broadcasts and FMAs of a plan).
__device__ __forceinline__ double plan_ip_dpp(double U, double V, const double (&hrow)[NG], double* cratio,
                                              int nc = NCO) {
    double w0 = 0.0, w1 = 0.0, a0 = 0.0, a1 = 0.0;
    int j = 0;
#pragma unroll
    for (int c = 0; c < NG; ++c) {
        if (c % NCO >= nc) continue;
        const double v = dbl_readlane(V, c);
        if (j++ % 2 == 0) {
            w0 = fma(hrow[c], v, w0);
            a0 = fma(fabs(hrow[c]), fabs(v), a0);
        } else {
            w1 = fma(hrow[c], v, w1);
            a1 = fma(fabs(hrow[c]), fabs(v), a1);
        }
    }
    const double s = dpp_sum32(U * (w0 + w1));
    const double sa = dpp_sum32(fabs(U) * (a0 + a1));
    *cratio = (s != 0.0 && sa <= S_CLIM * fabs(s)) ? 1.0 : INFINITY;   // (no division)
    return s;
}

// lam U = c0 U + c1 x U, x T_0 = T_1, x T_m = (T_{m+1} + T_{m-1}) / 2 within each part; the
// top coefficient is never multiplied (its degree would exceed SMAX; it is zero whenever
// this is called).
__device__ __forceinline__ double plan_mul_lam_dpp(double U, double c0, double c1) {
    const int lane = threadIdx.x & 63;
    const double um = dbl_dpp<0x138>(U);   // wave_shr:1 -> U[lane - 1]
    const double up = dbl_dpp<0x130>(U);   // wave_shl:1 -> U[lane + 1]
    const int pb = (lane < NCO) ? 0 : NCO, m = lane - pb;
    double X = 0.0;
    if (lane < NG) {
        if (m == 1) X += um;
        if (m >= 2) X += 0.5 * um;
        if (m <= NCO - 3) X += 0.5 * up;
    }
    return (lane < NG) ? c0 * U + c1 * X : 0.0;
}

// Finish the pass's bookkeeping and plan the next pass (scipy's loop: top-of-iteration test
// ||r|| < atol, then p = beta p + r, alpha = rho / p.Ap, r -= alpha A p).  Called by all 64
// lanes of one wave with the same S (state at the start of the pass) and the summed
// moments tot[NACC] (shared); lane 0 stores the new state.
__device__ void sstep_plan_wave(SStep* Sg, SStep S, const double* tot, int init, double rtol, int maxiter) {
    const int lane = threadIdx.x & 63;
    if (init) {
        S.c0 = S.ic0;   // the interval the INIT moments were taken over
        S.c1 = S.ic1;
        S.k = 0;
        S.rho_prev = 0.0;
        S.atol = fmax(0.0, rtol * sqrt(tot[0]));   // scipy: max(atol, rtol * ||b||)
        S.done = 0;
        S.passes = 0;
    } else {
        S.k += S.nsteps;
        if (S.fin) {
            S.done = S.conv ? 1 : 2;
            S.nsteps = 0;
            S.pend = 0;
            if (lane == 0) *Sg = S;
            return;
        }
    }
    // row `lane` of H[a][c] = <T_a u, T_c v>, u, v in {r, q} by part: (M_{a+c} + M_{|a-c|}) / 2
    // of family rr / rq / qq (degrees >= NMOM are never needed)
    double hrow[NG];
    {
        const int a = lane < NG ? lane : 0, ia = a % NCO, pa = a / NCO;
#pragma unroll
        for (int c = 0; c < NG; ++c) {
            const int ic = c % NCO, fam = pa + c / NCO;
            const double* M = tot + fam * NMOM;
            hrow[c] = (lane < NG && ia + ic < NMOM) ? 0.5 * (M[ia + ic] + M[ia > ic ? ia - ic : ic - ia]) : 0.0;
        }
    }
    double R = (lane == 0) ? 1.0 : 0.0;     // r_k     = 1 * r
    double P = (lane == NCO) ? 1.0 : 0.0;   // p_{k-1} = 1 * q
    double rho_prev = S.rho_prev;
    int n = 0;
    bool conv = false;
    double av = 0.0, bv = 0.0;   // lane i: step i's alpha, beta (stored after the loop)
    // wave-uniform tests as scalar branches (the values are uniform; the compiler cannot see it)
    auto uni = [](bool b) { return __builtin_amdgcn_readfirstlane(b ? 1 : 0) != 0; };
#pragma clang loop unroll(full)
    for (int i = 0; i < SMAX; ++i) {
        if (S.k + i >= maxiter) break;
        double rho, cr = 0.0;
        if (i == 0) rho = tot[0];
        else {
            rho = plan_ip_dpp(R, R, hrow, &cr, i + 1);
            if (uni(!(cr <= 1.0))) break;   // badly conditioned (or NaN): leave it to the next pass
        }
        if (uni(rho == 0.0 || sqrt(rho) < S.atol)) { conv = true; break; }
        const bool first = (S.k + i == 0);
        const double beta = first ? 0.0 : rho / rho_prev;
        const double Pn = first ? R : beta * P + R;
        const double Q = plan_mul_lam_dpp(Pn, S.c0, S.c1);
        const double den = plan_ip_dpp(Pn, Q, hrow, &cr, i + 2);
        if (i > 0 && uni(!(cr <= 1.0))) break;
        const double alpha = rho / den;
        R = R - alpha * Q;
        P = Pn;
        rho_prev = rho;
        av = (lane == i) ? alpha : av;
        bv = (lane == i) ? beta : bv;
        ++n;
    }
    if (lane < n) {
        Sg->a[lane] = av;
        Sg->b[lane] = bv;
    }
    S.nsteps = n;
    S.rho_prev = rho_prev;
    S.passes += 1;
    S.fin = 0;
    S.conv = conv ? 1 : 0;
    if (conv || S.k + n >= maxiter) {
        S.fin = 1;
        S.iters = conv ? S.k + n : maxiter;
        if (n == 0) S.done = conv ? 1 : 2;   // nothing left to apply
    }
    // Next pass's interval.  After n <= S_PROJ steps the plan knows the new residual's
    // coefficients R, so the mean and variance of its measure are Gram forms
    // (<R, lam R>, <lam R, lam R> over <R, R>; degrees <= 2n + 2 < NMOM); after more steps
    // it falls back to the measure these moments describe (one pass behind).  An INIT plan
    // also sets the next solve's INIT interval from the measure of b^ (consecutive outer
    // iterations' right-hand sides are close).
    const double lmin = S.gc0 - S.gc1, lmax = S.gc0 + S.gc1;
    auto to_interval = [&](double mean, double var, double& c0o, double& c1o) {
        double hi = fmin(lmax, mean + S_KAPPA * sqrt(fmax(var, 0.0)));
        hi = fmax(hi, lmin + 1e-3 * (lmax - lmin));
        if (hi == hi) {   // not NaN
            c0o = 0.5 * (hi + lmin);
            c1o = 0.5 * (hi - lmin);
        }
    };
    double nc0 = S.c0, nc1 = S.c1, ic0 = S.ic0, ic1 = S.ic1;
    double mom_mean = 0.0, mom_var = -1.0;   // the moments' own measure
    if (tot[0] > 0.0) {
        const double ex = tot[1] / tot[0], ex2 = 0.5 * (tot[2] + tot[0]) / tot[0];
        mom_mean = S.c0 + S.c1 * ex;
        mom_var = S.c1 * S.c1 * (ex2 - ex * ex);
    }
    const bool adapt = !(S.flags & 1);
    if (adapt && init && mom_var >= 0.0) to_interval(mom_mean, mom_var, ic0, ic1);
    bool projected = false;
    if (adapt && n > 0 && n <= S_PROJ && !S.fin) {
        double c1r, c2r, c3r;
        const double LR = plan_mul_lam_dpp(R, S.c0, S.c1);
        const double rr = plan_ip_dpp(R, R, hrow, &c1r, n + 1);
        const double rl = plan_ip_dpp(R, LR, hrow, &c2r, n + 2);
        const double ll = plan_ip_dpp(LR, LR, hrow, &c3r, n + 2);
        if (rr > 0.0) {
            const double mean = rl / rr;
            to_interval(mean, ll / rr - mean * mean, nc0, nc1);
            projected = true;
        }
    }
    if (adapt && !projected && mom_var >= 0.0) to_interval(mom_mean, mom_var, nc0, nc1);
    if (lane == 0) {   // scalars only: a[], b[] were stored above
        Sg->k = S.k; Sg->nsteps = S.nsteps; Sg->fin = S.fin; Sg->conv = S.conv; Sg->done = S.done;
        Sg->iters = S.iters; Sg->passes = S.passes; Sg->rho_prev = S.rho_prev; Sg->atol = S.atol;
        Sg->c0 = nc0; Sg->c1 = nc1; Sg->ic0 = ic0; Sg->ic1 = ic1; Sg->pend = 0;
    }
}

// What the last block does with the summed moments tot[NACC] (shared).  Without PLAN they go to
// this rank's slot of gath (k_spec_s2_plan plans after the all-gather) and every thread is done:
// true.  With PLAN, false in wave 0 alone, which goes on to plan the next pass (sstep_plan_wave).
template <bool PLAN, int NTH>
__device__ __forceinline__ bool moments_handed_over(const double* tot, double* gath, int rank) {
    if (!PLAN) {
        rank_slot_store<NACC, NTH>(gath, rank, tot);
        return true;
    }
    return threadIdx.x >= 64;
}

// ... after an INIT sweep that took the rr moments alone (q = 0: rq, qq vanish)
template <bool PLAN, int NTH>
__device__ __forceinline__ bool init_moments_handed_over(double* tot, double* gath, int rank) {
    for (int m = NMOM + threadIdx.x; m < NACC; m += NTH) tot[m] = 0.0;
    __syncthreads();
    return moments_handed_over<PLAN, NTH>(tot, gath, rank);
}

// element pair of tile t owned by this thread (see spec_for_each); n2 = 0: none
struct SpElem {
    int64_t i;
    double l0, l1;
    int n2;
};

template <int TR>
__device__ __forceinline__ SpElem spec_elem(const SpecTab& T, int t, int ntx, int rows) {
    SpElem e;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int row = (t / ntx) * TR + ty;
    const int kx = (t % ntx) * 128 + 2 * tx;
    e.n2 = 0;
    e.i = 0;
    e.l0 = e.l1 = 1.0;
    if (row < rows && kx < T.Nx) {
        const int kt = row / T.nyl, ky = T.y0 + (row - kt * T.nyl);
        const double rowmu = T.mt[kt] + T.my[ky];
        e.i = (int64_t)row * T.Nx + kx;
        e.n2 = (kx + 1 < T.Nx) ? 2 : 1;
        e.l0 = spec_lam(T, rowmu, kx);
        e.l1 = (e.n2 == 2) ? spec_lam(T, rowmu, kx + 1) : 1.0;
    }
    return e;
}

// gath == nullptr (FUSE): single shard, the last block plans the next pass itself.
// Otherwise the last block stores this shard's moments at gath[rank * NACC]; after the
// all-gather, k_spec_s2_plan sums them in rank order and plans (identically on every rank).
// 1024 threads: one block per CU at the pass's occupancy (4 waves / SIMD), so the
// cross-block tail gathers 48 x 256 partials in one round trip (with 256-thread blocks it
// was 48 x 1024 in six: 14 us of each pass).
// Occupancy of the pass kernels follows the accumulator count: 2 SMAX x 3 fp64 moments per
// thread = 12 SMAX VGPRs (96 at SMAX 8: 4 waves/SIMD in <= 128; 120 at 10: 3 waves in <= 168;
// 144 at 12: 2 waves), and a block is one CU's worth of waves (one block per CU).
constexpr int S2_WPE = 4;                                       // waves per SIMD
constexpr int S2_NTH = 256 * S2_WPE;                            // threads per block of the s-step pass

// 4 waves / SIMD: the streaming body needs the occupancy; the fused plan must fit beside it.
template <bool VEC, bool INIT, bool FUSE>
__global__ __launch_bounds__(S2_NTH) __attribute__((amdgpu_waves_per_eu(S2_WPE))) void k_spec_s2(SpecTab T, double* __restrict__ rh, double* __restrict__ ph,
                                                    const double* __restrict__ bh, SStep* Sg, RedBuf rb,
                                                    double rtol, int maxiter, double* gath, int rank) {
    constexpr int TR = S2_NTH / 64;   // tile = TR rows x 128 columns
    const SStep S0 = *Sg;             // uniform: scalar loads
    if (!INIT && (S0.done || S0.nsteps == 0)) return;
    const int k = S0.k, ns = INIT ? 0 : S0.nsteps;
    const double c0 = INIT ? S0.ic0 : S0.c0, ic1 = 1.0 / (INIT ? S0.ic1 : S0.c1);
    const bool loadq = !INIT && k > 0;
    // r_0 = b^: the INIT pass (or the fused t-axis kernel, which writes no r^) leaves it in b^
    const double* src = (INIT || k == 0) ? bh : rh;
    double acc[NACC];
#pragma unroll
    for (int m = 0; m < NACC; ++m) acc[m] = 0.0;
    // (a lambda around the shared function, here and in ring_pass_t: the two calls per tile are
    // inlined where the written-out formula was, and the tile loop keeps its instructions)
    auto moments = [&](double lam, double r, double q) { cheb_moments_acc<3, NMOM>(acc, (lam - c0) * ic1, r, q); };
    const int rows = T.Nt * T.nyl;
    const int ntx = (T.Nx + 127) / 128;
    const int ntiles = ntx * ((rows + TR - 1) / TR);
    // A plain grid-stride tile loop: software-pipelining it (next tile's loads issued first)
    // measured no faster at SMAX = 6 and spills at SMAX = 8.
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const SpElem e = spec_elem<TR>(T, t, ntx, rows);
        if (!e.n2) continue;
        double r0, r1, q0 = 0.0, q1 = 0.0;
        ld2<VEC>(src, e.i, e.n2, r0, r1);
        if (loadq) ld2<VEC>(ph, e.i, e.n2, q0, q1);
        if (INIT) {
            st2<VEC>(rh, e.i, e.n2, r0, r1);
        } else {
#pragma clang loop unroll(full)
            for (int i = 0; i < SMAX; ++i) {
                if (i < ns) {   // guard, not break: keeps the loop fully unrolled (S0 out of scratch)
                    // iteration k + i: p = beta p + r (p = r at k = 0); r -= alpha (lam p)
                    const double a = S0.a[i], b = S0.b[i];
                    // (k + i = 0: b = 0 and q = 0, so p = r)
                    const double p0 = fma(b, q0, r0);
                    const double p1 = fma(b, q1, r1);
                    r0 = fma(-a, e.l0 * p0, r0);
                    r1 = fma(-a, e.l1 * p1, r1);
                    q0 = p0;
                    q1 = p1;
                }
            }
            st2<VEC>(rh, e.i, e.n2, r0, r1);
            st2<VEC>(ph, e.i, e.n2, q0, q1);
        }
        moments(e.l0, r0, q0);
        if (e.n2 == 2) moments(e.l1, r1, q1);
    }
    __shared__ double tot[NACC];
    if (!grid_reduce_last_rs<NACC, S2_NTH>(acc, rb, tot)) return;
    if (moments_handed_over<FUSE, S2_NTH>(tot, gath, rank)) return;
    sstep_plan_wave(Sg, S0, tot, INIT ? 1 : 0, rtol, maxiter);
}

// ---------------------------------------------------------------------------- ring-fed pass
// The same pass with r, q streamed through a per-wave LDS ring by LDS-DMA
// (global_load_lds_dwordx4): each wave walks its own sequence of 128-column row segments
// ("wave tiles") and keeps D of them in flight, so a CU holds up to 16 x (D - 1) x 2 KiB of
// loads in flight without spending VGPRs on them (the register-fed pass, 121 VGPRs for the
// 48 moment accumulators, holds one tile per wave: ~32 KiB per CU, too little to cover the
// HBM latency under load -- it streamed at ~4.3 TB/s).  Counting: VMEM operations complete
// in issue order on gfx950 (stores included), so before reading tile j the wave waits until
// at most K operations are outstanding, K = those issued after tile j's loads.  The ring is
// read with inline-asm ds_read (invisible to hipcc's waitcnt pass, which would otherwise wait
// for the newest DMA), and the loop has no other vector-memory loads: the mu tables are
// staged in LDS before the pipeline starts (an ordinary load would complete behind every
// DMA in flight).  Per element the arithmetic is the register-fed pass's, in the same order:
// r, q are bit-identical; only the moment summation order differs (element-to-thread map).
// Ring depth: what the LDS left after the tables (18 KiB) and the reduction scratch allows
// (16 waves x 4 x 2 KiB at SMAX 8, 12 x 5 at 10, 8 x 8 at 12).
constexpr int RING_D = 4;
constexpr int RING_NW = S2_NTH / 64;    // waves per block
constexpr int RING_SLOT = 256;          // doubles per ring slot: r (128) then q (128)
constexpr int RING_TAB = 2304;          // mu_x, mu_t, mu_y (own rows) staged in LDS (doubles)
typedef __attribute__((address_space(3))) void lds_void_t;
// one wave's LDS writes ordered before what follows (its own lanes: a wave-local wait suffices)
#define FOTO_LDS_WAIT() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

__device__ __forceinline__ unsigned lds_u32(const void* p) { return (unsigned)(uintptr_t)(const lds_void_t*)p; }

__device__ __forceinline__ dbl2 lds_ld128(unsigned a) {   // caller waits lgkmcnt
    dbl2 v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(a) : "memory");
    return v;
}
__device__ __forceinline__ double lds_ld64(unsigned a) {
    double v;
    asm volatile("ds_read_b64 %0, %1" : "=v"(v) : "v"(a) : "memory");
    return v;
}

// wait until at most k vector-memory operations are outstanding (k wave-uniform; clamped)
template <int N>
__device__ __forceinline__ void vm_wait_imm() {
    static_assert(N >= 0 && N <= 63, "vmcnt range");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ void vm_wait(int k) {
    switch (k) {
#define FOTO_VMW(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
        FOTO_VMW(1) FOTO_VMW(2) FOTO_VMW(3) FOTO_VMW(4) FOTO_VMW(5) FOTO_VMW(6) FOTO_VMW(7) FOTO_VMW(8)
        FOTO_VMW(9) FOTO_VMW(10) FOTO_VMW(11) FOTO_VMW(12) FOTO_VMW(13) FOTO_VMW(14) FOTO_VMW(15)
        FOTO_VMW(16) FOTO_VMW(17) FOTO_VMW(18) FOTO_VMW(19) FOTO_VMW(20) FOTO_VMW(21) FOTO_VMW(22)
        FOTO_VMW(23) FOTO_VMW(24) FOTO_VMW(25) FOTO_VMW(26) FOTO_VMW(27) FOTO_VMW(28) FOTO_VMW(29)
        FOTO_VMW(30) FOTO_VMW(31)
#undef FOTO_VMW
        default:
            if (k > 31) asm volatile("s_waitcnt vmcnt(31)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
}

// Usable for a shard when Nx is even (16-B lanes) and the tables fit.  The flat tiling (Nx not
// a multiple of 128) also needs the box's element indices in 30 bits (32-bit element
// arithmetic; ring_divmod's quotients, at most Nt * nyl < 2^21 under the table bound, are
// exact); row-segment tiles index with 64-bit element offsets; the write-through stores take
// 32-bit byte offsets (a box under 4 GiB).
static inline bool ring_ok(const SpecTab& T) {
    const bool flat = (T.Nx % 128) != 0;
    return (T.Nx % 2) == 0 && T.Nx + T.Nt + T.nyl <= RING_TAB &&
           (!flat || (int64_t)T.Nt * T.nyl * T.Nx < (int64_t(1) << 30)) &&
           (int64_t)T.Nt * T.nyl * T.Nx * 8 < (int64_t(1) << 32);   // ring_store offsets
}

// Tables: mu_x [0, Nx), mu_t [Nx, Nx + Nt), mu_y of the own rows [Nx + Nt, + nyl).
// (first: the first thread taking part; a late-planning pass leaves wave 0 to its plan)
__device__ __forceinline__ void ring_stage_tables(const SpecTab& T, double* tab, int first = 0) {
    for (int i = (int)threadIdx.x - first; i >= 0 && i < T.Nx + T.Nt + T.nyl; i += S2_NTH - first)
        tab[i] = (i < T.Nx) ? T.mx[i] : (i < T.Nx + T.Nt) ? T.mt[i - T.Nx] : T.my[T.y0 + i - T.Nx - T.Nt];
}

// The wave's tile sequence: u = gw + j W (j < nj), u -> (row, 128-column segment cx) when the
// rows are whole tiles (Nx % 128 == 0); otherwise the box is tiled flat (tile u = elements
// [128 u, 128 u + 128) of the contiguous [t][y][x] box, rows found per lane), so row lengths
// like Middlebury's 584 (4.56 tiles) or 420 (3.28) leave no idle lanes in a last segment.
struct RingWave {
    int gw, W, nj, ntx;
    bool flat;
    int nel;         // elements of the box (flat tiling)
    double* wring;   // this wave's D slots
};

// floor(e / n) and the remainder, 0 <= e < 2^30, quotient < 2^21: the fp32 estimate is off by
// less than (e / n) 2^-21.7 + 1 < 2, and one correction each way makes it exact
__device__ __forceinline__ int ring_divmod(int e, int n, float inv, int* rem) {
    int q = (int)((float)e * inv);
    int r = e - q * n;
    if (r < 0) { --q; r += n; }
    else if (r >= n) { ++q; r -= n; }
    *rem = r;
    return q;
}

__device__ __forceinline__ RingWave ring_wave(const SpecTab& T, double* ring, int D) {
    RingWave w;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rows = T.Nt * T.nyl;
    w.ntx = (T.Nx + 127) / 128;
    w.flat = (T.Nx % 128) != 0;
    w.nel = w.flat ? rows * T.Nx : 0;   // (< 2^30 when flat: ring_ok)
    const int nwt = w.flat ? (w.nel + 127) / 128 : rows * w.ntx;
    w.gw = blockIdx.x * RING_NW + wv;
    w.W = gridDim.x * RING_NW;
    w.nj = w.gw < nwt ? (nwt - 1 - w.gw) / w.W + 1 : 0;
    w.wring = ring + wv * D * RING_SLOT;
    return w;
}

// Wave-uniform position of a row-segment tile (Nx % 128 == 0): row = u / ntx, cx = u % ntx,
// kt = row / nyl, ky = row % nyl, advanced by W tiles with scalar adds instead of the three
// integer divisions per tile (~30 SALU instructions each) the loop used to spend.
struct RingCursor {
    int row, cx, kt, ky;
    int dr, dc;   // W = dr * ntx + dc
    __device__ __forceinline__ void init(int u, int W, int ntx, int nyl) {
        row = u / ntx; cx = u - row * ntx;
        kt = row / nyl; ky = row - kt * nyl;
        dr = W / ntx; dc = W - dr * ntx;
    }
    __device__ __forceinline__ void step(int ntx, int nyl) {
        cx += dc;
        int d = dr;
        if (cx >= ntx) { cx -= ntx; ++d; }
        row += d;
        ky += d;
        while (ky >= nyl) { ky -= nyl; ++kt; }
    }
};

// DMA of a tile (r from src, q from ph when loadq) into ring slot `slot`; i: the element of
// this lane's first value (16 B per lane)
__device__ __forceinline__ void ring_dma(double* slot, int64_t i, const double* src, const double* ph, bool loadq) {
    __builtin_amdgcn_global_load_lds((const void*)(src + i), (lds_void_t*)slot, 16, 0, 0);
    if (loadq) __builtin_amdgcn_global_load_lds((const void*)(ph + i), (lds_void_t*)(slot + 128), 16, 0, 0);
}

// element index of this lane's pair in tile u (flat: idle lanes fetch a valid address, never read)
template <bool FLAT>
__device__ __forceinline__ int64_t ring_elem(const SpecTab& T, const RingWave& w, int u, int row, int cx) {
    const int lane = threadIdx.x & 63;
    if (FLAT) {
        const int e = u * 128 + 2 * lane;
        return (e < w.nel) ? e : u * 128;
    }
    return (int64_t)row * T.Nx + cx * 128 + 2 * lane;
}

// DMA of the wave's tile j (prologue issue outside the pass loop: the late-planning prefetch)
template <int D>
__device__ __forceinline__ void ring_issue(const SpecTab& T, const RingWave& w, int j, const double* src,
                                           const double* ph, bool loadq) {
    const int u = w.gw + j * w.W;
    int64_t i;
    if (w.flat) {
        i = ring_elem<true>(T, w, u, 0, 0);
    } else {
        const int row = u / w.ntx;
        i = ring_elem<false>(T, w, u, row, u - row * w.ntx);
    }
    ring_dma(w.wring + (j % D) * RING_SLOT, i, src, ph, loadq);
}

// 16-B store of r or q: write-through (sc1; see st_wt16); the s_nop covers
// the store-data hazard of a >8-B store before a later VALU write of its data registers
// (inline asm is outside the compiler's hazard tracking)
// (saddr form: the base in SGPRs and a 32-bit byte offset per lane, as the compiler's own stores;
// a 64-bit address per lane cost the tile loop 4 VGPRs and spilled it)
__device__ __forceinline__ void ring_store(double* base, int64_t i, dbl2 v) {
    const unsigned off = (unsigned)(i * 8);
    asm volatile("global_store_dwordx4 %0, %1, %2 sc1\n\ts_nop 1" ::"v"(off), "v"(v), "s"(base) : "memory");
}

// One pass over the wave's tiles with S0's planned steps (none for INIT): apply them, write r
// (and q), accumulate the moments of the new state into acc.  issued: tiles [0, issued) already
// have their DMAs in flight or landed (a prefetch), the rest of the prologue is issued here.
// FLAT is compile-time, so the row-segment loop has no tiling branches and no lane masks.
template <int D, bool INIT, bool FLAT>
__device__ __forceinline__ void ring_pass_t(const SpecTab& T, const RingWave& w, unsigned tab_a, const SStep& S0,
                                            double* __restrict__ rh, double* __restrict__ ph,
                                            const double* __restrict__ bh, double (&acc)[NACC], int issued, bool mom) {
    const int lane = threadIdx.x & 63;
    const int k = S0.k, ns = INIT ? 0 : S0.nsteps;
    // (the division runs on the VALU: readlane puts c0, 1 / c1 back in SGPRs, not in two VGPR
    // pairs the register-bound loop would spill)
    const double c0 = dbl_readlane(INIT ? S0.ic0 : S0.c0, 0), ic1 = dbl_readlane(1.0 / (INIT ? S0.ic1 : S0.c1), 0);
    // wave-uniform flags as readfirstlane'd ints: a bool the compiler keeps as a lane mask turns
    // the count switch and the q DMA into exec-masked (divergent) code
    const bool loadq = __builtin_amdgcn_readfirstlane((!INIT && k > 0) ? 1 : 0) != 0;
    const bool momu = __builtin_amdgcn_readfirstlane(mom ? 1 : 0) != 0;
    const double* src = (INIT || k == 0) ? bh : rh;   // r_0 = b^ (the INIT pass leaves it there)
    auto moments = [&](double lam, double r, double q) { cheb_moments_acc<3, NMOM>(acc, (lam - c0) * ic1, r, q); };
    const int nj = w.nj;
    const float invx = 1.0f / (float)T.Nx, invy = 1.0f / (float)T.nyl;
    const int g = loadq ? 2 : 1;               // DMA instructions per tile
    constexpr int NST = INIT ? 1 : 2;          // store instructions per tile
    RingCursor cp{}, ci{};                     // the tile being processed / the next DMA's tile
    if (!FLAT) {
        cp.init(w.gw, w.W, w.ntx, T.nyl);
        ci.init(w.gw + issued * w.W, w.W, w.ntx, T.nyl);
    }
    for (int j = issued; j < D - 1 && j < nj; ++j) {
        ring_dma(w.wring + (j % D) * RING_SLOT, ring_elem<FLAT>(T, w, w.gw + j * w.W, ci.row, ci.cx), src, ph, loadq);
        if (!FLAT) ci.step(w.ntx, T.nyl);
    }
    if (!FLAT && issued > D - 1) {   // (a prefetch never issues more than the prologue)
        ci.init(w.gw + (D - 1) * w.W, w.W, w.ntx, T.nyl);
    }
    for (int j = 0; j < nj; ++j) {
        if (j + D - 1 < nj) {
            ring_dma(w.wring + ((j + D - 1) % D) * RING_SLOT,
                     ring_elem<FLAT>(T, w, w.gw + (j + D - 1) * w.W, ci.row, ci.cx), src, ph, loadq);
            if (!FLAT) ci.step(w.ntx, T.nyl);
        }
        const int nG = min(j + D - 1, nj - 1) - j, nS = min(j, D - 1);
        // steady state (D - 1 tiles ahead and behind) as one immediate wait; the switch over
        // counts (a branch tree) only in the prologue and drain
        if (nG == D - 1 && nS == D - 1) {
            if (INIT || !loadq) vm_wait_imm<(1 + NST) * (D - 1)>();
            else vm_wait_imm<(2 + NST) * (D - 1)>();
        } else {
            vm_wait(__builtin_amdgcn_readfirstlane(g * nG + NST * nS));
        }
        const int u = w.gw + j * w.W;
        int kx, kt, ky;
        bool ok = true;
        int64_t i;
        if (FLAT) {   // per lane: element e -> (row, kx) -> (kt, ky)
            const int e0 = u * 128 + 2 * lane;
            ok = e0 < w.nel;
            const int e = ok ? e0 : u * 128;
            const int row = ring_divmod(e, T.Nx, invx, &kx);
            kt = ring_divmod(row, T.nyl, invy, &ky);
            i = e;
        } else {      // whole row segments: every lane valid
            kx = cp.cx * 128 + 2 * lane;
            kt = cp.kt;
            ky = cp.ky;
            i = (int64_t)cp.row * T.Nx + kx;
            cp.step(w.ntx, T.nyl);
        }
        const unsigned sa = lds_u32(w.wring + (j % D) * RING_SLOT) + 16 * lane;
        dbl2 rv = lds_ld128(sa);
        dbl2 qv = loadq ? lds_ld128(sa + 1024) : dbl2{0.0, 0.0};
        double mtv = lds_ld64(tab_a + 8 * (T.Nx + kt));
        double myv = lds_ld64(tab_a + 8 * (T.Nx + T.Nt + ky));
        dbl2 mxv = lds_ld128(tab_a + 8 * (ok ? kx : 0));
        // the wait names every asm-loaded register, so no use is scheduled above it
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(rv), "+v"(qv), "+v"(mtv), "+v"(myv), "+v"(mxv) :: "memory");
        const double rowmu = mtv + myv;
        const double l0 = T.reps + T.r * (rowmu + mxv[0]);
        const double l1 = T.reps + T.r * (rowmu + mxv[1]);
        double r0 = rv[0], r1 = rv[1], q0 = qv[0], q1 = qv[1];
        if (!INIT) {
            // fully unrolled with a guard, not a break (a break leaves a rolled loop that indexes
            // S0.a / S0.b from scratch with a divergent exit and a vmcnt(0) wait; measured 3x
            // slower at SMAX 10)
#pragma clang loop unroll(full)
            for (int st = 0; st < SMAX; ++st) {
                if (st < ns) {
                    // iteration k + st: p = beta p + r (k + st = 0: b = 0, q = 0, so p = r);
                    // r -= alpha (lam p)
                    const double a = S0.a[st], b = S0.b[st];
                    const double p0 = fma(b, q0, r0);
                    const double p1 = fma(b, q1, r1);
                    r0 = fma(-a, l0 * p0, r0);
                    r1 = fma(-a, l1 * p1, r1);
                    q0 = p0;
                    q1 = p1;
                }
            }
        }
        if (ok) {
            ring_store(rh, i, dbl2{r0, r1});
            if (!INIT) ring_store(ph, i, dbl2{q0, q1});
        }
        if (momu) {
            // idle lanes of a flat tail contribute exact zeros (r = q = 0: fma(t, 0, acc) = acc)
            if (!ok) r0 = r1 = q0 = q1 = 0.0;
            moments(l0, r0, q0);
            moments(l1, r1, q1);
        }
    }
}

// The pass over the wave's tiles with S0's planned steps (dispatch on the tiling; per element the
// arithmetic is the register-fed pass's, in the same order).
template <int D, bool INIT>
__device__ __forceinline__ void ring_pass(const SpecTab& T, const RingWave& w, unsigned tab_a, const SStep& S0,
                                          double* __restrict__ rh, double* __restrict__ ph,
                                          const double* __restrict__ bh, double (&acc)[NACC], int issued,
                                          bool mom = true) {
    if (w.flat) ring_pass_t<D, INIT, true>(T, w, tab_a, S0, rh, ph, bh, acc, issued, mom);
    else ring_pass_t<D, INIT, false>(T, w, tab_a, S0, rh, ph, bh, acc, issued, mom);
}

// SStep from LDS into wave-uniform registers (the plan made in LDS feeds the step loop's
// scalar operands)
__device__ __forceinline__ SStep sstep_uniform(const SStep* p) {
    static_assert(sizeof(SStep) % 4 == 0, "SStep is whole dwords");
    constexpr int NW = sizeof(SStep) / 4;
    int wd[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) wd[i] = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(p)[i]);
    SStep s;
    __builtin_memcpy(&s, wd, sizeof s);
    return s;
}

// FUSE (working passes): a pass plans itself.  The pass that takes the moments leaves them in
// gath (this rank's slot; between passes of a sharded solve the all-gather fills the others)
// with S.pend = 1; the next pass's blocks each make that plan at their start, from the slots
// summed in rank order (as k_spec_s2_plan sums them, so every rank plans identically)
// (wave 0, identical inputs and code, so identical plans) while the other waves' first ring
// tiles are already loading, instead of one block planning in the tail of the previous pass
// with the whole chip idle behind it.  The last block (ticket) publishes the new moments and
// state once every block has read the old ones.  The pass whose plan finishes the solve (fin)
// skips the moments and its last block marks the solve done; a plan that finds the solve done
// at once (no step left) still passes the ticket, so that one block stores the final state.
// INIT passes plan in their tail (the fused t-DCT INIT and the ring INIT pass), leaving pend = 0.
template <int D, bool INIT, bool FUSE>
__global__ __launch_bounds__(S2_NTH) __attribute__((amdgpu_waves_per_eu(S2_WPE))) void k_spec_s2r(
        SpecTab T, double* __restrict__ rh, double* __restrict__ ph, const double* __restrict__ bh, SStep* Sg,
        RedBuf rb, double rtol, int maxiter, double* gath, int rank, int world) {
    constexpr bool LATE = FUSE && !INIT;
    __shared__ __attribute__((aligned(16))) double ring[RING_NW * D * RING_SLOT + RING_TAB];
    // A late-planning pass needs the previous pass's moments: their loads are issued before the
    // state's, so the two round trips overlap instead of running back to back (the plan waits
    // for both).  The asm use pins the loads above the state checks.
    __shared__ double tot[NACC];
    // the state the tail publishes: the plan made at the start (late) or the one in Sg; kept in
    // LDS so the tile loop holds only the fields it uses in registers (the whole SStep live
    // across the loop cost SGPR spills -- v_readlane reloads in every tile)
    __shared__ SStep Sl;
    double gpre = 0.0;
    if (LATE && threadIdx.x < NACC) gpre = gath[threadIdx.x];   // rank 0's slot
    SStep S0 = *Sg;
    if (LATE && threadIdx.x < NACC) tot[threadIdx.x] = gpre;    // (waits for the moments only)
    if (!INIT && S0.done) return;
    const bool late = LATE && S0.pend;
    if (!INIT && !late && S0.nsteps == 0) return;
    double* tab = ring + RING_NW * D * RING_SLOT;
    const RingWave w = ring_wave(T, ring, D);
    int issued = 0;
    if constexpr (LATE) {
        if (late) {
            // Wave 0 plans at once: the previous pass's moments into LDS (its own lanes, so a
            // wave-local wait orders them), its first tiles issued behind them, the plan.  The
            // other waves stage the tables and issue their first tiles meanwhile.
            const int k = S0.k + S0.nsteps;
            const double* src = (k == 0) ? bh : rh;
            if (!S0.fin) issued = min(D - 1, w.nj);   // the plan will apply steps
            if (threadIdx.x < 64) {
                // the ranks' moments, summed in rank order (k_spec_s2_plan's: 0 + g0 = g0), rank
                // 0's loaded at entry
                if (threadIdx.x < NACC && world > 1) {
                    double t = gpre;
                    for (int g = 1; g < world; ++g) t += gath[g * NACC + threadIdx.x];
                    tot[threadIdx.x] = t;
                }
                if (threadIdx.x == 0) Sl = S0;
                FOTO_LDS_WAIT();
                for (int j = 0; j < issued; ++j) ring_issue<D>(T, w, j, src, ph, k > 0);
                sstep_plan_wave(&Sl, S0, tot, 0, rtol, maxiter);
            } else {
                ring_stage_tables(T, tab, 64);
                for (int j = 0; j < issued; ++j) ring_issue<D>(T, w, j, src, ph, k > 0);
            }
            __syncthreads();   // plan, tables
            S0 = sstep_uniform(&Sl);
        } else {
            if (threadIdx.x == 0) Sl = S0;
            ring_stage_tables(T, tab);
            __syncthreads();
        }
    } else {
        ring_stage_tables(T, tab);
        __syncthreads();
    }
    double acc[NACC];
#pragma unroll
    for (int m = 0; m < NACC; ++m) acc[m] = 0.0;
    // the pass whose plan finished the solve (fin) needs no moments: its tail marks the solve
    // done (the bookkeeping sstep_plan_wave's fin branch would do at the next pass's start)
    const bool final_pass = LATE && S0.fin && !S0.done;
    if (!LATE || !S0.done) ring_pass<D, INIT>(T, w, lds_u32(tab), S0, rh, ph, bh, acc, issued, !final_pass);
    else if (issued) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // drain the prefetch
    if (!grid_reduce_last_rs<NACC, S2_NTH>(acc, rb, tot)) return;
    if constexpr (LATE) {
        // this rank's slot (the all-gather between passes fills the others).  rank_slot_store's loop
        // written out: inlined from there, its bound test merges with the entry's threadIdx.x < NACC,
        // which then stays live across the tile loop and moves this kernel's SGPR spills
        if (!S0.done && !final_pass)
            for (int m = threadIdx.x; m < NACC; m += S2_NTH) gath[rank * NACC + m] = tot[m];
        if (threadIdx.x == 0) {
            SStep So = Sl;   // == S0 (thread 0 wrote it before the barrier)
            if (final_pass) {
                So.k += So.nsteps;
                So.done = So.conv ? 1 : 2;
                So.nsteps = 0;
                So.pend = 0;
            } else {
                So.pend = S0.done ? 0 : 1;
            }
            *Sg = So;
        }
        return;
    }
    if (moments_handed_over<FUSE, S2_NTH>(tot, gath, rank)) return;
    sstep_plan_wave(Sg, S0, tot, INIT ? 1 : 0, rtol, maxiter);
}

constexpr bool ring_fits(int D) { return (RING_NW * D * RING_SLOT + RING_TAB) * 8 <= 150 * 1024; }
static_assert(ring_fits(RING_D), "ring + tables exceed the LDS");

// Run-time booleans to template arguments: with_bools(f, a, b) calls f(A, B) with A, B
// std::true_type / std::false_type objects (A() is a constant expression), so a launcher names
// its kernel once instead of once per combination.
template <class F>
static auto with_bools(F&& f) {
    return f();
}
template <class F, class... B>
static auto with_bools(F&& f, bool b, B... rest) {
    return b ? with_bools([&](auto... c) { return f(std::true_type{}, c...); }, rest...)
             : with_bools([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}

// host launcher
static hipError_t launch_s2_ring(const SpecTab& T, double* rh, double* ph, const double* bh, SStep* Sg, RedBuf rb,
                                 double rtol, int maxiter, double* gath, int rank, bool init, bool fuse,
                                 int nb = 256, hipStream_t s = 0, int world = 1) {
    return with_bools([&](auto I, auto F) {
        k_spec_s2r<RING_D, I(), F()><<<nb, S2_NTH, 0, s>>>(T, rh, ph, bh, Sg, rb, rtol, maxiter, gath, rank, world);
        return hipGetLastError();
    }, init, fuse);
}

// Multi-shard planning step (one wave): moments summed over ranks in rank order.
__global__ __launch_bounds__(64) void k_spec_s2_plan(SStep* Sg, const double* __restrict__ gath, int world, int init,
                                                     double rtol, int maxiter) {
    __shared__ double tot[NACC];
    const SStep S0 = *Sg;
    for (int m = threadIdx.x; m < NACC; m += 64) {
        double s = 0.0;
        for (int g = 0; g < world; ++g) s += gath[g * NACC + m];
        tot[m] = s;
    }
    __syncthreads();
    if (!init && S0.done) return;
    sstep_plan_wave(Sg, S0, tot, init, rtol, maxiter);
}

// ============================================================================ t axis, one thread per column
//
// The t-axis DCT of a single shard's spectral box [kt][ky][kx]: ncols = Ny Nx columns of NTT
// values at stride ncols.  A thread holds its column in registers, folds it into even / odd
// halves (C[k][NTT-1-j] = (-1)^k C[k][j]) and applies the two NTT/2 x NTT/2 halves of the
// DCT-II matrix, whose entries are wave-uniform (scalar loads): NTT^2 / 2 FMA per column and
// one read + one write of the volume, coalesced across the threads of a wave.  Ch holds
// E[m][j] = C[2m][j], then O[m][j] = C[2m+1][j] (m, j < NTT/2).  Two fusions remove whole
// passes from the s-step solve:
//   forward (+ INIT): b^ and, in the same sweep, the Chebyshev moments of r_0 = b^ (q = 0;
//     k_spec_s2<INIT>'s per-element formula), summed across blocks; the last block plans
//     the first pass.  The first pass reads r_0 from b^, so no r^ = b^ copy is made.
//   inverse (+ xhat): x^ = (b^ - r^) / lam formed in registers from b^ and r^.
template <int NTT>
struct TCol {
    static constexpr int H = NTT / 2;
    static_assert(NTT % 2 == 0 && NTT >= 2 && NTT <= 32, "even column lengths up to 32");
};

constexpr int TC_NTH = 256;
// Waves per SIMD of the t-column kernels: the VGPR count of the Nt = 32 kernels; 1024 of the
// bench grid's 1200 blocks are resident (5, so the grid fits in one round: DESIGN.md 3.5).
constexpr int TC_WPE = 4;

// MODE 2 (single shard): the last block plans the first pass; MODE 1 (a sharded box): it stores
// this rank's INIT moments at gath[rank * NACC] for the all-gather and k_spec_s2_plan; MODE 0:
// b^ only (the Gauss-compressed CG takes its own measure of b^)
constexpr int TC_PLAIN = 0, TC_GATH = 1, TC_PLAN = 2;
template <int NTT, int MODE>
__global__ __launch_bounds__(TC_NTH) __attribute__((amdgpu_waves_per_eu(TC_WPE))) void k_dct_t_fwd_init(SpecTab T, const double* __restrict__ Ch,
                                                           const double* __restrict__ in, double* __restrict__ bh,
                                                           SStep* Sg, RedBuf rb, double rtol, int maxiter,
                                                           double* gath, int rank) {
    constexpr int H = TCol<NTT>::H;
    const int64_t ncols = (int64_t)T.nyl * T.Nx;
    const int64_t c = (int64_t)blockIdx.x * TC_NTH + threadIdx.x;
    if constexpr (MODE == TC_PLAIN) {
        // b^ only: the whole column's loads first (no mu_t staging, no barrier: with them the
        // column loads started a memory latency late and were waited for in pieces)
        if (c >= ncols) return;
        double x[NTT];
#pragma unroll
        for (int j = 0; j < NTT; ++j) x[j] = ld_dead(&in[j * ncols + c]);
#pragma unroll
        for (int m = 0; m < H; ++m) {
            double e = 0.0, o = 0.0;
#pragma unroll
            for (int j = 0; j < H; ++j) {
                e = fma(Ch[m * H + j], x[j] + x[NTT - 1 - j], e);
                o = fma(Ch[H * H + m * H + j], x[j] - x[NTT - 1 - j], o);
            }
            bh[(2 * m) * ncols + c] = e;
            bh[(2 * m + 1) * ncols + c] = o;
        }
        return;
    }
    const SStep S0 = *Sg;
    const double c0 = S0.ic0, ic1 = 1.0 / S0.ic1;   // INIT interval (previous solve's b^ measure)
    double acc[NMOM];
#pragma unroll
    for (int m = 0; m < NMOM; ++m) acc[m] = 0.0;
    __shared__ double mts[NTT];   // mu_t in LDS (a global read per element after each b^ store)
    if (threadIdx.x < NTT) mts[threadIdx.x] = T.mt[threadIdx.x];
    __syncthreads();
    if (c < ncols) {
        const int kyl = (int)(c / T.Nx), kx = (int)(c - (int64_t)kyl * T.Nx), ky = T.y0 + kyl;
        // mu_y, mu_x of the column read once: inside emit they were re-read after every b^
        // store (the compiler cannot rule out aliasing), a dependent round trip per element
        const double myv = T.my[ky], mxv = T.mx[kx];
        double s[H], d[H];
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const double a = in[j * ncols + c], b = in[(NTT - 1 - j) * ncols + c];
            s[j] = a + b;
            d[j] = a - b;
        }
        auto emit = [&](int k, double X) {
            bh[k * ncols + c] = X;
            const double lam = T.reps + T.r * ((mts[k] + myv) + mxv);   // spec_lam's order
            cheb_moments_acc<1, NMOM>(acc, (lam - c0) * ic1, X);
        };
#pragma unroll
        for (int m = 0; m < H; ++m) {
            double e = 0.0, o = 0.0;
#pragma unroll
            for (int j = 0; j < H; ++j) {
                e = fma(Ch[m * H + j], s[j], e);
                o = fma(Ch[H * H + m * H + j], d[j], o);
            }
            emit(2 * m, e);
            emit(2 * m + 1, o);
        }
    }
    __shared__ double tot[NACC];
    if (!grid_reduce_last_rs<NMOM, TC_NTH>(acc, rb, tot)) return;
    if (init_moments_handed_over<MODE == TC_PLAN, TC_NTH>(tot, gath, rank)) return;
    sstep_plan_wave(Sg, S0, tot, 1, rtol, maxiter);
}

// Sg->k = iterations applied; 0: no pass ran, r^ was never written and r = b^ (x^ = 0).
// PLAIN: bh holds x^ itself (the Gauss-compressed CG's k_gq_xhat output); rh, Sg unused.
template <int NTT, bool PLAIN = false>
__global__ __launch_bounds__(TC_NTH) __attribute__((amdgpu_waves_per_eu(TC_WPE))) void k_dct_t_inv_xhat(SpecTab T, const double* __restrict__ Ch,
                                                           const double* __restrict__ bh, const double* __restrict__ rh,
                                                           const SStep* Sg, double* __restrict__ out) {
    constexpr int H = TCol<NTT>::H;
    const int64_t ncols = (int64_t)T.nyl * T.Nx;
    const int64_t c = (int64_t)blockIdx.x * TC_NTH + threadIdx.x;
    if (c >= ncols) return;
    if (!PLAIN && Sg->k == 0) rh = bh;
    const int kyl = (int)(c / T.Nx), kx = (int)(c - (int64_t)kyl * T.Nx), ky = T.y0 + kyl;
    double xe[H], xo[H];   // x^_{2m}, x^_{2m+1}
#pragma unroll
    for (int m = 0; m < H; ++m) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int k = 2 * m + p;
            double v;
            if constexpr (PLAIN) {
                v = ld_dead(&bh[k * ncols + c]);
            } else {
                const double lam = spec_lam(T, T.mt[k] + T.my[ky], kx);
                v = (bh[k * ncols + c] - rh[k * ncols + c]) / lam;
            }
            if (p == 0) xe[m] = v;
            else xo[m] = v;
        }
    }
#pragma unroll
    for (int j = 0; j < H; ++j) {
        double e = 0.0, o = 0.0;
#pragma unroll
        for (int m = 0; m < H; ++m) {
            e = fma(Ch[m * H + j], xe[m], e);
            o = fma(Ch[H * H + m * H + j], xo[m], o);
        }
        out[j * ncols + c] = e + o;
        out[(NTT - 1 - j) * ncols + c] = e - o;
    }
}

// ---------------------------------------------------------------------------- t axis, two waves per column
// Columns too long for one thread's registers (Nt = 64 at BASELINE config 4, 1024 x 1024 x 64:
// 32 folded pairs + 32 outputs + the INIT moments would need ~180 VGPRs).  A wave pair shares 64
// columns: the even wave (role 0) owns the even outputs k = 2m (E s, s_j = x_j + x_{NTT-1-j}), the
// odd wave (role 1) the odd ones (O d, d_j = x_j - x_{NTT-1-j}).  Each wave reads the whole column
// itself (the partner's second read of the same lines is an L2 hit), so the forward needs no
// exchange; the inverse exchanges its half sums e_j / o_j through LDS in chunks of 8 rows
// (out_j = e_j + o_j, out_{NTT-1-j} = e_j - o_j).  Per wave the matrix half is wave-uniform
// (E or O: scalar loads), and every plane is read and written as 64 contiguous doubles per
// wave instruction -- the strided FFT this replaces ran at ~1 TB/s (64 planes 8 MB apart per
// block).
constexpr int TP_CH = 8;   // inverse: rows per LDS exchange chunk

// (64 points: 32 folded values + 16 moment sums + the recurrence need ~130 VGPRs: 3 waves per
// SIMD, no spills)
template <int NTT, int MODE>
__global__ __launch_bounds__(TC_NTH) __attribute__((amdgpu_waves_per_eu(NTT > 48 ? 3 : 4))) void k_dct_tp_fwd_init(
        SpecTab T, const double* __restrict__ Ch, const double* __restrict__ in, double* __restrict__ bh, SStep* Sg,
        RedBuf rb, double rtol, int maxiter, double* gath, int rank) {
    constexpr int H = NTT / 2;
    static_assert(NTT % 2 == 0 && H % TP_CH == 0, "even column length, whole exchange chunks");
    const int64_t ncols = (int64_t)T.nyl * T.Nx;
    const int lane = threadIdx.x & 63;
    const int role = __builtin_amdgcn_readfirstlane((threadIdx.x >> 6) & 1);       // 0 even, 1 odd
    const int pair = __builtin_amdgcn_readfirstlane(threadIdx.x >> 7);
    const int64_t c = ((int64_t)blockIdx.x * (TC_NTH / 128) + pair) * 64 + lane;
    const SStep S0 = *Sg;
    const double c0 = S0.ic0, ic1 = 1.0 / S0.ic1;   // INIT interval (previous solve's b^ measure)
    double acc[NMOM];
#pragma unroll
    for (int m = 0; m < NMOM; ++m) acc[m] = 0.0;
    __shared__ double mts[NTT];
    for (int i = threadIdx.x; i < NTT; i += TC_NTH) mts[i] = T.mt[i];
    __syncthreads();
    if (c < ncols) {
        const int kyl = (int)(c / T.Nx), kx = (int)(c - (int64_t)kyl * T.Nx), ky = T.y0 + kyl;
        const double myv = T.my[ky], mxv = T.mx[kx];
        const double sg = role ? -1.0 : 1.0;
        double v[H];   // s (even wave) or d (odd wave)
#pragma unroll
        for (int j = 0; j < H; ++j) v[j] = in[j * ncols + c] + sg * in[(NTT - 1 - j) * ncols + c];
        const double* M = Ch + role * H * H;   // E or O, wave-uniform
#pragma unroll
        for (int m = 0; m < H; ++m) {
            double X = 0.0;
#pragma unroll
            for (int j = 0; j < H; ++j) X = fma(M[m * H + j], v[j], X);
            const int k = 2 * m + role;
            bh[k * ncols + c] = X;
            if constexpr (MODE == TC_PLAIN) continue;
            const double lam = T.reps + T.r * ((mts[k] + myv) + mxv);   // spec_lam's order
            cheb_moments_acc<1, NMOM>(acc, (lam - c0) * ic1, X);
        }
    }
    if constexpr (MODE == TC_PLAIN) return;
    __shared__ double tot[NACC];
    if (!grid_reduce_last_rs<NMOM, TC_NTH>(acc, rb, tot)) return;
    if (init_moments_handed_over<MODE == TC_PLAN, TC_NTH>(tot, gath, rank)) return;
    sstep_plan_wave(Sg, S0, tot, 1, rtol, maxiter);
}

template <int NTT, bool PLAIN = false>
__global__ __launch_bounds__(TC_NTH) __attribute__((amdgpu_waves_per_eu(4))) void k_dct_tp_inv_xhat(
        SpecTab T, const double* __restrict__ Ch, const double* __restrict__ bh, const double* __restrict__ rh,
        const SStep* Sg, double* __restrict__ out) {
    constexpr int H = NTT / 2;
    const int64_t ncols = (int64_t)T.nyl * T.Nx;
    const int lane = threadIdx.x & 63;
    const int role = __builtin_amdgcn_readfirstlane((threadIdx.x >> 6) & 1);
    const int pair = __builtin_amdgcn_readfirstlane(threadIdx.x >> 7);
    const int64_t c = ((int64_t)blockIdx.x * (TC_NTH / 128) + pair) * 64 + lane;
    const bool ok = c < ncols;
    if (!PLAIN && Sg->k == 0) rh = bh;   // no pass ran: r = b^, x^ = 0
    __shared__ double xs[TC_NTH / 128][2][TP_CH][64];   // [pair][role][row of chunk][column]
    double xk[H];   // x^_{2m + role}
    if (ok) {
        const int kyl = (int)(c / T.Nx), kx = (int)(c - (int64_t)kyl * T.Nx), ky = T.y0 + kyl;
#pragma unroll
        for (int m = 0; m < H; ++m) {
            const int k = 2 * m + role;
            if constexpr (PLAIN) {
                xk[m] = bh[k * ncols + c];
            } else {
                const double lam = spec_lam(T, T.mt[k] + T.my[ky], kx);
                xk[m] = (bh[k * ncols + c] - rh[k * ncols + c]) / lam;
            }
        }
    } else {
#pragma unroll
        for (int m = 0; m < H; ++m) xk[m] = 0.0;
    }
    const double* M = Ch + role * H * H;
#pragma unroll
    for (int j0 = 0; j0 < H; j0 += TP_CH) {
#pragma unroll
        for (int jj = 0; jj < TP_CH; ++jj) {
            double e = 0.0;
#pragma unroll
            for (int m = 0; m < H; ++m) e = fma(M[m * H + j0 + jj], xk[m], e);
            xs[pair][role][jj][lane] = e;
        }
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < TP_CH; ++jj) {
            const double e = xs[pair][0][jj][lane], o = xs[pair][1][jj][lane];
            const int j = j0 + jj;
            if (ok) {
                if (role == 0) out[j * ncols + c] = e + o;
                else out[(NTT - 1 - j) * ncols + c] = e - o;
            }
        }
        __syncthreads();
    }
}

#define FOTO_TPAIR_SIZES(X) X(48) X(64)

#define FOTO_TCOL_SIZES(X) X(2) X(4) X(6) X(8) X(10) X(12) X(14) X(16) X(20) X(24) X(32)

#include "foto_gauss.inc"

static bool tcol_supported(int n) {
#define FOTO_TCOL_CASE(NN) if (n == NN) return true;
    FOTO_TCOL_SIZES(FOTO_TCOL_CASE)
    FOTO_TPAIR_SIZES(FOTO_TCOL_CASE)
#undef FOTO_TCOL_CASE
    return false;
}
static bool tpair_size(int n) {
#define FOTO_TCOL_CASE(NN) if (n == NN) return true;
    FOTO_TPAIR_SIZES(FOTO_TCOL_CASE)
#undef FOTO_TCOL_CASE
    return false;
}

// ============================================================================ plan

static int split_start_h(int n, int W, int h) {
    const int base = n / W, extra = n % W;
    return h * base + std::min(h, extra);
}

struct SpecImpl {
    Geo g{};
    int rank = 0, world = 1;
    int y0 = 0, nyl = 0;          // spectral box rows (sharded: Ny split over ranks)
    double r = 1, eps = 0;
    double *bh = nullptr, *rh = nullptr, *ph = nullptr, *tmp = nullptr;   // spectral box
    double* tmpp = nullptr;       // physical slab scratch (one halo plane per side: tmpp[-nxy ..])
    double *Cx = nullptr, *Cy = nullptr, *Ct = nullptr, *CxT = nullptr, *CyT = nullptr, *CtT = nullptr;
    double *mx = nullptr, *my = nullptr, *mt = nullptr;
    double *Fx = nullptr, *Fy = nullptr, *Ft = nullptr;   // FFT-DCT tables (nullptr: GEMM path)
    RedBuf rb{};
    double* gath = nullptr;       // s = 1: 2 doubles; s-step sharded: world * NACC
    CGScal* S = nullptr;
    CGScal* hS = nullptr;
    SStep* S2 = nullptr;
    SStep* hS2 = nullptr;
    int nblocks2 = 0;
    bool ring = false;   // s-step passes by the LDS-ring kernel
    int nb_ring = 0;
    double* Cth = nullptr;        // t-axis DCT-II even | odd halves (column kernels)
    bool tcol = false;            // single shard, s-step, Nt in FOTO_TCOL_SIZES
    int tcol_nb = 0;              // column kernels' blocks
    int last_passes = 0;          // passes of the previous s-step solve (first chunk size)
    // deferred solves in flight (solve_deferred -> finish), oldest first: one for the s-step
    // CG, up to two for the Gauss CG (two outer iterations in flight)
    struct Pend {
        int launched = 0, maxiter = 0, hslot = 0;
        double rtol = 0.0;
        double *b = nullptr, *x = nullptr;
    };
    Pend pq[2];
    int npend = 0;
    int sstep = 1;
    Tuning tn;                    // the knobs as the owning context read them (init's argument)
    DevArena mem;                 // every device block of the plan
    int nblocks = 0;
    double c0 = 0, c1 = 1;
    // Gauss-compressed CG (cg_mode 3, foto_gauss.inc); gauss_active: the solve in flight uses it
    bool gauss = false, gauss_active = false;
    GqState* gq = nullptr;
    GqState* hgq2[2] = {nullptr, nullptr};   // pinned: the header (K, status, conv, done, bn2, rn2) of
    int hslot = 0, hlast = 0;                // the last two solves (hslot: the next one's)
    GqState* dgq2[2] = {nullptr, nullptr};   // their device addresses (coherent host memory)
    GqNodes* gqn = nullptr;
    double* gq_hist = nullptr;    // world histograms (slot rank is this box's)
    double* gq_tab = nullptr;
    GqBins* gq_bins = nullptr;    // bin edges of the measure and the solution table
    GqQCos* gq_qcos = nullptr;    // the solution table's transform constants
    GqPub* gq_pub = nullptr;      // k_gq_cgtab's (alpha, beta) slots
    // bin-ordered histogram (k_gq_hist_perm): the box's voxels grouped by bin, chunked
    unsigned* gq_permv = nullptr;
    GqChunk* gq_chunks = nullptr;
    int gq_nch = 0;
    int* gq_cfirst = nullptr;     // [GQ_NB + 1] first chunk of each bin
    double* gq_rowmu = nullptr;   // mu_t + mu_y per box row
    double* gq_ppart = nullptr;   // [chunk id][GQ_NM] chunk sums
    GqExact* gq_exact = nullptr;  // exact bins (the whole grid's distinct eigenvalues)

    // k_spec_s2r LATE: working ring passes plan at their start; the pass a plan finishes marks
    // the solve done in its tail
    int late_plan() const { return ring ? 1 : 0; }

    int alloc(size_t bytes, void** p) { return mem.alloc(bytes, p); }
    ~SpecImpl() {
        mem.clear();   // (here, not as a member's destructor: the device blocks go before the pinned ones)
        if (hS) (void)hipHostFree(hS);
        if (hS2) (void)hipHostFree(hS2);
        for (GqState* h : hgq2)
            if (h) (void)hipHostFree(h);
    }
    SpecTab tab() const {
        SpecTab T;
        T.mt = mt; T.my = my; T.mx = mx; T.r = r; T.reps = r * eps;
        T.Nt = g.Nt; T.Ny = g.Ny; T.Nx = g.Nx;
        T.y0 = y0; T.nyl = nyl;
        return T;
    }
    bool vec() const { return (g.Nx % 2) == 0; }
    double nbox() const { return (double)g.Nt * nyl * g.Nx; }
};

// the s-step state as a fresh plan has it (c0, c1 for the column kernels' fused INIT)
static int reset_s2(SpecImpl* P, hipStream_t s) {
    SStep h{};
    h.c0 = P->c0;
    h.c1 = P->c1;
    h.gc0 = P->c0;
    h.gc1 = P->c1;
    h.ic0 = P->c0;   // the first solve's INIT moments: the whole spectrum
    h.ic1 = P->c1;
    h.flags = P->tn.sadapt ? 0 : 1;   // FOTO_SADAPT=0: whole-spectrum interval for every pass (A/B runs)
    *P->hS2 = h;
    FOTO_HIP_CHECK(hipMemcpyAsync(P->S2, P->hS2, sizeof(SStep), hipMemcpyHostToDevice, s));
    FOTO_HIP_CHECK(hipStreamSynchronize(s));   // hS2 is reused by polling
    return 0;
}

// k_gq_cgtab's slots as a fresh plan has them: every (alpha, beta) NaN, kdone -1, ticket 0
static int gq_pub_clear(SpecImpl* P, hipStream_t s) {
    if (!P->gq_pub) return 0;
    FOTO_HIP_CHECK(hipMemsetAsync(P->gq_pub, 0xff, sizeof(GqPub), s));   // (all-ones: NaN, -1)
    FOTO_HIP_CHECK(hipMemsetAsync(&P->gq_pub->ticket, 0, sizeof(unsigned), s));
    return 0;
}

// The bin-ordered voxel list of a box T (k_gq_hist_perm): per-row run counts by bin, a scan
// over the rows of each bin, the bins' first entries (host and device), then every row writes
// its runs.  perm (rows * Nx), rowmu (rows), first_d / tot_d (GQ_NB + 1 / GQ_NB) are the
// caller's; the count table is scratch.
static int gq_perm_lists(SpecImpl* P, const SpecTab& T, unsigned* perm, double* rowmu, int* first_d, int* tot_d,
                         std::vector<int>& htot, std::vector<int>& hfirst, hipStream_t s) {
    const int rows = T.Nt * T.nyl;
    const int64_t N = (int64_t)rows * T.Nx;
    k_gq_rowmu<<<(rows + 255) / 256, 256, 0, s>>>(T, rowmu);
    FOTO_HIP_CHECK(hipGetLastError());
    DevArena scratch;   // (freed on every return)
    int* cnt = nullptr;
    const size_t ncnt = (size_t)GQ_NB * rows;
    FOTO_TRY(scratch.alloc_n(ncnt, &cnt));
    htot.assign(GQ_NB, 0);
    hfirst.assign(GQ_NB + 1, 0);
    FOTO_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(int) * ncnt, s));
    k_gq_perm_count<<<(rows + 255) / 256, 256, 0, s>>>(T, P->gq_bins, rowmu, 1.0 / P->c1, cnt);
    k_gq_perm_scan<<<GQ_NB, 256, 0, s>>>(rows, cnt, tot_d);
    FOTO_HIP_CHECK(hipMemcpyAsync(htot.data(), tot_d, sizeof(int) * GQ_NB, hipMemcpyDeviceToHost, s));
    FOTO_HIP_CHECK(hipStreamSynchronize(s));
    int64_t acc = 0;
    for (int bb = 0; bb < GQ_NB; ++bb) {
        hfirst[bb] = (int)acc;
        acc += htot[bb];
    }
    hfirst[GQ_NB] = (int)acc;
    if (acc != N) {
        set_error("gauss perm: %lld voxels binned, box has %lld", (long long)acc, (long long)N);
        return FOTO_ERR_STATE;
    }
    FOTO_HIP_CHECK(hipMemcpyAsync(first_d, hfirst.data(), sizeof(int) * (GQ_NB + 1), hipMemcpyHostToDevice, s));
    k_gq_perm_fill<<<(rows + 255) / 256, 256, 0, s>>>(T, P->gq_bins, rowmu, 1.0 / P->c1, cnt, first_d, perm);
    FOTO_HIP_CHECK(hipGetLastError());
    FOTO_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

// The chunk list in dispatch order.  Neighbouring bins share the cache lines of b^ (a 16-voxel
// line holds runs of ~2 bins of a row), and a bin's chunks walk the rows in order, so the chunks
// of all bins over the same rows read the same lines at about the same time -- from the same L2
// only if they run on the same XCD.  Workgroups go round-robin to the 8 XCDs (block k to XCD
// k % 8) and a block's 4 waves take slots 4k .. 4k + 3: slot lists are filled so that XCD x
// gets the chunks whose first row lies in the x-th eighth of the rows (lists too short keep bin order).
// The sums go to part[chunk id] either way, so the histogram is bit-identical.
static int gq_order_chunks(SpecImpl* P, std::vector<GqChunk>& ch, int rows, hipStream_t s) {
    const int nx = 8;
    const int n = (int)ch.size();
    if (n < 4 * nx) return 0;
    std::vector<int> row(n);
    {
        DevArena scratch;   // (freed on every return and before the host-side ordering)
        void* b = nullptr;
        FOTO_TRY(scratch.alloc(sizeof(GqChunk) * n + sizeof(int) * n, &b));
        GqChunk* dch = (GqChunk*)b;
        int* drow = (int*)(dch + n);
        FOTO_HIP_CHECK(hipMemcpyAsync(dch, ch.data(), sizeof(GqChunk) * n, hipMemcpyHostToDevice, s));
        k_gq_chunk_rows<<<(n + 255) / 256, 256, 0, s>>>(dch, n, P->gq_permv, drow);
        FOTO_HIP_CHECK(hipGetLastError());
        FOTO_HIP_CHECK(hipMemcpyAsync(row.data(), drow, sizeof(int) * n, hipMemcpyDeviceToHost, s));
        FOTO_HIP_CHECK(hipStreamSynchronize(s));
    }
    std::vector<std::vector<int>> L(nx);
    for (int c = 0; c < n; ++c) L[std::min(nx - 1, (int)((int64_t)row[c] * nx / std::max(1, rows)))].push_back(c);
    std::vector<size_t> at(nx, 0);
    const int nb = (n + 3) / 4;
    std::vector<GqChunk> out((size_t)nb * 4, GqChunk{0, 0, 0, -1});
    for (int k = 0; k < nb; ++k)
        for (int w = 0; w < 4; ++w) {
            int x = k % nx;
            if (at[x] == L[x].size()) {   // this XCD's share is used up: the longest remaining list
                size_t best = 0;
                x = -1;
                for (int y = 0; y < nx; ++y)
                    if (L[y].size() - at[y] > best) { best = L[y].size() - at[y]; x = y; }
                if (x < 0) continue;
            }
            out[(size_t)k * 4 + w] = ch[L[x][at[x]++]];
        }
    ch.swap(out);
    return 0;
}

// this box's list and chunks, and the exact bins of the whole grid (from the box's list when the
// box is the grid, else from a scratch list of the grid: every rank derives the same table)
static int gq_build_perm(SpecImpl* P, hipStream_t s) {
    const SpecTab T = P->tab();
    // exact bins of at most GQ_M points (their points are the rule).  FOTO_GQ_EXACT (A/B): -1
    // none; up to GQ_XS = 16 also takes bins of 9-16 points through the Stieltjes procedure --
    // measured less accurate (the 5-step iterate of an 8x24x20 grid 1.6e-10 from scipy's against
    // 2.3e-12; the node / weight solve loses digits on clustered points), not the default
    const int xmax = P->tn.gq_exact != Tuning::AUTO ? std::min(P->tn.gq_exact, GQ_XS) : GQ_M;
    const int rows = P->g.Nt * P->nyl;
    const int64_t N = (int64_t)rows * P->g.Nx;
    void* b = nullptr;
    FOTO_TRY(P->alloc(sizeof(double) * rows, &b)); P->gq_rowmu = (double*)b;
    FOTO_TRY(P->alloc(sizeof(unsigned) * N, &b)); P->gq_permv = (unsigned*)b;
    FOTO_TRY(P->alloc(sizeof(int) * (2 * GQ_NB + 1), &b));
    int* first_d = (int*)b;
    int* tot_d = first_d + GQ_NB + 1;
    std::vector<int> htot, hfirst;
    FOTO_TRY(gq_perm_lists(P, T, P->gq_permv, P->gq_rowmu, first_d, tot_d, htot, hfirst, s));
    std::vector<GqChunk> ch;
    std::vector<int> cfirst(GQ_NB + 1);
    for (int bb = 0; bb < GQ_NB; ++bb) {
        cfirst[bb] = (int)ch.size();
        for (int st = 0; st < htot[bb]; st += GQ_PCH)
            ch.push_back(GqChunk{bb, hfirst[bb] + st, std::min(GQ_PCH, htot[bb] - st), (int)ch.size()});
    }
    cfirst[GQ_NB] = (int)ch.size();
    const int nch = (int)ch.size();
    FOTO_TRY(P->alloc(sizeof(int) * (GQ_NB + 1), &b)); P->gq_cfirst = (int*)b;
    FOTO_TRY(P->alloc(sizeof(double) * GQ_NM * std::max(1, nch), &b)); P->gq_ppart = (double*)b;
    FOTO_TRY(gq_order_chunks(P, ch, rows, s));
    P->gq_nch = (int)ch.size();
    FOTO_TRY(P->alloc(sizeof(GqChunk) * std::max<size_t>(1, ch.size()), &b)); P->gq_chunks = (GqChunk*)b;
    FOTO_HIP_CHECK(hipMemcpyAsync(P->gq_chunks, ch.data(), sizeof(GqChunk) * ch.size(), hipMemcpyHostToDevice, s));
    FOTO_HIP_CHECK(hipMemcpyAsync(P->gq_cfirst, cfirst.data(), sizeof(int) * (GQ_NB + 1), hipMemcpyHostToDevice, s));
    if (P->nyl == P->g.Ny) {
        k_gq_exact<<<GQ_NB / 64, 64, 0, s>>>(T, P->gq_permv, first_d, tot_d, P->gq_rowmu, 1.0 / P->c1, xmax, P->gq_exact);
        FOTO_HIP_CHECK(hipGetLastError());
        FOTO_HIP_CHECK(hipStreamSynchronize(s));
        return 0;
    }
    SpecTab TG = T;   // the whole grid
    TG.y0 = 0;
    TG.nyl = P->g.Ny;
    const int grows = P->g.Nt * P->g.Ny;
    DevArena scratch;   // (freed on every return)
    unsigned* gperm = nullptr;
    double* growmu = nullptr;
    int* gidx = nullptr;
    FOTO_TRY(scratch.alloc_n((size_t)grows * P->g.Nx, &gperm));
    FOTO_TRY(scratch.alloc_n((size_t)grows, &growmu));
    FOTO_TRY(scratch.alloc_n((size_t)(2 * GQ_NB + 1), &gidx));
    FOTO_TRY(gq_perm_lists(P, TG, gperm, growmu, gidx, gidx + GQ_NB + 1, htot, hfirst, s));
    k_gq_exact<<<GQ_NB / 64, 64, 0, s>>>(TG, gperm, gidx, gidx + GQ_NB + 1, growmu, 1.0 / P->c1, xmax, P->gq_exact);
    FOTO_HIP_CHECK(hipGetLastError());
    FOTO_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

int SpectralPlan::init(const Geo& g, int rank, int world, double r, double eps, int sstep, const Tuning& tn,
                       hipStream_t s) {
    // cg_mode 3: the Gauss-compressed CG, with the s-step machinery kept for the (rare) redo
    const bool gauss = (sstep == 3);
    if (gauss) sstep = 2;
    if (sstep != 1 && sstep != 2) {
        set_error("spectral CG: s-step must be 1 or 2");
        return FOTO_ERR_ARG;
    }
    if (world > 1 && sstep != 2) {
        set_error("sharded spectral CG needs cg_mode = 2 (s-step)");
        return FOTO_ERR_ARG;
    }
    if (world > g.Ny) {
        set_error("sharded spectral CG needs Ny >= world (rows are split over ranks)");
        return FOTO_ERR_ARG;
    }
    if (!(eps > 0.0)) {
        set_error("spectral CG needs reg_epsilon > 0 (x = (b - r) / lam)");
        return FOTO_ERR_ARG;
    }
    auto* P = new SpecImpl();
    impl = P;
    P->sstep = sstep;
    P->tn = tn;
    P->g = g;
    P->rank = rank;
    P->world = world;
    P->y0 = split_start_h(g.Ny, world, rank);
    P->nyl = split_start_h(g.Ny, world, rank + 1) - P->y0;
    P->r = r;
    P->eps = eps;
    const size_t NB = (size_t)g.Nt * P->nyl * g.Nx;          // spectral box
    const size_t NS = (size_t)g.nloc * g.nxy;                // physical slab
    void* b;
    FOTO_TRY(P->alloc(NB * 8, &b)); P->bh = (double*)b;
    FOTO_TRY(P->alloc(NB * 8, &b)); P->rh = (double*)b;
    FOTO_TRY(P->alloc(NB * 8, &b)); P->ph = (double*)b;
    FOTO_TRY(P->alloc(std::max(NB, NS) * 8, &b)); P->tmp = (double*)b;
    if (world > 1) {
        FOTO_TRY(P->alloc((NS + 2 * (size_t)g.nxy) * 8, &b)); P->tmpp = (double*)b + g.nxy;
    }
    std::vector<double> C, CT, mu;
    // the n x n matrices only for an axis the FFT kernels do not take (dct_fft_axis's rule):
    // 2 x 3.3 MB of host cosines and blocking copies per 640-axis saved at context creation
    auto up = [&](int n, double** Cd, double** CTd, double** mud) -> int {
        int m1, m2;
        const bool fft = tn.dct_fft && n >= 64 && fft_factors(n, &m1, &m2);
        if (fft) dct_eigen(n, mu);
        else dct_matrix(n, C, CT, mu);
        void* p;
        if (!fft) {
            FOTO_TRY(P->alloc(C.size() * 8, &p)); *Cd = (double*)p;
            FOTO_TRY(P->alloc(CT.size() * 8, &p)); *CTd = (double*)p;
            FOTO_HIP_CHECK(hipMemcpy(*Cd, C.data(), C.size() * 8, hipMemcpyHostToDevice));
            FOTO_HIP_CHECK(hipMemcpy(*CTd, CT.data(), CT.size() * 8, hipMemcpyHostToDevice));
        }
        FOTO_TRY(P->alloc(mu.size() * 8, &p)); *mud = (double*)p;
        FOTO_HIP_CHECK(hipMemcpy(*mud, mu.data(), mu.size() * 8, hipMemcpyHostToDevice));
        return (int)0;
    };
    FOTO_TRY(up(g.Nx, &P->Cx, &P->CxT, &P->mx));
    const double mx_max = mu.back();
    FOTO_TRY(up(g.Ny, &P->Cy, &P->CyT, &P->my));
    const double my_max = mu.back();
    FOTO_TRY(up(g.Nt, &P->Ct, &P->CtT, &P->mt));
    const double mt_max = mu.back();
    auto upf = [&](int n, double** Fd) -> int {
        int m1, m2;
        if (!tn.dct_fft || !fft_factors(n, &m1, &m2)) return 0;   // (no table: dct_pass takes the GEMM kernels)
        const std::vector<double> t = fft_table(n);
        void* p;
        FOTO_TRY(P->alloc(t.size() * 8, &p));
        *Fd = (double*)p;
        FOTO_HIP_CHECK(hipMemcpy(*Fd, t.data(), t.size() * 8, hipMemcpyHostToDevice));
        return 0;
    };
    FOTO_TRY(upf(g.Nx, &P->Fx));
    FOTO_TRY(upf(g.Ny, &P->Fy));
    FOTO_TRY(upf(g.Nt, &P->Ft));
    // Chebyshev scaling of lam: global spectrum bounds (identical on every rank)
    const double lmin = r * eps, lmax = r * eps + r * (mt_max + my_max + mx_max);
    P->c0 = 0.5 * (lmax + lmin);
    P->c1 = 0.5 * (lmax - lmin);
    const int rows = g.Nt * P->nyl;
    const int ntiles = ((g.Nx + 127) / 128) * ((rows + 3) / 4);
    P->nblocks = std::min(ntiles, 2048);
    {
        // one resident wave of blocks: blocks per CU at the pass kernel's occupancy x CUs
        const int ntiles2 = ((g.Nx + 127) / 128) * ((rows + S2_NTH / 64 - 1) / (S2_NTH / 64));
        int dev = 0, cus = 256, per_cu = 0;
        FOTO_HIP_CHECK(hipGetDevice(&dev));
        FOTO_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        FOTO_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_spec_s2<true, false, true>, S2_NTH, 0));
        P->nblocks2 = std::min(ntiles2, std::max(1, per_cu) * cus);
        // ring-fed pass (k_spec_s2r): one 1024-thread block per CU (its LDS ring), at most one
        // block per 16 wave tiles; FOTO_RING=0 selects the register-fed pass (A/B runs)
        P->ring = ring_ok(P->tab()) && tn.ring;
        const int nwt = ((g.Nx + 127) / 128) * rows;
        P->nb_ring = std::max(1, std::min({P->nblocks2, cus, (nwt + RING_NW - 1) / RING_NW}));
    }
    // FOTO_TCOL=0: t axis by dct_pass + separate INIT / xhat passes (A/B runs)
    P->tcol = sstep == 2 && tcol_supported(g.Nt) && tn.tcol;
    if (P->tcol) {
        const int H = g.Nt / 2;
        dct_matrix(g.Nt, C, CT, mu);
        std::vector<double> ch((size_t)2 * H * H);
        for (int m = 0; m < H; ++m)
            for (int j = 0; j < H; ++j) {
                ch[(size_t)m * H + j] = C[(size_t)(2 * m) * g.Nt + j];
                ch[(size_t)H * H + m * H + j] = C[(size_t)(2 * m + 1) * g.Nt + j];
            }
        FOTO_TRY(P->alloc(ch.size() * 8, &b));
        P->Cth = (double*)b;
        FOTO_HIP_CHECK(hipMemcpy(P->Cth, ch.data(), ch.size() * 8, hipMemcpyHostToDevice));
        const int per_block = tpair_size(g.Nt) ? TC_NTH / 2 : TC_NTH;   // wave pairs: 64 columns per 2 waves
        P->tcol_nb = (int)(((int64_t)P->nyl * g.Nx + per_block - 1) / per_block);
    }
    const int cap = std::max({2 * P->nblocks, NACC * P->nblocks2, NMOM * P->tcol_nb});
    FOTO_TRY(P->alloc(sizeof(double) * (cap + 8), &b));
    P->rb.partials = (double*)b;
    P->rb.ticket = (unsigned*)((double*)b + cap);
    P->rb.cap = cap;
    FOTO_HIP_CHECK(hipMemsetAsync(P->rb.ticket, 0, 8 * sizeof(double), s));
    FOTO_TRY(P->alloc(sizeof(double) * std::max(4, NACC * world), &b)); P->gath = (double*)b;
    FOTO_TRY(P->alloc(sizeof(CGScal), &b)); P->S = (CGScal*)b;
    FOTO_HIP_CHECK(hipHostMalloc((void**)&P->hS, sizeof(CGScal)));
    FOTO_TRY(P->alloc(sizeof(SStep), &b)); P->S2 = (SStep*)b;
    FOTO_HIP_CHECK(hipHostMalloc((void**)&P->hS2, sizeof(SStep)));
    FOTO_TRY(reset_s2(P, s));
    // the Gauss-compressed CG needs the bin-ordered voxel list; boxes its packing does not
    // cover run the s-step CG (decided on the whole grid, so every rank agrees)
    P->gauss = gauss && gq_perm_ok(g.Nx, g.Nt * g.Ny);
    if (P->gauss) {
        FOTO_TRY(P->alloc(sizeof(GqState), &b)); P->gq = (GqState*)b;
        FOTO_HIP_CHECK(hipMemsetAsync(P->gq, 0, sizeof(GqState), s));
        for (int k = 0; k < 2; ++k) {
            FOTO_HIP_CHECK(hipHostMalloc((void**)&P->hgq2[k], sizeof(GqState), hipHostMallocMapped | hipHostMallocCoherent));
            std::memset((void*)P->hgq2[k], 0, sizeof(GqState));
            FOTO_HIP_CHECK(hipHostGetDevicePointer((void**)&P->dgq2[k], P->hgq2[k], 0));
        }
        FOTO_TRY(P->alloc(sizeof(GqNodes), &b)); P->gqn = (GqNodes*)b;
        FOTO_TRY(P->alloc(sizeof(double) * GQ_HIST * world, &b)); P->gq_hist = (double*)b;
        FOTO_TRY(P->alloc(GQ_TAB_BYTES, &b)); P->gq_tab = (double*)b;
        // k_gq_xhat holds the whole table (128 KB) in dynamic LDS, beside its 10 KB bin tables
        FOTO_HIP_CHECK(hipFuncSetAttribute((const void*)k_gq_xhat, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)GQ_TAB_BYTES));
        FOTO_TRY(P->alloc(sizeof(GqBins), &b)); P->gq_bins = (GqBins*)b;
        k_gq_bins<<<1, 256, 0, s>>>(P->gq_bins);
        FOTO_TRY(P->alloc(sizeof(GqQCos), &b)); P->gq_qcos = (GqQCos*)b;
        k_gq_qcos<<<1, 256, 0, s>>>(P->gq_qcos);
        FOTO_TRY(P->alloc(sizeof(GqPub), &b)); P->gq_pub = (GqPub*)b;
        FOTO_TRY(gq_pub_clear(P, s));
        FOTO_HIP_CHECK(hipGetLastError());
        FOTO_TRY(P->alloc(sizeof(GqExact), &b)); P->gq_exact = (GqExact*)b;
        FOTO_TRY(gq_build_perm(P, s));
        FOTO_HIP_CHECK(hipStreamSynchronize(s));
    }
    return 0;
}

SpectralPlan::~SpectralPlan() { delete impl; }

// ---------------------------------------------------------------------------- launchers

// one axis of [outer][n][inner]: FFT kernels where the length has an instantiation, GEMM otherwise
static hipError_t dct_pass(const SpecImpl* P, int axis, bool inv, int outer, int inner, const double* in, double* out,
                           hipStream_t s) {
    const double* tab = axis == 0 ? P->Fx : axis == 1 ? P->Fy : P->Ft;
    const int n = axis == 0 ? P->g.Nx : axis == 1 ? P->g.Ny : P->g.Nt;
    const hipError_t e = dct_fft_axis(outer, n, inner, inv, tab, in, out, s);
    if (e != hipErrorNotSupported) return e;
    const double* C = axis == 0 ? (inv ? P->CxT : P->Cx) : axis == 1 ? (inv ? P->CyT : P->Cy) : (inv ? P->CtT : P->Ct);
    return dct_axis(outer, n, inner, C, in, out, s);
}

// One s-step pass (init: r^ = b^ and r_0's moments).  Single shard: the pass plans the next one
// itself; sharded: its moments go to gath for the all-gather and cg_plan -- except the working
// ring passes, which plan at their start from the moments gathered from all `world` ranks (LATE).
static hipError_t launch_s2(SpecImpl* P, bool init, double rtol, int maxiter, hipStream_t s) {
    const SpecTab T = P->tab();
    const bool fuse = P->world == 1;
    if (P->ring)
        return launch_s2_ring(T, P->rh, P->ph, P->bh, P->S2, P->rb, rtol, maxiter, P->gath, P->rank, init,
                              fuse || !init, P->nb_ring, s, init ? 1 : P->world);
    return with_bools([&](auto V, auto I, auto F) {
        k_spec_s2<V(), I(), F()><<<P->nblocks2, S2_NTH, 0, s>>>(T, P->rh, P->ph, P->bh, P->S2, P->rb, rtol, maxiter,
                                                                 P->gath, P->rank);
        return hipGetLastError();
    }, P->vec(), init, fuse);
}

// the one-step CG's r^ = b^ and iteration k
static hipError_t launch_init(SpecImpl* P, hipStream_t s) {
    return with_bools([&](auto V) {
        k_spec_init<V()><<<P->nblocks, NT, 0, s>>>(P->tab(), P->bh, P->rh, P->rb, P->gath);
        return hipGetLastError();
    }, P->vec());
}
static hipError_t launch_cg(SpecImpl* P, int k, double rtol, hipStream_t s) {
    return with_bools([&](auto V) {
        k_spec_cg<V()><<<P->nblocks, NT, 0, s>>>(P->tab(), k, P->rh, P->ph, P->S, P->rb, P->gath, rtol);
        return hipGetLastError();
    }, P->vec());
}

// x^ = (b^ - r^) / lam into a box buffer
static hipError_t launch_xhat(SpecImpl* P, double* out, hipStream_t s) {
    return with_bools([&](auto V) {
        k_spec_xhat<V()><<<P->nblocks, NT, 0, s>>>(P->tab(), P->bh, P->rh, out);
        return hipGetLastError();
    }, P->vec());
}

// x^ = Q(lam) b^ (the Gauss-compressed CG's solution table) into a box buffer: persistent
// 1024-thread blocks, the table in LDS.  Sized for the whole table (32 rows, 128 KB) one block
// fits a CU; sized for the first GQ_XQL = 17 rows (68 KB, what K <= ~200 needs; the table
// kernel's qn is not known when this launch is enqueued) two fit, and any rows beyond are read
// from the global table.
static hipError_t gq_xhat(SpecImpl* P, double* out, hipStream_t s) {
    const SpecTab T = P->tab();
    const int rows = P->g.Nt * P->nyl;
    constexpr int ql = GQ_XQL;
    static_assert(ql > 0 && ql < GQ_QN, "the LDS part of the table: two blocks per CU");
    const int per_cu = 2;
    const int nb = std::max(1, std::min(per_cu * cus_count(), (rows + GQ_XNTH / 64 - 1) / (GQ_XNTH / 64)));
    k_gq_xhat<<<nb, GQ_XNTH, (size_t)ql * GQ_QB * sizeof(double), s>>>(T, P->bh, P->gq_tab, P->gq, P->gq_bins,
                                                                       1.0 / P->c1, out, ql);
    return hipGetLastError();
}

// The t-axis column kernels.  Forward (in -> b^) in one of the TC_* modes: TC_PLAN, a single
// shard, the kernel plans the first pass; TC_GATH, sharded, it leaves this rank's INIT moments in
// gath for the all-gather; TC_PLAIN, b^ only.  Inverse (-> out): in == nullptr forms
// x^ = (b^ - r^)/lam in the kernel (s-step); otherwise in holds x^ itself (gq_xhat's output).
static hipError_t launch_tcol(SpecImpl* P, bool inv, const double* in, double* out, double rtol, int maxiter,
                              hipStream_t s, int mode = TC_PLAN) {
    const SpecTab T = P->tab();
    const int nb = P->tcol_nb;
#define FOTO_TCOL_FWD(NN, FWD, M) \
    FWD<NN, M><<<nb, TC_NTH, 0, s>>>(T, P->Cth, in, P->bh, P->S2, P->rb, rtol, maxiter, P->gath, P->rank)
#define FOTO_TCOL_LAUNCH(NN, FWD, INV)                                                                  \
    if (P->g.Nt == NN) {                                                                                \
        if (inv && in) INV<NN, true><<<nb, TC_NTH, 0, s>>>(T, P->Cth, in, nullptr, nullptr, out);       \
        else if (inv) INV<NN><<<nb, TC_NTH, 0, s>>>(T, P->Cth, P->bh, P->rh, P->S2, out);               \
        else if (mode == TC_PLAN) FOTO_TCOL_FWD(NN, FWD, TC_PLAN);                                      \
        else if (mode == TC_GATH) FOTO_TCOL_FWD(NN, FWD, TC_GATH);                                      \
        else FOTO_TCOL_FWD(NN, FWD, TC_PLAIN);                                                          \
        return hipGetLastError();                                                                       \
    }
#define FOTO_TCOL_ONE(NN) FOTO_TCOL_LAUNCH(NN, k_dct_t_fwd_init, k_dct_t_inv_xhat)
#define FOTO_TCOL_PAIR(NN) FOTO_TCOL_LAUNCH(NN, k_dct_tp_fwd_init, k_dct_tp_inv_xhat)
    FOTO_TCOL_SIZES(FOTO_TCOL_ONE)
    FOTO_TPAIR_SIZES(FOTO_TCOL_PAIR)
#undef FOTO_TCOL_PAIR
#undef FOTO_TCOL_ONE
#undef FOTO_TCOL_LAUNCH
#undef FOTO_TCOL_FWD
    return hipErrorNotSupported;
}

// ---------------------------------------------------------------------------- the transform chain
// forward = (Ct (x) Cy (x) Cx): x and y over a range of physical planes, then t over the spectral
// box; inverse = transpose: x^, t^-1 over the box, then y^-1 and x^-1 over planes.  The four
// stages below are the only places that launch a transform.  Which buffers a stage reads and
// writes is the caller's route (a single shard's s-step solve may clobber b, the Gauss CG's must
// not; a shard's planes pass through the all-to-all between the stages).
//
// A Span is one KTimer interval of class cls around the stages run under it; each stage adds the
// bytes it moves (8 per element read or written).
struct Span {
    KTimer* kt;
    hipStream_t s;
    int cls;
    hipEvent_t e;
    double bytes = 0.0;
    Span(KTimer* kt, hipStream_t s, int cls) : kt(kt), s(s), cls(cls), e(kt ? kt->start(s) : nullptr) {}
    int close() {
        if (kt) kt->stop(e, s, cls, bytes);
        return 0;
    }
};

// np planes: src -x-> mid -y-> dst
static int chain_fwd_xy(SpecImpl* P, Span& sp, int np, const double* src, double* mid, double* dst) {
    const Geo& g = P->g;
    FOTO_HIP_CHECK(dct_pass(P, 0, false, np * g.Ny, 1, src, mid, sp.s));
    FOTO_HIP_CHECK(dct_pass(P, 1, false, np, g.Nx, mid, dst, sp.s));
    sp.bytes += 4.0 * 8.0 * (double)np * (double)g.nxy;
    return 0;
}

// box src -t-> b^: the column kernel in the given TC_* mode where the plan has one
static int chain_fwd_t(SpecImpl* P, Span& sp, int mode, const double* src, double rtol, int maxiter) {
    if (P->tcol) FOTO_HIP_CHECK(launch_tcol(P, false, src, nullptr, rtol, maxiter, sp.s, mode));
    else FOTO_HIP_CHECK(dct_pass(P, 2, false, 1, P->nyl * P->g.Nx, src, P->bh, sp.s));
    sp.bytes += 2.0 * 8.0 * P->nbox();
    return 0;
}

// x^ -t^-1-> box out.  x^ is the s-step CG's (b^ - r^)/lam, the Gauss CG's Q(lam) b^, or already
// in xh.  The column kernel forms the s-step's x^ itself; every other x^ goes through xh.
enum XHat { XH_NONE, XH_SSTEP, XH_GAUSS };
static int chain_inv_t(SpecImpl* P, Span& sp, XHat src, double* xh, double* out) {
    if (src == XH_GAUSS) FOTO_HIP_CHECK(gq_xhat(P, xh, sp.s));
    else if (src == XH_SSTEP && !P->tcol) FOTO_HIP_CHECK(launch_xhat(P, xh, sp.s));
    if (P->tcol) FOTO_HIP_CHECK(launch_tcol(P, true, src == XH_SSTEP ? nullptr : xh, out, 0.0, 0, sp.s));
    else FOTO_HIP_CHECK(dct_pass(P, 2, true, 1, P->nyl * P->g.Nx, xh, out, sp.s));
    sp.bytes += (P->tcol ? 3.0 : 2.0) * 8.0 * P->nbox();
    return 0;
}

// np planes: src -y^-1-> mid -x^-1-> dst
static int chain_inv_yx(SpecImpl* P, Span& sp, int np, const double* src, double* mid, double* dst) {
    const Geo& g = P->g;
    FOTO_HIP_CHECK(dct_pass(P, 1, true, np, g.Nx, src, mid, sp.s));
    FOTO_HIP_CHECK(dct_pass(P, 0, true, np * g.Ny, 1, mid, dst, sp.s));
    sp.bytes += 4.0 * 8.0 * (double)np * (double)g.nxy;
    return 0;
}

// single shard: b (physical) -x-> tmp -y-> mid -t-> b^
static int forward(SpecImpl* P, const double* b, double* mid, int mode, double rtol, int maxiter, KTimer* kt,
                   hipStream_t s) {
    Span sp(kt, s, FOTO_K_DCT);
    FOTO_TRY(chain_fwd_xy(P, sp, P->g.Nt, b, P->tmp, mid));
    FOTO_TRY(chain_fwd_t(P, sp, mode, mid, rtol, maxiter));
    return sp.close();
}

// single shard: x^ -t^-1-> tb -y^-1-> mid -x^-1-> x (physical)
static int inverse(SpecImpl* P, XHat src, double* xh, double* tb, double* mid, double* x, KTimer* kt, hipStream_t s) {
    Span sp(kt, s, FOTO_K_DCT);
    FOTO_TRY(chain_inv_t(P, sp, src, xh, tb));
    // (bytes_k as it has been reported: here k_gq_xhat's read of b^ counts without the column
    // kernel too, which the sharded inv_t does not do)
    if (src == XH_GAUSS && !P->tcol) sp.bytes += 8.0 * P->nbox();
    FOTO_TRY(chain_inv_yx(P, sp, P->g.Nt, tb, mid, x));
    return sp.close();
}

// single shard, after the s-step or the one-step CG: (b^, r^) -> x with b as scratch.  Without
// the column kernels k_spec_xhat runs ahead of the timed chain.
static int inverse_sstep(SpecImpl* P, double* b, double* x, KTimer* kt, hipStream_t s) {
    if (!P->tcol) FOTO_HIP_CHECK(launch_xhat(P, P->tmp, s));
    return inverse(P, P->tcol ? XH_SSTEP : XH_NONE, P->tmp, b, P->tmp, x, kt, s);
}

// ---------------------------------------------------------------------------- s-step and one-step CG (host)

static int s2_launch(SpecImpl* P, bool init, double rtol, int maxiter, KTimer* kt, hipStream_t s) {
    hipEvent_t e = kt ? kt->start(s) : nullptr;
    FOTO_HIP_CHECK(launch_s2(P, init, rtol, maxiter, s));
    if (kt) kt->stop(e, s, FOTO_K_SPEC, (init ? 16.0 : 32.0) * P->nbox());
    return 0;
}

// n passes and, behind them, the copy of the state to the pinned hS2
template <class Pass>
static int enqueue_passes(SpecImpl* P, int n, Pass&& pass, hipStream_t s) {
    for (int j = 0; j < n; ++j) FOTO_TRY(pass());
    FOTO_HIP_CHECK(hipMemcpyAsync(P->hS2, P->S2, sizeof(SStep), hipMemcpyDeviceToHost, s));
    return 0;
}

// The s-step pass loop: the host polls the done flag between chunks of passes.  A poll idles the
// GPU for the host's wake-up (measured up to ~1 ms per solve when polling every pass), while a
// pass launched after the solve finished exits in a few us -- so over-predict: the first chunk is
// the previous solve's pass count + 2 (8 without one), then chunks of 2.  launched > 0: a
// deferred solve, whose passes and state copy the stream has passed; the loop only continues it.
// pass() enqueues one pass on each of `shards` local shards.
template <class Pass>
static int pass_loop(SpecImpl* P, int launched, int shards, int maxiter, Pass&& pass, int* iters, int* info,
                     KTimer* kt, hipStream_t s) {
    int passes = launched;
    while (passes == 0 || !P->hS2->done) {
        const int chunk = passes > 0 ? 2 : P->last_passes > 0 ? P->last_passes + 2 : 8;
        FOTO_TRY(enqueue_passes(P, chunk, pass, s));
        FOTO_HIP_CHECK(hipStreamSynchronize(s));
        passes += chunk;
        if (!P->hS2->done && passes > maxiter + 4) {
            set_error("spectral s-step CG did not terminate");
            return FOTO_ERR_STATE;
        }
    }
    *iters = P->hS2->iters;
    *info = (P->hS2->done == 1) ? 0 : maxiter;
    P->last_passes = P->hS2->passes;
    // S.passes counts the plans (INIT's and every working pass's but the last), i.e. the
    // passes that applied steps; the launches beyond them exited at once -- keep them out of
    // the per-kernel timing
    if (kt) kt->discard_last(FOTO_K_SPEC, std::max(0, passes - P->hS2->passes) * shards);
    return 0;
}

// b^ -> r^ by the s-step CG, waited for.  init_done: the fused t-axis kernel already reset the
// state, took r_0's moments and planned (no reset_s2, a host wait per solve: the INIT plan
// rewrites every field but the constant c0, c1, which init() set)
static int solve_s2(SpecImpl* P, double rtol, int maxiter, int* iters, int* info, KTimer* kt, hipStream_t s,
                    bool init_done) {
    if (!init_done) FOTO_TRY(s2_launch(P, true, rtol, maxiter, kt, s));
    return pass_loop(P, 0, 1, maxiter, [&] { return s2_launch(P, false, rtol, maxiter, kt, s); }, iters, info, kt, s);
}

// b^ -> r^ by the one-step CG (Chronopoulos-Gear), polled in chunks from `predicted` iterations
static int solve_s1(SpecImpl* P, double rtol, int maxiter, int predicted, int* iters, int* info, KTimer* kt,
                    hipStream_t s) {
    FOTO_HIP_CHECK(launch_init(P, s));
    FOTO_HIP_CHECK(hipMemsetAsync(P->S, 0, sizeof(CGScal), s));
    auto step = [&](int k) -> int {
        hipEvent_t e = kt ? kt->start(s) : nullptr;
        FOTO_HIP_CHECK(launch_cg(P, k, rtol, s));
        if (kt) kt->stop(e, s, FOTO_K_SPEC, (k == 0 ? 24.0 : 32.0) * P->nbox());
        return 0;
    };
    bool done = false;
    return cg_poll_chunks(predicted > 4 ? predicted - 3 : 8, maxiter, step, P->S, P->hS, s, &done, iters, info);
}

// ---------------------------------------------------------------------------- Gauss-compressed CG (host)
// one shard: k_gq_nodes_w sums the chunk sums itself (no histogram pass)
static bool gq_fused_reduce(const SpecImpl* P) { return P->world == 1; }

// b^ -> this box's histogram (slot rank of gq_hist)
static int gq_measure(SpecImpl* P, KTimer* kt, hipStream_t s) {
    const SpecTab T = P->tab();
    hipEvent_t e = kt ? kt->start(s) : nullptr;
    const int nbk = std::max(1, (P->gq_nch + 3) / 4);
    k_gq_hist_perm<<<nbk, 256, 0, s>>>(T, P->bh, P->gq_permv, P->gq_chunks, P->gq_nch, P->gq_bins, P->gq_exact,
                                       P->gq_rowmu, 1.0 / P->c1, P->gq_ppart);
    FOTO_HIP_CHECK(hipGetLastError());
    // (one shard: the node kernel takes the bin sums itself, from the chunk sums)
    if (!gq_fused_reduce(P)) {
        k_gq_perm_reduce<<<GQ_HIST / 4, 256, 0, s>>>(P->gq_ppart, P->gq_cfirst, P->gq_hist + (size_t)P->rank * GQ_HIST);
        FOTO_HIP_CHECK(hipGetLastError());
    }
    if (kt) kt->stop(e, s, FOTO_K_SPEC, 8.0 * P->nbox());
    return 0;
}

// the world histograms -> Gauss nodes -> CG coefficients -> solution table; header to host
static int gq_solve(SpecImpl* P, double rtol, int maxiter, KTimer* kt, hipStream_t s) {
    hipEvent_t e = kt ? kt->start(s) : nullptr;
    if (gq_fused_reduce(P))
        k_gq_nodes_w<<<GQ_NB / 4, 256, 0, s>>>(nullptr, P->gq_ppart, P->gq_cfirst, P->gq_bins, P->gq_exact, 1,
                                               P->r * P->eps, P->c1, P->gqn);
    else
        k_gq_nodes_w<<<GQ_NB / 4, 256, 0, s>>>(P->gq_hist, nullptr, nullptr, P->gq_bins, P->gq_exact, P->world,
                                               P->r * P->eps, P->c1, P->gqn);
    FOTO_HIP_CHECK(hipGetLastError());
    // FOTO_GQ_KLIM forces the s-step redo path.  The one knob read per solve, not through Tuning:
    // it is a test hook that tests/test_gpu_batch.py sets under a live context.
    const int klim = std::max(0, std::min(GQ_KMAX, (int)env_int("FOTO_GQ_KLIM", GQ_KMAX)));
    // the header to the host slot: stored by the CG kernel itself (FOTO_HOST_CRIT=0: a copy)
    P->hlast = P->hslot;
    P->hslot ^= 1;
    const bool direct = P->tn.host_crit;
    if (P->tn.gq_cgtab) {
        k_gq_cgtab<<<1 + GQ_TAB / 256, 256, 0, s>>>(P->gqn, rtol, maxiter, klim, P->gq,
                                                    direct ? P->dgq2[P->hlast] : nullptr, P->gq_pub, P->gq_bins,
                                                    P->gq_qcos, P->r * P->eps, P->c1, P->gq_tab);
        FOTO_HIP_CHECK(hipGetLastError());
    } else {
        k_gq_cg<<<1, GQ_CGNTH, 0, s>>>(P->gqn, rtol, maxiter, klim, P->gq, direct ? P->dgq2[P->hlast] : nullptr);
        FOTO_HIP_CHECK(hipGetLastError());
        k_gq_qtab<<<GQ_TAB / 256, 256, 0, s>>>(P->gq, P->gq_bins, P->gq_qcos, P->r * P->eps, P->c1, P->gq_tab);
        FOTO_HIP_CHECK(hipGetLastError());
    }
    if (kt) kt->stop(e, s, FOTO_K_SPEC, 0.0);
    if (!direct)
        FOTO_HIP_CHECK(hipMemcpyAsync(P->hgq2[P->hlast], P->gq, offsetof(GqState, alpha), hipMemcpyDeviceToHost, s));
    P->gauss_active = true;
    return 0;
}

// a failed solve broke the done chain (k_gq_cg); once it is redone, later solves may run again
static int gq_unbreak(SpecImpl* P, hipStream_t s) {
    FOTO_HIP_CHECK(hipMemsetAsync(&P->gq->broken, 0, sizeof(int), s));
    return 0;
}

// How the Gauss solve in header slot h ended, once the stream has passed its header store.
// !*ok (K beyond the table, or a breakdown): the solve is over and its done chain mended; the
// caller redoes it with the s-step CG from b^, which is still intact.  A good solve stays
// active -- its x^ comes from the table -- unless `end`: nothing of it is left to enqueue.
static int gq_outcome(SpecImpl* P, int h, int maxiter, bool end, int* ok, int* iters, int* info, hipStream_t s) {
    const GqState* H = P->hgq2[h];
    *ok = H->status == 0;
    *iters = H->K;
    *info = H->conv ? 0 : maxiter;
    if (!*ok || end) P->gauss_active = false;
    if (!*ok) FOTO_TRY(gq_unbreak(P, s));
    return 0;
}

// single shard: b (physical) -> b^ -> measure -> CG -> x, all enqueued.  b is only read: the
// transforms run through the box buffers (b -x-> tmp -y-> rh -t-> b^; x^ -> rh -t-> tmp -y-> rh
// -x-> x), so F survives a solve whose prox was skipped -- a failed solve with the next outer
// iteration already enqueued behind it (foto_bb.cpp) then finds its right-hand side intact.
static int gq_enqueue(SpecImpl* P, const double* b, double* x, double rtol, int maxiter, KTimer* kt, hipStream_t s) {
    FOTO_TRY(forward(P, b, P->rh, TC_PLAIN, rtol, maxiter, kt, s));
    FOTO_TRY(gq_measure(P, kt, s));
    FOTO_TRY(gq_solve(P, rtol, maxiter, kt, s));
    return inverse(P, XH_GAUSS, P->rh, P->tmp, P->rh, x, kt, s);
}

// the s-step CG from b^ (still intact) when the tables could not represent the solve
static int gq_redo(SpecImpl* P, double* b, double* x, double rtol, int maxiter, int* iters, int* info, KTimer* kt,
                   hipStream_t s) {
    FOTO_TRY(solve_s2(P, rtol, maxiter, iters, info, kt, s, false));
    return inverse_sstep(P, b, x, kt, s);
}

// ---------------------------------------------------------------------------- single shard

int SpectralPlan::solve(double* b, double* x, double rtol, int maxiter, int predicted, int* iters, int* info,
                        KTimer* kt, hipStream_t s) {
    SpecImpl* P = impl;
    if (P->gauss) {
        FOTO_TRY(gq_enqueue(P, b, x, rtol, maxiter, kt, s));
        FOTO_HIP_CHECK(hipStreamSynchronize(s));
        int ok = 0;
        FOTO_TRY(gq_outcome(P, P->hlast, maxiter, true, &ok, iters, info, s));
        return ok ? 0 : gq_redo(P, b, x, rtol, maxiter, iters, info, kt, s);
    }
    // b (physical) -> b^ (with the column kernels: and the INIT plan); b is scratch afterwards
    FOTO_TRY(forward(P, b, b, TC_PLAN, rtol, maxiter, kt, s));
    if (P->sstep == 2) FOTO_TRY(solve_s2(P, rtol, maxiter, iters, info, kt, s, P->tcol));
    else FOTO_TRY(solve_s1(P, rtol, maxiter, predicted, iters, info, kt, s));
    return inverse_sstep(P, b, x, kt, s);
}

bool SpectralPlan::deferrable() const {
    const SpecImpl* P = impl;
    if (P->gauss) return P->world == 1 && P->npend < 2;   // fixed work: nothing to predict
    return P->tcol && P->sstep == 2 && P->world == 1 && P->last_passes > 0 && P->npend == 0;
}

const int* SpectralPlan::done_flag() const { return impl->gauss ? &impl->gq->done : &impl->S2->done; }

int SpectralPlan::pending() const { return impl->npend; }

int SpectralPlan::solve_deferred(double* b, double* x, double rtol, int maxiter, KTimer* kt, hipStream_t s) {
    SpecImpl* P = impl;
    if (!deferrable()) {
        set_error("spectral CG: deferred solve needs a single-shard plan with a free slot (s-step: after a finished solve)");
        return FOTO_ERR_STATE;
    }
    SpecImpl::Pend& d = P->pq[P->npend];
    d.b = b;
    d.x = x;
    d.rtol = rtol;
    d.maxiter = maxiter;
    d.launched = 0;
    if (P->gauss) {
        FOTO_TRY(gq_enqueue(P, b, x, rtol, maxiter, kt, s));
        d.hslot = P->hlast;
        ++P->npend;
        return 0;
    }
    FOTO_TRY(forward(P, b, b, TC_PLAN, rtol, maxiter, kt, s));
    // the previous solve's pass count + margin (passes past the end exit at once);
    // FOTO_CG_MARGIN overrides the default 2 (tests force the redo path with a negative one)
    d.launched = std::max(1, P->last_passes + P->tn.cg_margin);
    FOTO_TRY(enqueue_passes(P, d.launched, [&] { return s2_launch(P, false, rtol, maxiter, kt, s); }, s));
    FOTO_TRY(inverse_sstep(P, b, x, kt, s));
    ++P->npend;
    return 0;
}

bool SpectralPlan::oldest_needs_redo() const {
    const SpecImpl* P = impl;
    if (P->npend == 0) return false;
    if (P->gauss) return P->hgq2[P->pq[0].hslot]->status != 0;
    return !P->hS2->done;
}

int SpectralPlan::drop_newest(hipStream_t s) {
    SpecImpl* P = impl;
    if (P->npend == 0 || !P->gauss) {
        set_error("spectral CG: no Gauss solve in flight to drop");
        return FOTO_ERR_STATE;
    }
    --P->npend;
    // the dropped solve may have failed or followed a failed one: its flags mean nothing now
    return gq_unbreak(P, s);
}

int SpectralPlan::finish(int* iters, int* info, int* redo, KTimer* kt, hipStream_t s) {
    SpecImpl* P = impl;
    if (P->npend == 0) {
        set_error("spectral CG: no deferred solve to finish");
        return FOTO_ERR_STATE;
    }
    if (P->npend > 1 && oldest_needs_redo()) {
        set_error("spectral CG: a failed solve must be redone before the next one runs (drop it first)");
        return FOTO_ERR_STATE;
    }
    const SpecImpl::Pend d = P->pq[0];
    P->pq[0] = P->pq[1];
    --P->npend;
    if (P->gauss) {
        int ok = 0;
        FOTO_TRY(gq_outcome(P, d.hslot, d.maxiter, P->npend == 0, &ok, iters, info, s));
        *redo = !ok;
        return ok ? 0 : gq_redo(P, d.b, d.x, d.rtol, d.maxiter, iters, info, kt, s);
    }
    // the predicted passes were not enough: continue, polling, and redo x
    *redo = !P->hS2->done;
    FOTO_TRY(pass_loop(P, d.launched, 1, d.maxiter, [&] { return s2_launch(P, false, d.rtol, d.maxiter, kt, s); },
                       iters, info, kt, s));
    if (*redo) FOTO_TRY(inverse_sstep(P, d.b, d.x, kt, s));
    return 0;
}

// ----------------------------------------------------------------------------- sharded phases
// Physical slab [tl][y][x] (planes t0..t0+nloc) <-> spectral box [kt][ky - y0][kx].

int SpectralPlan::fwd_local(double* b, int lo, int hi, KTimer* kt, hipStream_t s) {
    const Geo& g = impl->g;
    if (lo < 0 || hi > g.nloc || hi <= lo) {
        set_error("spectral CG: fwd_local planes [%d, %d) outside the slab", lo, hi);
        return FOTO_ERR_ARG;
    }
    const int64_t o = (int64_t)lo * g.nxy;
    Span sp(kt, s, FOTO_K_SLAB);
    FOTO_TRY(chain_fwd_xy(impl, sp, hi - lo, b + o, impl->tmpp + o, b + o));   // (b: the all-to-all's source)
    return sp.close();
}

int SpectralPlan::fwd_t(KTimer* kt, hipStream_t s) {
    Span sp(kt, s, FOTO_K_DCT);
    // box tmp -> b^; the column kernel also leaves this rank's INIT moments in gath (cg_begin then
    // launches nothing) unless the Gauss CG takes its own measure of b^
    FOTO_TRY(chain_fwd_t(impl, sp, impl->gauss ? TC_PLAIN : TC_GATH, impl->tmp, 0.0, 0));
    return sp.close();
}

int SpectralPlan::cg_begin(double rtol, int maxiter, KTimer* kt, hipStream_t s) {
    if (impl->tcol && !impl->gauss) return 0;   // the column kernel of fwd_t took the INIT moments
    return s2_launch(impl, true, rtol, maxiter, kt, s);
}

int SpectralPlan::cg_pass(double rtol, int maxiter, KTimer* kt, hipStream_t s) {
    return s2_launch(impl, false, rtol, maxiter, kt, s);
}

int SpectralPlan::cg_plan(int init, double rtol, int maxiter, hipStream_t s) {
    if (!init && impl->late_plan()) return 0;   // the next cg_pass plans at its start
    k_spec_s2_plan<<<1, 64, 0, s>>>(impl->S2, impl->gath, impl->world, init, rtol, maxiter);
    FOTO_HIP_CHECK(hipGetLastError());
    return 0;
}

int SpectralPlan::sstep_passes(const std::function<int()>& pass, int shards, int maxiter, int* iters, int* info,
                               KTimer* kt, hipStream_t s) {
    return pass_loop(impl, 0, shards, maxiter, pass, iters, info, kt, s);
}

int SpectralPlan::inv_t(KTimer* kt, hipStream_t s) {
    SpecImpl* P = impl;
    Span sp(kt, s, FOTO_K_DCT);
    // x^ through the box buffer that box_out() is not, the box of x~ to box_out()
    FOTO_TRY(chain_inv_t(P, sp, P->gauss_active ? XH_GAUSS : XH_SSTEP, P->tcol ? P->rh : P->tmp, box_out()));
    return sp.close();
}

int SpectralPlan::inv_local(double* scratch, double* x, int lo, int hi, KTimer* kt, hipStream_t s) {
    const Geo& g = impl->g;
    if (lo < -1 || hi > g.nloc + 1 || hi <= lo) {   // (one halo plane per side: phi's halo)
        set_error("spectral CG: inv_local planes [%d, %d) outside the slab and its halo", lo, hi);
        return FOTO_ERR_ARG;
    }
    const int64_t o = (int64_t)lo * g.nxy;
    Span sp(kt, s, FOTO_K_SLAB);
    // (scratch: the all-to-all's target)
    FOTO_TRY(chain_inv_yx(impl, sp, hi - lo, scratch + o, impl->tmpp + o, x + o));
    return sp.close();
}

bool SpectralPlan::gauss() const { return impl->gauss; }
int SpectralPlan::gauss_hist_size() { return GQ_HIST; }
double* SpectralPlan::gauss_hist() const { return impl->gq_hist; }

int SpectralPlan::gauss_measure(KTimer* kt, hipStream_t s) { return gq_measure(impl, kt, s); }

int SpectralPlan::gauss_solve(double rtol, int maxiter, KTimer* kt, hipStream_t s) {
    return gq_solve(impl, rtol, maxiter, kt, s);
}

int SpectralPlan::gauss_wait(int maxiter, int* ok, int* iters, int* info, hipStream_t s) {
    FOTO_HIP_CHECK(hipStreamSynchronize(s));
    return gq_outcome(impl, impl->hlast, maxiter, false, ok, iters, info, s);   // (ok: inv_t is still to come)
}

int SpectralPlan::gauss_result(int maxiter, int* ok, int* iters, int* info, hipStream_t s) {
    return gq_outcome(impl, impl->hlast, maxiter, true, ok, iters, info, s);
}

void SpectralPlan::gauss_end() { impl->gauss_active = false; }

int SpectralPlan::reset(hipStream_t s) {
    SpecImpl* P = impl;
    P->npend = 0;
    P->gauss_active = false;
    if (P->gq) FOTO_HIP_CHECK(hipMemsetAsync(P->gq, 0, sizeof(GqState), s));
    FOTO_TRY(gq_pub_clear(P, s));
    P->last_passes = 0;
    FOTO_HIP_CHECK(hipMemsetAsync(P->S, 0, sizeof(CGScal), s));
    FOTO_HIP_CHECK(hipMemsetAsync(P->rb.ticket, 0, 8 * sizeof(double), s));
    return reset_s2(P, s);
}

double* SpectralPlan::box_in() const { return impl->tmp; }
double* SpectralPlan::box_out() const { return impl->tcol ? impl->tmp : impl->rh; }
double* SpectralPlan::gath() const { return impl->gath; }
int SpectralPlan::moments() { return NACC; }
int SpectralPlan::y0() const { return impl->y0; }
int SpectralPlan::nyl() const { return impl->nyl; }

}  // namespace foto
