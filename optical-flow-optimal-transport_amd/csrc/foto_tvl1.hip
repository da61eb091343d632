// libfoto: duality-based TV-L1 flow with an illumination channel on gfx950 (Zach, Pock & Bischof
// 2007; the illumination term of Chambolle & Pock 2011).  include/foto.h has the algorithm.
//
// Coarse to fine on the GN pyramid's levels (its restriction, prolongation and export kernels, not
// copies of them); per level `warps` linearisations (k_tvl1_coeffs), each followed by `iters` inner
// iterations of pointwise thresholding plus a 3-point stencil.  No linear solve, no atomics, no
// reductions, no data-dependent stop: the launch sequence is a function of the options alone.
//
// Two launch structures, the same bits (the iteration's expressions exist once, below): several
// iterations per launch on LDS tiles (k_tvl1_tile, the default: per_launch = 5), or
// one launch per inner iteration (k_tvl1_iter, per_launch = 1).  The specification's iteration is "U from P, then
// P from the new U"; a launch runs the same sequence shifted by half a step, "P from U, then U from
// the new P", so that one thread needs no value another thread of the launch writes: it updates P
// at its own pixel and recomputes the two neighbouring P components its divergence reads (the
// x-component of the pixel to the left, the y-component of the pixel above) by the one expression
// tv_dual, so a value has the same bits wherever it is computed.  U and P are read from one buffer
// and written to a second one.  A level's first launch has no P step (P = 0 there) and a level's
// last P step is never needed (P is dropped); foto_tvl1_iterate, which returns P, ends with a
// launch that has the P step alone.
// The kernels are float64; the working set is cache-resident at the sizes people run (DESIGN.md
// 3.16 has the byte counts and the measurements of both structures).
#include <chrono>
#include <cmath>
#include <memory>
#include <vector>

#include "foto_devmem.h"
#include "foto_devutil.h"
#include "foto_gn.h"

namespace foto {

// ----------------------------------------------------------------------------- kernels

// One warp's coefficients at U0 = (u, v): g = S(f2; x + u, y + v), a1 = S(Gx f2; .), a2 =
// S(Gy f2; .), a3 = -gamma g, n2 = |a|^2, rc = g - f1 - a1 u - a2 v; co = [5][w h].  Gx, Gy are
// cdiff_x / cdiff_y of foto_devutil.h.  Three gathers through one sample_taps; every tap index is
// inside the frame whatever the displacement.
__global__ __launch_bounds__(NT) void k_tvl1_coeffs(int w, int h, double gamma, const double* __restrict__ f1,
                                                    const double* __restrict__ f2, const double* __restrict__ U,
                                                    double* __restrict__ co) {
    const int64_t n = (int64_t)w * h;
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int y = (int)((unsigned)i / (unsigned)w), x = (int)i - y * w;
    const double u = U[i], v = U[n + i];
    const SampleTaps T = sample_taps(w, h, (double)x + u, (double)y + v);
    const int i0 = T.i0, j0 = T.j0;
    const int64_t r0 = (int64_t)j0 * w, r1 = r0 + w;
    const double g = sample_sum(T, f2[r0 + i0], f2[r0 + i0 + 1], f2[r1 + i0], f2[r1 + i0 + 1]);
    const double a1 = sample_sum(T, cdiff_x(f2, w, i0, r0), cdiff_x(f2, w, i0 + 1, r0), cdiff_x(f2, w, i0, r1),
                                 cdiff_x(f2, w, i0 + 1, r1));
    const double a2 = sample_sum(T, cdiff_y(f2, w, h, i0, j0), cdiff_y(f2, w, h, i0 + 1, j0), cdiff_y(f2, w, h, i0, j0 + 1),
                                 cdiff_y(f2, w, h, i0 + 1, j0 + 1));
    const double a3 = -gamma * g;
    co[i] = a1;
    co[n + i] = a2;
    co[2 * n + i] = a3;
    co[3 * n + i] = (a1 * a1 + a2 * a2) + a3 * a3;
    co[4 * n + i] = ((g - f1[i]) - a1 * u) - a2 * v;
}

struct TvPar {
    double lt;      // lambda theta
    double theta;
    double tt;      // tau / theta
};

// The iteration's three expressions, the only copies: both launch structures below evaluate a value
// through them, so it has the same bits whichever computed it.
//   the dual step of one channel at a pixel with a right (hX) / lower (hY) neighbour: c, ux, uy =
//   U_d there, to the right and below; (p0, p1) = P_d:
//     (dx, dy) = fwd(U_d), den = 1 + tt sqrt(dx^2 + dy^2), P_d <- (P_d + tt (dx, dy)) / den
__device__ __forceinline__ void tv_dual_val(double c, double ux, double uy, bool hX, bool hY, double p0, double p1,
                                            double tt, double& ox, double& oy) {
    const double dx = hX ? ux - c : 0.0, dy = hY ? uy - c : 0.0;
    const double den = 1.0 + tt * sqrt(dx * dx + dy * dy);
    ox = (p0 + tt * dx) / den;
    oy = (p1 + tt * dy) / den;
}
//   the step length k from rho = ((rc + a1 u) + a2 v) + a3 w
__device__ __forceinline__ double tv_step_len(double rc, double n2, const double (&a)[3], double u, double v, double w,
                                              double lt) {
    const double rho = ((rc + a[0] * u) + a[1] * v) + a[2] * w;
    double k = n2 > 1e-12 ? -rho / n2 : 0.0;
    k = rho > lt * n2 ? -lt : k;
    k = rho < -lt * n2 ? lt : k;
    return k;
}
//   one axis of div(P): c = the component here, l = at the previous pixel of the axis
__device__ __forceinline__ double tv_div1(bool first, bool last, double c, double l) {
    return first ? c : (last ? -l : c - l);
}
//   the primal step of one channel
__device__ __forceinline__ double tv_primal_val(double u, double k, double a, double theta, double divx, double divy) {
    return (u + k * a) + theta * (divx + divy);
}

// P_d at pixel (x, y) after the dual step from U_d (DOP), or as it stands.  x in [0, w - 1], y in
// [0, h - 1]; the forward neighbours are loaded from clamped indices.
template <bool DOP>
__device__ __forceinline__ void tv_dual(const double* __restrict__ u, const double* __restrict__ px,
                                        const double* __restrict__ py, int w, int h, int x, int y, double tt,
                                        double& ox, double& oy) {
    const int64_t i = (int64_t)y * w + x;
    const double p0 = px[i], p1 = py[i];
    if (!DOP) {
        ox = p0;
        oy = p1;
        return;
    }
    const bool hX = x < w - 1, hY = y < h - 1;
    tv_dual_val(u[i], u[hX ? i + 1 : i], u[hY ? i + w : i], hX, hY, p0, p1, tt, ox, oy);
}

// One launch of the inner iteration on a w x h level: the dual step (DOP), then the primal step
// (DOU) with the thresholding of rho.  U = [3][w h], P = [6][w h] = (px, py) of u, v, w.  Ui / Pi
// are read, Uo / Po written (Uo unused without DOU, Po without DOP).
template <bool DOP, bool DOU>
__global__ __launch_bounds__(NT) void k_tvl1_iter(int w, int h, int tiles_x, TvPar par, const double* __restrict__ co,
                                                  const double* __restrict__ Ui, double* __restrict__ Uo,
                                                  const double* __restrict__ Pi, double* __restrict__ Po) {
    const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)blockIdx.x - ty * tiles_x;
    const int x = tx * TX + (threadIdx.x & (TX - 1)), y = ty * TY + (threadIdx.x / TX);
    if (x >= w || y >= h) return;
    const int64_t n = (int64_t)w * h, i = (int64_t)y * w + x;
    double k = 0.0, a[3];
    if (DOU) {
        a[0] = co[i]; a[1] = co[n + i]; a[2] = co[2 * n + i];
        k = tv_step_len(co[4 * n + i], co[3 * n + i], a, Ui[i], Ui[n + i], Ui[2 * n + i], par.lt);
    }
    const int xm = max(x - 1, 0), ym = max(y - 1, 0);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double* u = Ui + d * n;
        const double *px = Pi + 2 * d * n, *py = px + n;
        double cx, cy;
        tv_dual<DOP>(u, px, py, w, h, x, y, par.tt, cx, cy);
        if (DOP) {
            Po[2 * d * n + i] = cx;
            Po[(2 * d + 1) * n + i] = cy;
        }
        if (DOU) {
            double lx, ly, t;
            tv_dual<DOP>(u, px, py, w, h, xm, y, par.tt, lx, t);   // px of the pixel to the left
            tv_dual<DOP>(u, px, py, w, h, x, ym, par.tt, t, ly);   // py of the pixel above
            const double divx = tv_div1(x == 0, x == w - 1, cx, lx), divy = tv_div1(y == 0, y == h - 1, cy, ly);
            Uo[d * n + i] = tv_primal_val(u[i], k, a[d], par.theta, divx, divy);
        }
    }
}

// K inner iterations in one launch, on LDS.  A block loads the TR_W x TR_H region around its
// (TR_W - 2K) x (TR_H - 2K) tile -- U and P, nine fields, 72 B a pixel, 54 KiB -- and runs the
// launch-per-iteration sequence on it, "P from U" then "U from the new P", a barrier after each,
// every region pixel inside the frame in every round; each thread keeps the coefficients of its
// three pixels in registers.  A value K - j rings inside the region is exact after round j (a
// round's dependence reaches one pixel in every direction, and at a frame edge the boundary rule
// reads nothing beyond it); the rim's values are computed from region-clamped neighbours, finite,
// wrong and never stored.  After K rounds the tile's pixels are stored: U_{i+K} and the P of the
// last round, what K launches of k_tvl1_iter leave.  first_p = 0: the first round has no P step (a
// level's first launch).  Tiles partition the frame, so no value is stored twice.
constexpr int TR_W = 32, TR_H = 24, TR_N = TR_W * TR_H, TR_PER = TR_N / NT;
constexpr int TV_KMAX = 8;   // TR_H - 2 K >= 8
static_assert(TR_N % NT == 0 && TR_H - 2 * TV_KMAX > 0, "the tile region");

__global__ __launch_bounds__(NT) void k_tvl1_tile(int w, int h, int tiles_x, int K, int first_p, TvPar par,
                                                  const double* __restrict__ co, const double* __restrict__ Ui,
                                                  double* __restrict__ Uo, const double* __restrict__ Pi,
                                                  double* __restrict__ Po) {
    __shared__ double sU[3][TR_N], sP[6][TR_N];
    const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)blockIdx.x - ty * tiles_x;
    const int ox = tx * (TR_W - 2 * K) - K, oy = ty * (TR_H - 2 * K) - K;   // the region's origin in the frame
    const int64_t n = (int64_t)w * h;
    int li[TR_PER], gx[TR_PER], gy[TR_PER];
    bool in[TR_PER];
    double a[TR_PER][3], n2[TR_PER], rc[TR_PER];
#pragma unroll
    for (int q = 0; q < TR_PER; ++q) {
        li[q] = threadIdx.x + q * NT;
        gx[q] = ox + (li[q] & (TR_W - 1));
        gy[q] = oy + li[q] / TR_W;
        in[q] = gx[q] >= 0 && gx[q] < w && gy[q] >= 0 && gy[q] < h;
        const int64_t i = in[q] ? (int64_t)gy[q] * w + gx[q] : 0;   // (a pixel outside the frame loads pixel 0 and keeps zeros)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            a[q][d] = co[d * n + i];
            const double u = Ui[d * n + i];
            sU[d][li[q]] = in[q] ? u : 0.0;
        }
        n2[q] = co[3 * n + i];
        rc[q] = co[4 * n + i];
#pragma unroll
        for (int d = 0; d < 6; ++d) {
            const double p = Pi[d * n + i];
            sP[d][li[q]] = in[q] ? p : 0.0;
        }
    }
    __syncthreads();
    for (int j = 0; j < K; ++j) {
        if (j > 0 || first_p) {
#pragma unroll
            for (int q = 0; q < TR_PER; ++q) {
                if (!in[q]) continue;
                const int l = li[q], lx = l & (TR_W - 1), ly = l / TR_W;
                const int r = lx < TR_W - 1 ? l + 1 : l, b = ly < TR_H - 1 ? l + TR_W : l;   // clamped to the region
                const bool hX = gx[q] < w - 1, hY = gy[q] < h - 1;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    double px, py;
                    tv_dual_val(sU[d][l], sU[d][r], sU[d][b], hX, hY, sP[2 * d][l], sP[2 * d + 1][l], par.tt, px, py);
                    sP[2 * d][l] = px;
                    sP[2 * d + 1][l] = py;
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < TR_PER; ++q) {
            if (!in[q]) continue;
            const int l = li[q], lx = l & (TR_W - 1), ly = l / TR_W;
            const int lf = lx > 0 ? l - 1 : l, up = ly > 0 ? l - TR_W : l;
            const double k = tv_step_len(rc[q], n2[q], a[q], sU[0][l], sU[1][l], sU[2][l], par.lt);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double divx = tv_div1(gx[q] == 0, gx[q] == w - 1, sP[2 * d][l], sP[2 * d][lf]);
                const double divy = tv_div1(gy[q] == 0, gy[q] == h - 1, sP[2 * d + 1][l], sP[2 * d + 1][up]);
                sU[d][l] = tv_primal_val(sU[d][l], k, a[q][d], par.theta, divx, divy);
            }
        }
        __syncthreads();
    }
    const bool wrote_p = first_p || K > 1;
#pragma unroll
    for (int q = 0; q < TR_PER; ++q) {
        const int lx = li[q] & (TR_W - 1), ly = li[q] / TR_W;
        if (!in[q] || lx < K || lx >= TR_W - K || ly < K || ly >= TR_H - K) continue;
        const int64_t i = (int64_t)gy[q] * w + gx[q];
#pragma unroll
        for (int d = 0; d < 3; ++d) Uo[d * n + i] = sU[d][li[q]];
        if (wrote_p)
#pragma unroll
            for (int d = 0; d < 6; ++d) Po[d * n + i] = sP[d][li[q]];
    }
}

// m = gamma w, the reported luminosity
__global__ __launch_bounds__(NT) void k_tvl1_lum(int64_t n, double gamma, const double* __restrict__ wch,
                                                 double* __restrict__ m) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i < n) m[i] = gamma * wch[i];
}

static hipError_t launch_tvl1_coeffs(int w, int h, double gamma, const double* f1, const double* f2, const double* U,
                                     double* co, hipStream_t s) {
    k_tvl1_coeffs<<<flat_blocks((int64_t)w * h), NT, 0, s>>>(w, h, gamma, f1, f2, U, co);
    return hipGetLastError();
}

// The ping-pong state of a level's iteration: U[cu] and P[cp] hold the current values.
struct TvState {
    double* U[2];
    double* P[2];
    int cu = 0, cp = 0;
};

enum TvStep { TV_PRIMAL, TV_BOTH, TV_DUAL };

static hipError_t launch_tvl1_iter(int w, int h, const TvPar& par, const double* co, TvState& S, TvStep step,
                                   hipStream_t s) {
    // (a flat grid of tiles, row by row: w h < 2^31 keeps the count far below the grid limit)
    const int tiles_x = (w + TX - 1) / TX;
    const unsigned grid = (unsigned)tiles_x * (unsigned)((h + TY - 1) / TY);
    const double *Ui = S.U[S.cu], *Pi = S.P[S.cp];
    double *Uo = S.U[1 - S.cu], *Po = S.P[1 - S.cp];
    if (step == TV_PRIMAL) k_tvl1_iter<false, true><<<grid, NT, 0, s>>>(w, h, tiles_x, par, co, Ui, Uo, Pi, nullptr);
    else if (step == TV_BOTH) k_tvl1_iter<true, true><<<grid, NT, 0, s>>>(w, h, tiles_x, par, co, Ui, Uo, Pi, Po);
    else k_tvl1_iter<true, false><<<grid, NT, 0, s>>>(w, h, tiles_x, par, co, Ui, nullptr, Pi, Po);
    if (step != TV_DUAL) S.cu = 1 - S.cu;
    if (step != TV_PRIMAL) S.cp = 1 - S.cp;
    return hipGetLastError();
}

static hipError_t launch_tvl1_tile(int w, int h, const TvPar& par, const double* co, TvState& S, int K, bool first_p,
                                   hipStream_t s) {
    const int iw = TR_W - 2 * K, ih = TR_H - 2 * K;
    const int tiles_x = (w + iw - 1) / iw;
    const unsigned grid = (unsigned)tiles_x * (unsigned)((h + ih - 1) / ih);
    k_tvl1_tile<<<grid, NT, 0, s>>>(w, h, tiles_x, K, first_p ? 1 : 0, par, co, S.U[S.cu], S.U[1 - S.cu], S.P[S.cp],
                                    S.P[1 - S.cp]);
    S.cu = 1 - S.cu;
    if (first_p || K > 1) S.cp = 1 - S.cp;
    return hipGetLastError();
}

// `count` inner iterations on one set of coefficients, at most per_launch of them in a launch
// (1: k_tvl1_iter, one launch each); first_p: the first of them has its P step.
static int tvl1_run(int w, int h, const TvPar& par, const double* co, TvState& S, int count, int per_launch,
                    bool first_p, hipStream_t s, int* launches) {
    for (int done = 0; done < count; ++*launches) {
        const bool fp = first_p || done > 0;
        if (per_launch == 1) {
            FOTO_HIP_CHECK(launch_tvl1_iter(w, h, par, co, S, fp ? TV_BOTH : TV_PRIMAL, s));
            ++done;
        } else {
            const int k = std::min(per_launch, count - done);
            FOTO_HIP_CHECK(launch_tvl1_tile(w, h, par, co, S, k, fp, s));
            done += k;
        }
    }
    return 0;
}

static int tvl1_per_launch_check(int per_launch, const char* who) {
    if (per_launch < 1 || per_launch > FOTO_TVL1_MAX_PER_LAUNCH) {
        set_error("%s: per_launch = %d: 1 .. %d iterations per launch", who, per_launch, FOTO_TVL1_MAX_PER_LAUNCH);
        return FOTO_ERR_ARG;
    }
    return 0;
}
static_assert(FOTO_TVL1_MAX_PER_LAUNCH == TV_KMAX, "include/foto.h and the tile kernel");

// ----------------------------------------------------------------------------- option rules (host)

static int tvl1_par_check(double lambda, double theta, double tau, const char* who) {
    if (!(theta > 0) || !(tau > 0) || !std::isfinite(theta) || !std::isfinite(tau)) {
        set_error("%s: theta = %g, tau = %g: both must be positive and finite", who, theta, tau);
        return FOTO_ERR_ARG;
    }
    if (!std::isfinite(lambda) || lambda < 0) {
        set_error("%s: lambda = %g: the data weight must be finite and >= 0", who, lambda);
        return FOTO_ERR_ARG;
    }
    return 0;
}

static int tvl1_opts_check(const foto_tvl1_opts& o) {
    FOTO_TRY(tvl1_par_check(o.lambda, o.theta, o.tau, "foto_tvl1_create"));
    if (!std::isfinite(o.gamma) || o.gamma < 0) {
        set_error("foto_tvl1_create: gamma = %g: the illumination coupling must be finite and >= 0", o.gamma);
        return FOTO_ERR_ARG;
    }
    if (o.warps < 1 || o.iters < 1) {
        set_error("foto_tvl1_create: warps = %d, iters = %d: both counts must be >= 1", o.warps, o.iters);
        return FOTO_ERR_ARG;
    }
    return tvl1_per_launch_check(o.per_launch, "foto_tvl1_create");
}

}  // namespace foto

using namespace foto;

// ============================================================================ the plan (host)

struct foto_tvl1 {
    int w = 0, h = 0, device = 0;
    foto_tvl1_opts o{};
    std::vector<int> wl, hl;             // level sizes, finest first
    hipStream_t s = nullptr;             // everything between ingest and export runs here
    DevArena mem;
    std::vector<double*> f1, f2;         // the frames per level
    TvState S;                           // sized for level 0; a level uses the front of each buffer
    double* co = nullptr;                // [5][w h]; after the last level its front holds m
    std::vector<hipEvent_t> lev_ev;      // start, then the end of each level (coarsest first)
    StreamLink link;

    ~foto_tvl1() {
        if (s) (void)hipStreamSynchronize(s);
        for (auto e : lev_ev) if (e) (void)hipEventDestroy(e);
        mem.clear();
        stream_release(s);
    }
};

namespace foto {

struct TvDev {
    const foto_image* f1;
    const foto_image* f2;
    void* out;
    int dtype, layout;
    hipStream_t user;
};

static int tvl1_solve(foto_tvl1* T, const double* h1, const double* h2, double* u, double* v, double* m,
                      const TvDev* dv, foto_tvl1_stats* st) {
    const auto wall0 = std::chrono::steady_clock::now();
    hipStream_t s = T->s;
    const foto_tvl1_opts& o = T->o;
    const int L = (int)T->wl.size();
    const size_t n0 = (size_t)T->w * T->h;
    const TvPar par{o.lambda * o.theta, o.theta, o.tau / o.theta};
    TvState& S = T->S;
    std::vector<int> launches(L, 0);
    if (dv) FOTO_TRY(T->link.enter(dv->user, s));   // (before the first read of a frame)
    FOTO_HIP_CHECK(hipEventRecord(T->lev_ev[0], s));
    if (dv) {
        FOTO_HIP_CHECK(launch_ingest(*dv->f1, T->w, T->h, T->f1[0], s));
        FOTO_HIP_CHECK(launch_ingest(*dv->f2, T->w, T->h, T->f2[0], s));
    } else {
        FOTO_HIP_CHECK(hipMemcpyAsync(T->f1[0], h1, n0 * sizeof(double), hipMemcpyHostToDevice, s));
        FOTO_HIP_CHECK(hipMemcpyAsync(T->f2[0], h2, n0 * sizeof(double), hipMemcpyHostToDevice, s));
    }
    for (int l = 0; l + 1 < L; ++l)
        FOTO_HIP_CHECK(launch_pyr_down(T->wl[l], T->hl[l], T->f1[l], T->f2[l], T->f1[l + 1], T->f2[l + 1], s));
    for (int l = L - 1; l >= 0; --l) {
        const int w = T->wl[l], h = T->hl[l];
        const size_t n = (size_t)w * h;
        if (l == L - 1) {
            FOTO_HIP_CHECK(hipMemsetAsync(S.U[S.cu], 0, 3 * n * sizeof(double), s));
        } else {   // the coarser level's (u, v, w), prolonged into the other buffer
            FOTO_HIP_CHECK(launch_pyr_up(T->wl[l + 1], T->hl[l + 1], w, h, S.U[S.cu], S.U[1 - S.cu], s));
            S.cu = 1 - S.cu;
            ++launches[l];
        }
        FOTO_HIP_CHECK(hipMemsetAsync(S.P[S.cp], 0, 6 * n * sizeof(double), s));
        for (int k = 0; k < o.warps; ++k) {
            FOTO_HIP_CHECK(launch_tvl1_coeffs(w, h, o.gamma, T->f1[l], T->f2[l], S.U[S.cu], T->co, s));
            ++launches[l];
            FOTO_TRY(tvl1_run(w, h, par, T->co, S, o.iters, o.per_launch, k > 0, s, &launches[l]));
        }
        FOTO_HIP_CHECK(hipEventRecord(T->lev_ev[L - l], s));
    }
    const double* U = S.U[S.cu];
    k_tvl1_lum<<<flat_blocks((int64_t)n0), NT, 0, s>>>((int64_t)n0, o.gamma, U + 2 * n0, T->co);
    FOTO_HIP_CHECK(hipGetLastError());
    if (dv) {
        FOTO_HIP_CHECK(launch_export((int64_t)n0, U, U + n0, T->co, dv->out, dv->dtype, dv->layout, s));
        FOTO_TRY(T->link.leave(s, dv->user));
    } else {
        FOTO_HIP_CHECK(hipMemcpyAsync(u, U, n0 * sizeof(double), hipMemcpyDeviceToHost, s));
        FOTO_HIP_CHECK(hipMemcpyAsync(v, U + n0, n0 * sizeof(double), hipMemcpyDeviceToHost, s));
        FOTO_HIP_CHECK(hipMemcpyAsync(m, T->co, n0 * sizeof(double), hipMemcpyDeviceToHost, s));
        FOTO_HIP_CHECK(hipStreamSynchronize(s));
    }
    if (st) {
        st->levels = L;
        st->launches_total = 0;
        FOTO_HIP_CHECK(hipEventSynchronize(T->lev_ev[L]));
        for (int l = 0; l < L; ++l) {
            st->launches_total += launches[l];
            if (l >= st->cap) continue;
            if (st->wl) st->wl[l] = T->wl[l];
            if (st->hl) st->hl[l] = T->hl[l];
            if (st->launches) st->launches[l] = launches[l];
            if (st->ms_level) {
                float t = 0.f;
                FOTO_HIP_CHECK(hipEventElapsedTime(&t, T->lev_ev[L - 1 - l], T->lev_ev[L - l]));
                st->ms_level[l] = t;
            }
        }
        st->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    return 0;
}

}  // namespace foto

extern "C" {

int foto_tvl1_opts_default(foto_tvl1_opts* o) {
    if (!o) { set_error("foto_tvl1_opts_default: null argument"); return FOTO_ERR_ARG; }
    o->lambda = 38.0;
    o->theta = 0.3;
    o->tau = 0.25;
    o->gamma = 0.1;
    o->levels = 4;
    o->warps = 5;
    o->iters = 30;
    o->min_size = 16;
    o->per_launch = 5;   // (measured: DESIGN.md 3.16)
    return 0;
}

int foto_tvl1_create(int w, int h, const foto_tvl1_opts* opts, foto_tvl1** out) {
    if (!out) { set_error("foto_tvl1_create: null argument"); return FOTO_ERR_ARG; }
    auto T = std::make_unique<foto_tvl1>();
    (void)foto_tvl1_opts_default(&T->o);
    if (opts) T->o = *opts;
    int wl[FOTO_GN_PYR_MAX_LEVELS], hl[FOTO_GN_PYR_MAX_LEVELS], L = 0;
    FOTO_TRY(foto_gn_pyr_sizes(w, h, T->o.levels, T->o.min_size, wl, hl, FOTO_GN_PYR_MAX_LEVELS, &L));
    FOTO_TRY(tvl1_opts_check(T->o));
    T->w = w; T->h = h;
    T->wl.assign(wl, wl + L);
    T->hl.assign(hl, hl + L);
    FOTO_HIP_CHECK(hipGetDevice(&T->device));
    FOTO_TRY(stream_acquire(&T->s));
    const size_t n0 = (size_t)w * h;
    size_t frames = 0;
    for (int l = 0; l < L; ++l) frames += 2 * (size_t)wl[l] * hl[l];
    double* q = nullptr;   // one block: the level frames, U twice, P twice, the coefficients
    FOTO_TRY(T->mem.alloc_n(frames + (2 * 3 + 2 * 6 + 5) * n0, &q));
    for (int l = 0; l < L; ++l) {
        const size_t n = (size_t)wl[l] * hl[l];
        T->f1.push_back(q); q += n;
        T->f2.push_back(q); q += n;
    }
    for (int b = 0; b < 2; ++b) { T->S.U[b] = q; q += 3 * n0; }
    for (int b = 0; b < 2; ++b) { T->S.P[b] = q; q += 6 * n0; }
    T->co = q;
    T->lev_ev.assign(L + 1, nullptr);
    for (auto& e : T->lev_ev) FOTO_HIP_CHECK(hipEventCreate(&e));
    *out = T.release();
    return 0;
}

void foto_tvl1_destroy(foto_tvl1* p) { delete p; }

int foto_tvl1_device(const foto_tvl1* p) { return p ? p->device : -1; }

int foto_tvl1_solve(foto_tvl1* p, const double* f1, const double* f2, double* u, double* v, double* m,
                    foto_tvl1_stats* stats) {
    if (!p || !f1 || !f2 || !u || !v || !m) { set_error("foto_tvl1_solve: null argument"); return FOTO_ERR_ARG; }
    return tvl1_solve(p, f1, f2, u, v, m, nullptr, stats);
}

int foto_tvl1_solve_dev(foto_tvl1* p, const foto_image* f1, const foto_image* f2, void* out, int dtype, int layout,
                        void* stream, foto_tvl1_stats* stats) {
    if (!p || !f1 || !f2) { set_error("foto_tvl1_solve_dev: null argument"); return FOTO_ERR_ARG; }
    // device memory of the plan's device, checked before anything is enqueued
    FOTO_TRY(image_dev_check(f1, p->w, p->h, p->device, "foto_tvl1_solve_dev (f1)"));
    FOTO_TRY(image_dev_check(f2, p->w, p->h, p->device, "foto_tvl1_solve_dev (f2)"));
    FOTO_TRY(export_check(out, dtype, layout, (int64_t)p->w * p->h, p->device, "foto_tvl1_solve_dev"));
    const TvDev dv{f1, f2, out, dtype, layout, (hipStream_t)stream};
    return tvl1_solve(p, nullptr, nullptr, nullptr, nullptr, nullptr, &dv, stats);
}

// ----------------------------------------------------------------------------- test entries

int foto_tvl1_coeffs(const double* f1, const double* f2, const double* u, const double* v, int w, int h,
                     double gamma, double* out5) {
    if (!f1 || !f2 || !u || !v || !out5) { set_error("foto_tvl1_coeffs: null argument"); return FOTO_ERR_ARG; }
    FOTO_TRY(image_size_check(w, h, 2, "foto_tvl1_coeffs"));
    CallScope S;
    FOTO_TRY(S.init());
    const size_t n = (size_t)w * h;
    double *d1, *d2, *U, *co;
    FOTO_TRY(S.up(f1, n, &d1));
    FOTO_TRY(S.up(f2, n, &d2));
    FOTO_TRY(S.dev(2 * n, &U));
    FOTO_TRY(S.dev(5 * n, &co));
    FOTO_TRY(S.up_to(u, n, U));
    FOTO_TRY(S.up_to(v, n, U + n));
    FOTO_HIP_CHECK(launch_tvl1_coeffs(w, h, gamma, d1, d2, U, co, S.s));
    FOTO_TRY(S.down(out5, co, 5 * n));
    return S.sync();
}

int foto_tvl1_iterate(const double* coef5, double* U3, double* P6, int w, int h, double lambda, double theta,
                      double tau, int n_iters, int per_launch) {
    if (!coef5 || !U3 || !P6) { set_error("foto_tvl1_iterate: null argument"); return FOTO_ERR_ARG; }
    FOTO_TRY(image_size_check(w, h, 2, "foto_tvl1_iterate"));
    FOTO_TRY(tvl1_par_check(lambda, theta, tau, "foto_tvl1_iterate"));
    if (n_iters < 1) { set_error("foto_tvl1_iterate: n = %d: the count must be >= 1", n_iters); return FOTO_ERR_ARG; }
    FOTO_TRY(tvl1_per_launch_check(per_launch, "foto_tvl1_iterate"));
    CallScope C;
    FOTO_TRY(C.init());
    const size_t n = (size_t)w * h;
    double* co;
    TvState S;
    FOTO_TRY(C.up(coef5, 5 * n, &co));
    FOTO_TRY(C.up(U3, 3 * n, &S.U[0]));
    FOTO_TRY(C.up(P6, 6 * n, &S.P[0]));
    FOTO_TRY(C.dev(3 * n, &S.U[1]));
    FOTO_TRY(C.dev(6 * n, &S.P[1]));
    const TvPar par{lambda * theta, theta, tau / theta};
    // U P U P ... U P as a first launch without its P step, the rest with both, and a last launch
    // that has the P step alone
    int launches = 0;
    FOTO_TRY(tvl1_run(w, h, par, co, S, n_iters, per_launch, false, C.s, &launches));
    FOTO_HIP_CHECK(launch_tvl1_iter(w, h, par, co, S, TV_DUAL, C.s));
    FOTO_TRY(C.down(U3, S.U[S.cu], 3 * n));
    FOTO_TRY(C.down(P6, S.P[S.cp], 6 * n));
    return C.sync();
}

}  // extern "C"
