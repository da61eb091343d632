// libfoto: coarse-to-fine Gennert-Negahdaripour flow with warping on gfx950.
//
// The GN brightness equation is a linearisation (good for about a pixel).  The pyramid restricts
// both frames, solves on the coarsest level, and from there to level 0 repeats: prolong the flow,
// warp the second frame by it, solve for the increment with the prior's smoothness term in the
// right-hand side (the TOTAL flow is regularised), add the increment (include/foto.h and DESIGN.md
// have the algorithm).  Every solve is a foto_gn_plan's, one plan per level, all on one stream.
// The kernels here are float64, one thread per pixel, memory-bound gathers; no LDS.
#include <chrono>
#include <cmath>
#include <memory>
#include <vector>

#include "foto_devmem.h"
#include "foto_devutil.h"
#include "foto_gn.h"

namespace foto {

// ----------------------------------------------------------------------------- kernels

// (S(f; x, y), the clamped bilinear sample of the prolongation and the warp: pyr_sample, foto_devutil.h)

// Restriction of both frames of a level, one thread per coarse pixel.  A lane reads the two
// neighbouring doubles of each of its two rows, so a wave's loads cover one contiguous 1 KB span
// per row and every fetched line is used whole; the stores are contiguous.  The summation order is
// fixed: the result is tested for equal bits.
__global__ __launch_bounds__(NT) void k_pyr_down(int w, int h, int wc, int hc, const double* __restrict__ f1,
                                                 const double* __restrict__ f2, double* __restrict__ c1,
                                                 double* __restrict__ c2) {
    const int64_t I = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (I >= (int64_t)wc * hc) return;
    const int j = (int)((unsigned)I / (unsigned)wc), i = (int)I - j * wc;
    const int I0 = 2 * i, I1 = min(2 * i + 1, w - 1), J0 = 2 * j, J1 = min(2 * j + 1, h - 1);
    const int64_t a = (int64_t)J0 * w, b = (int64_t)J1 * w;
    c1[I] = 0.25 * (((f1[a + I0] + f1[a + I1]) + f1[b + I0]) + f1[b + I1]);
    c2[I] = 0.25 * (((f2[a + I0] + f2[a + I1]) + f2[b + I0]) + f2[b + I1]);
}

// Prolongation of u, v, m ([3][wc hc] -> [3][w h]) with the displacement scales, one thread per
// fine pixel
__global__ __launch_bounds__(NT) void k_pyr_up(int wc, int hc, int w, int h, const double* __restrict__ c,
                                               double* __restrict__ o) {
    const int64_t n = (int64_t)w * h, nc = (int64_t)wc * hc;
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int y = (int)((unsigned)i / (unsigned)w), x = (int)i - y * w;
    const double sx = ((double)x + 0.5) * (double)wc / (double)w - 0.5;
    const double sy = ((double)y + 0.5) * (double)hc / (double)h - 0.5;
    o[i] = ((double)w / (double)wc) * pyr_sample(c, wc, hc, sx, sy);
    o[n + i] = ((double)h / (double)hc) * pyr_sample(c + nc, wc, hc, sx, sy);
    o[2 * n + i] = pyr_sample(c + 2 * nc, wc, hc, sx, sy);
}

// g = (1 - m) S(f2; x + u, y + v), one thread per pixel; p = the prior [3][w h]
__global__ __launch_bounds__(NT) void k_pyr_warp(int w, int h, const double* __restrict__ f2,
                                                 const double* __restrict__ p, double* __restrict__ g) {
    const int64_t n = (int64_t)w * h;
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int y = (int)((unsigned)i / (unsigned)w), x = (int)i - y * w;
    g[i] = (1.0 - p[2 * n + i]) * pyr_sample(f2, w, h, (double)x + p[i], (double)y + p[n + i]);
}

// b -= [alpha N u0; alpha N v0; lambda N m0]: the Laplacian part of the operator's rows (gn_lap_row
// with the bare diagonal coef * c) on the prior
__global__ __launch_bounds__(NT) void k_gn_rhs_prior(int w, int h, double a, double l, const double* __restrict__ x0,
                                                     double* __restrict__ b) {
    const int64_t n = (int64_t)w * h;
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const GNPix P = gn_pix(w, h, i);
    double xv[3][5];
    gn_gather5(P, w, i, [&](int f, int64_t j) { return x0[f * n + j]; }, xv);
    const double coef[3] = {a, a, l};
#pragma unroll
    for (int f = 0; f < 3; ++f)
        b[f * n + i] -= gn_lap_row(P, coef[f], coef[f] * P.c, [&](int k) { return xv[f][k]; }, 0.0);
}

__global__ __launch_bounds__(NT) void k_gn_add(int64_t n, double* __restrict__ x, const double* __restrict__ x0) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i < n) x[i] = x[i] + x0[i];
}

hipError_t launch_gn_rhs_prior(int w, int h, double alpha, double lam, const double* x0, double* b, hipStream_t s) {
    k_gn_rhs_prior<<<flat_blocks((int64_t)w * h), NT, 0, s>>>(w, h, alpha, lam, x0, b);
    return hipGetLastError();
}

hipError_t launch_gn_add(int64_t n, double* x, const double* x0, hipStream_t s) {
    k_gn_add<<<flat_blocks(n), NT, 0, s>>>(n, x, x0);
    return hipGetLastError();
}

hipError_t launch_pyr_down(int w, int h, const double* f1, const double* f2, double* c1, double* c2, hipStream_t s) {
    const int wc = (w + 1) / 2, hc = (h + 1) / 2;
    k_pyr_down<<<flat_blocks((int64_t)wc * hc), NT, 0, s>>>(w, h, wc, hc, f1, f2, c1, c2);
    return hipGetLastError();
}

hipError_t launch_pyr_up(int wc, int hc, int w, int h, const double* c, double* o, hipStream_t s) {
    k_pyr_up<<<flat_blocks((int64_t)w * h), NT, 0, s>>>(wc, hc, w, h, c, o);
    return hipGetLastError();
}

static hipError_t launch_pyr_warp(int w, int h, const double* f2, const double* p, double* g, hipStream_t s) {
    k_pyr_warp<<<flat_blocks((int64_t)w * h), NT, 0, s>>>(w, h, f2, p, g);
    return hipGetLastError();
}

// ----------------------------------------------------------------------------- level sizes (host)

static int pyr_sizes(int w, int h, int levels, int min_size, std::vector<int>& wl, std::vector<int>& hl,
                     const char* who) {
    FOTO_TRY(image_size_check(w, h, 2, who));
    if (levels < 1) { set_error("levels = %d: the pyramid needs >= 1 level", levels); return FOTO_ERR_ARG; }
    if (min_size < 2) { set_error("min_size = %d: a level needs >= 2 pixels per axis", min_size); return FOTO_ERR_ARG; }
    wl.assign(1, w);
    hl.assign(1, h);
    while ((int)wl.size() < levels && (int)wl.size() < FOTO_GN_PYR_MAX_LEVELS &&
           std::min(wl.back(), hl.back()) >= 2 * (int64_t)min_size) {
        wl.push_back((wl.back() + 1) / 2);
        hl.push_back((hl.back() + 1) / 2);
    }
    return 0;
}

}  // namespace foto

using namespace foto;

// ============================================================================ the pyramid (host)

struct foto_gn_pyr {
    int w = 0, h = 0, device = 0, warps = 1;
    std::vector<int> wl, hl;             // level sizes, finest first
    hipStream_t s = nullptr;             // everything between ingest and export runs here
    std::vector<foto_gn_plan*> plan;     // one per level (each keeps its own iteration prediction)
    double* base = nullptr;
    std::vector<double*> f2;             // the second frame per level (a level's d2 holds its warp)
    double* pr = nullptr;                // the prior of the running solve, [3][w_l h_l]
    std::vector<hipEvent_t> lev_ev;      // start, then the end of each level (coarsest first)
    std::vector<hipEvent_t> own_ev;      // pairs around the pyramid's own kernels (stats only)
    StreamLink link;

    ~foto_gn_pyr() {
        if (s) (void)hipStreamSynchronize(s);
        for (auto* p : plan) foto_gn_plan_destroy(p);
        for (auto e : lev_ev) if (e) (void)hipEventDestroy(e);
        for (auto e : own_ev) if (e) (void)hipEventDestroy(e);
        if (base) (void)hipFree(base);
        stream_release(s);
    }
};

namespace foto {

struct PyrDev {
    const foto_image* f1;
    const foto_image* f2;
    void* out;
    int dtype, layout;
    hipStream_t user;
};

static int pyr_solve(foto_gn_pyr* P, const double* h1, const double* h2, double* u, double* v, double* m,
                     const PyrDev* dv, foto_gn_pyr_stats* st) {
    const auto wall0 = std::chrono::steady_clock::now();
    hipStream_t s = P->s;
    const int L = (int)P->wl.size();
    const size_t n0 = (size_t)P->w * P->h;
    // pairs of events around the pyramid's own kernels, only when a report is asked for
    size_t own_used = 0;
    auto tick = [&]() -> int {
        if (!st) return 0;
        if (own_used == P->own_ev.size()) {
            hipEvent_t e = nullptr;
            FOTO_HIP_CHECK(hipEventCreate(&e));
            P->own_ev.push_back(e);
        }
        FOTO_HIP_CHECK(hipEventRecord(P->own_ev[own_used++], s));
        return 0;
    };
    if (dv) FOTO_TRY(P->link.enter(dv->user, s));   // (before the first read of a frame)
    FOTO_HIP_CHECK(hipEventRecord(P->lev_ev[0], s));
    {
        const GnBufs B0 = gn_plan_bufs(P->plan[0]);
        if (dv) {
            FOTO_HIP_CHECK(launch_ingest(*dv->f1, P->w, P->h, B0.d1, s));
            FOTO_HIP_CHECK(launch_ingest(*dv->f2, P->w, P->h, P->f2[0], s));
        } else {
            FOTO_HIP_CHECK(hipMemcpyAsync(B0.d1, h1, n0 * sizeof(double), hipMemcpyHostToDevice, s));
            FOTO_HIP_CHECK(hipMemcpyAsync(P->f2[0], h2, n0 * sizeof(double), hipMemcpyHostToDevice, s));
        }
    }
    FOTO_TRY(tick());
    for (int l = 0; l + 1 < L; ++l)
        FOTO_HIP_CHECK(launch_pyr_down(P->wl[l], P->hl[l], gn_plan_bufs(P->plan[l]).d1, P->f2[l],
                                       gn_plan_bufs(P->plan[l + 1]).d1, P->f2[l + 1], s));
    FOTO_TRY(tick());
    int nsolve = 0, nfail = 0;
    for (int l = L - 1; l >= 0; --l) {
        const int w = P->wl[l], h = P->hl[l];
        const size_t n = (size_t)w * h;
        const GnBufs B = gn_plan_bufs(P->plan[l]);
        for (int k = 0; k < P->warps; ++k, ++nsolve) {
            const bool first = l == L - 1 && k == 0;   // no prior: today's plan solve
            FOTO_TRY(tick());
            if (first) {
                FOTO_HIP_CHECK(hipMemcpyAsync(B.d2, P->f2[l], n * sizeof(double), hipMemcpyDeviceToDevice, s));
            } else {
                if (k == 0)   // the level below's flow, prolonged
                    FOTO_HIP_CHECK(launch_pyr_up(P->wl[l + 1], P->hl[l + 1], w, h, gn_plan_bufs(P->plan[l + 1]).x,
                                                 P->pr, s));
                else          // this level's flow so far (gn_setup zeroes x)
                    FOTO_HIP_CHECK(hipMemcpyAsync(P->pr, B.x, 3 * n * sizeof(double), hipMemcpyDeviceToDevice, s));
                FOTO_HIP_CHECK(launch_pyr_warp(w, h, P->f2[l], P->pr, B.d2, s));
            }
            FOTO_TRY(tick());
            int its = 0;
            bool done = false;
            FOTO_TRY(gn_plan_solve_prior(P->plan[l], first ? nullptr : P->pr, &its, &done));
            if (!done) ++nfail;
            if (st && nsolve < st->cap) {
                if (st->its) st->its[nsolve] = its;
                if (st->info) st->info[nsolve] = done ? 0 : its;
            }
        }
        FOTO_HIP_CHECK(hipEventRecord(P->lev_ev[L - l], s));
    }
    const GnBufs B0 = gn_plan_bufs(P->plan[0]);
    if (dv) {
        FOTO_HIP_CHECK(launch_export((int64_t)n0, B0.x, B0.x + n0, B0.x + 2 * n0, dv->out, dv->dtype, dv->layout, s));
        FOTO_TRY(P->link.leave(s, dv->user));
    } else {
        double* const outs[3] = {u, v, m};
        for (int c = 0; c < 3; ++c)
            FOTO_HIP_CHECK(hipMemcpyAsync(outs[c], B0.x + c * n0, n0 * sizeof(double), hipMemcpyDeviceToHost, s));
        FOTO_HIP_CHECK(hipStreamSynchronize(s));
    }
    if (st) {
        st->levels = L;
        st->solves = nsolve;
        FOTO_HIP_CHECK(hipEventSynchronize(P->lev_ev[L]));
        for (int l = 0; l < FOTO_GN_PYR_MAX_LEVELS; ++l) {
            st->wl[l] = l < L ? P->wl[l] : 0;
            st->hl[l] = l < L ? P->hl[l] : 0;
            st->ms_level[l] = 0.0;
        }
        for (int l = L - 1; l >= 0; --l) {
            float t = 0.f;
            FOTO_HIP_CHECK(hipEventElapsedTime(&t, P->lev_ev[L - 1 - l], P->lev_ev[L - l]));
            st->ms_level[l] = t;
        }
        st->ms_new = 0.0;
        for (size_t e = 0; e + 1 < own_used; e += 2) {
            float t = 0.f;
            FOTO_HIP_CHECK(hipEventElapsedTime(&t, P->own_ev[e], P->own_ev[e + 1]));
            st->ms_new += t;
        }
        st->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    return nfail;
}

static int pyr_opts_check(const foto_gn_pyr_opts& o) {
    if (o.warps < 1) { set_error("warps = %d: the pyramid needs >= 1 solve per level", o.warps); return FOTO_ERR_ARG; }
    if (o.maxiter < 0) { set_error("maxiter < 0"); return FOTO_ERR_ARG; }
    return 0;
}

}  // namespace foto

extern "C" {

int foto_gn_pyr_sizes(int w, int h, int levels, int min_size, int* wl, int* hl, int cap, int* n) {
    if (!wl || !hl || !n) { set_error("foto_gn_pyr_sizes: null argument"); return FOTO_ERR_ARG; }
    std::vector<int> a, b;
    FOTO_TRY(pyr_sizes(w, h, levels, min_size, a, b, "foto_gn_pyr_sizes"));
    if (cap < (int)a.size()) { set_error("foto_gn_pyr_sizes: cap = %d for %d levels", cap, (int)a.size()); return FOTO_ERR_ARG; }
    for (size_t l = 0; l < a.size(); ++l) { wl[l] = a[l]; hl[l] = b[l]; }
    *n = (int)a.size();
    return 0;
}

int foto_gn_pyr_opts_default(foto_gn_pyr_opts* o) {
    if (!o) { set_error("foto_gn_pyr_opts_default: null argument"); return FOTO_ERR_ARG; }
    o->levels = 4;
    o->warps = 3;
    o->min_size = 16;
    o->rtol = 1e-10;
    o->maxiter = 200000;
    return 0;
}

int foto_gn_pyr_create(int w, int h, double alpha, double lambda_, const foto_gn_pyr_opts* opts, foto_gn_pyr** out) {
    if (!out) { set_error("foto_gn_pyr_create: null argument"); return FOTO_ERR_ARG; }
    foto_gn_pyr_opts o;
    (void)foto_gn_pyr_opts_default(&o);
    if (opts) o = *opts;
    auto P = std::make_unique<foto_gn_pyr>();
    FOTO_TRY(pyr_sizes(w, h, o.levels, o.min_size, P->wl, P->hl, "foto_gn_pyr_create"));
    FOTO_TRY(pyr_opts_check(o));
    if (!(alpha > 0) || !(lambda_ > 0)) {
        set_error("GN needs alpha > 0 and lambda > 0 (the block-Jacobi smoother divides by them)");
        return FOTO_ERR_ARG;
    }
    P->w = w; P->h = h; P->warps = o.warps;
    const int L = (int)P->wl.size();
    FOTO_HIP_CHECK(hipGetDevice(&P->device));
    FOTO_TRY(stream_acquire(&P->s));
    size_t total = 3 * (size_t)w * h;
    for (int l = 0; l < L; ++l) total += (size_t)P->wl[l] * P->hl[l];
    FOTO_HIP_CHECK(hipMalloc((void**)&P->base, total * sizeof(double)));
    double* q = P->base;
    P->pr = q; q += 3 * (size_t)w * h;
    for (int l = 0; l < L; ++l) { P->f2.push_back(q); q += (size_t)P->wl[l] * P->hl[l]; }
    for (int l = 0; l < L; ++l) {
        foto_gn_plan* pl = nullptr;
        FOTO_TRY(gn_plan_make(P->wl[l], P->hl[l], alpha, lambda_, o.rtol, o.maxiter, P->s, &pl));
        P->plan.push_back(pl);
    }
    P->lev_ev.assign(L + 1, nullptr);
    for (auto& e : P->lev_ev) FOTO_HIP_CHECK(hipEventCreate(&e));
    *out = P.release();
    return 0;
}

void foto_gn_pyr_destroy(foto_gn_pyr* p) { delete p; }

int foto_gn_pyr_device(const foto_gn_pyr* p) { return p ? p->device : -1; }

int foto_gn_pyr_solve(foto_gn_pyr* p, const double* f1, const double* f2, double* u, double* v, double* m,
                      foto_gn_pyr_stats* stats) {
    if (!p || !f1 || !f2 || !u || !v || !m) { set_error("foto_gn_pyr_solve: null argument"); return FOTO_ERR_ARG; }
    return pyr_solve(p, f1, f2, u, v, m, nullptr, stats);
}

int foto_gn_pyr_solve_dev(foto_gn_pyr* p, const foto_image* f1, const foto_image* f2, void* out, int dtype,
                          int layout, void* stream, foto_gn_pyr_stats* stats) {
    if (!p || !f1 || !f2) { set_error("foto_gn_pyr_solve_dev: null argument"); return FOTO_ERR_ARG; }
    // device memory of the pyramid's device, checked before anything is enqueued
    FOTO_TRY(image_dev_check(f1, p->w, p->h, p->device, "foto_gn_pyr_solve_dev (f1)"));
    FOTO_TRY(image_dev_check(f2, p->w, p->h, p->device, "foto_gn_pyr_solve_dev (f2)"));
    FOTO_TRY(export_check(out, dtype, layout, (int64_t)p->w * p->h, p->device, "foto_gn_pyr_solve_dev"));
    const PyrDev dv{f1, f2, out, dtype, layout, (hipStream_t)stream};
    return pyr_solve(p, nullptr, nullptr, nullptr, nullptr, nullptr, &dv, stats);
}

// ----------------------------------------------------------------------------- test entries

int foto_pyr_down(const double* f1, const double* f2, int w, int h, double* c1, double* c2) {
    if (!f1 || !f2 || !c1 || !c2) { set_error("foto_pyr_down: null argument"); return FOTO_ERR_ARG; }
    FOTO_TRY(image_size_check(w, h, 1, "foto_pyr_down"));
    CallScope S;
    FOTO_TRY(S.init());
    const size_t n = (size_t)w * h, nc = (size_t)((w + 1) / 2) * ((h + 1) / 2);
    double *d1, *d2, *o1, *o2;
    FOTO_TRY(S.dev(n, &d1));
    FOTO_TRY(S.dev(n, &d2));
    FOTO_TRY(S.dev(nc, &o1));
    FOTO_TRY(S.dev(nc, &o2));
    FOTO_TRY(S.up_to(f1, n, d1));
    FOTO_TRY(S.up_to(f2, n, d2));
    FOTO_HIP_CHECK(launch_pyr_down(w, h, d1, d2, o1, o2, S.s));
    FOTO_TRY(S.down(c1, o1, nc));
    FOTO_TRY(S.down(c2, o2, nc));
    return S.sync();
}

int foto_pyr_up(const double* u, const double* v, const double* m, int wc, int hc, int w, int h, double* uo,
                double* vo, double* mo) {
    if (!u || !v || !m || !uo || !vo || !mo) { set_error("foto_pyr_up: null argument"); return FOTO_ERR_ARG; }
    FOTO_TRY(image_size_check(wc, hc, 2, "foto_pyr_up (coarse)"));
    FOTO_TRY(image_size_check(w, h, 2, "foto_pyr_up (fine)"));
    CallScope S;
    FOTO_TRY(S.init());
    const size_t n = (size_t)w * h, nc = (size_t)wc * hc;
    double *c, *o;
    FOTO_TRY(S.dev(3 * nc, &c));
    FOTO_TRY(S.dev(3 * n, &o));
    const double* const in[3] = {u, v, m};
    double* const outs[3] = {uo, vo, mo};
    for (int f = 0; f < 3; ++f) FOTO_TRY(S.up_to(in[f], nc, c + f * nc));
    FOTO_HIP_CHECK(launch_pyr_up(wc, hc, w, h, c, o, S.s));
    for (int f = 0; f < 3; ++f) FOTO_TRY(S.down(outs[f], o + f * n, n));
    return S.sync();
}

int foto_gn_warp_prior(const double* f2, const double* u, const double* v, const double* m, int w, int h, double* g) {
    if (!f2 || !u || !v || !m || !g) { set_error("foto_gn_warp_prior: null argument"); return FOTO_ERR_ARG; }
    FOTO_TRY(image_size_check(w, h, 2, "foto_gn_warp_prior"));
    CallScope S;
    FOTO_TRY(S.init());
    const size_t n = (size_t)w * h;
    double *d2, *p, *o;
    FOTO_TRY(S.dev(n, &d2));
    FOTO_TRY(S.dev(3 * n, &p));
    FOTO_TRY(S.dev(n, &o));
    FOTO_TRY(S.up_to(f2, n, d2));
    const double* const in[3] = {u, v, m};
    for (int f = 0; f < 3; ++f) FOTO_TRY(S.up_to(in[f], n, p + f * n));
    FOTO_HIP_CHECK(launch_pyr_warp(w, h, d2, p, o, S.s));
    FOTO_TRY(S.down(g, o, n));
    return S.sync();
}

int foto_gn_solve_prior(const double* f1, const double* g, int w, int h, double alpha, double lambda_, double rtol,
                        int maxiter, const double* u0, const double* v0, const double* m0, double* u, double* v,
                        double* m, int* iterations) {
    if (!f1 || !g || !u || !v || !m) { set_error("foto_gn_solve_prior: null argument"); return FOTO_ERR_ARG; }
    const bool prior = u0 || v0 || m0;
    if (prior && (!u0 || !v0 || !m0)) { set_error("foto_gn_solve_prior: a prior needs u0, v0 and m0"); return FOTO_ERR_ARG; }
    // (the prior's block is declared before the plan's owner, so it is freed after it: destroying
    // the plan drains the plan's stream first, and the solve on it may still read the prior)
    DevArena mem;
    double* x0 = nullptr;
    foto_gn_plan* pl = nullptr;
    FOTO_TRY(foto_gn_plan_create(w, h, alpha, lambda_, rtol, maxiter, &pl));
    const std::unique_ptr<foto_gn_plan, void (*)(foto_gn_plan*)> owner(pl, foto_gn_plan_destroy);
    const GnBufs B = gn_plan_bufs(pl);
    const size_t n = (size_t)w * h;
    FOTO_HIP_CHECK(hipMemcpyAsync(B.d1, f1, n * sizeof(double), hipMemcpyHostToDevice, B.s));
    FOTO_HIP_CHECK(hipMemcpyAsync(B.d2, g, n * sizeof(double), hipMemcpyHostToDevice, B.s));
    if (prior) {
        FOTO_TRY(mem.alloc_n(3 * n, &x0));
        const double* const in[3] = {u0, v0, m0};
        for (int f = 0; f < 3; ++f)
            FOTO_HIP_CHECK(hipMemcpyAsync(x0 + f * n, in[f], n * sizeof(double), hipMemcpyHostToDevice, B.s));
    }
    int its = 0;
    bool done = false;
    FOTO_TRY(gn_plan_solve_prior(pl, x0, &its, &done));
    double* const outs[3] = {u, v, m};
    for (int f = 0; f < 3; ++f)
        FOTO_HIP_CHECK(hipMemcpyAsync(outs[f], B.x + f * n, n * sizeof(double), hipMemcpyDeviceToHost, B.s));
    FOTO_HIP_CHECK(hipStreamSynchronize(B.s));
    if (iterations) *iterations = its;
    return done ? 0 : maxiter;
}

}  // extern "C"
