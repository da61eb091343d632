// libfoto C ABI: per-operator entry points (operators.py matvecs, stepB, RHS, flow
// extraction) and the GN solver (classical.GLLOpticalFlow.process).  Every call copies
// the caller's host buffers to the current device, runs the kernels on a private stream
// and copies the result back; device scratch lives only for the call.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>

#include "foto_devmem.h"
#include "foto_internal.h"

using namespace foto;

namespace {

Geo make_geo(int Nt, int Nx, int Ny) {
    Geo g;
    g.Nt = Nt; g.Ny = Ny; g.Nx = Nx; g.t0 = 0; g.nloc = Nt; g.nxy = (int64_t)Nx * Ny;
    return g;
}

int bc_flag(char bc, int* bcD) {
    if (bc == 'N' || bc == 'n') { *bcD = 0; return 0; }
    if (bc == 'D' || bc == 'd') { *bcD = 1; return 0; }
    set_error("These boundary conditions are not implemented");   // operators.py:6-7
    return FOTO_ERR_BC;
}

}  // namespace

extern "C" {

int foto_grad_st(const double* phi, int Nt, int Nx, int Ny, double* out3) {
    FOTO_TRY(grid_size_check(Nt, Nx, Ny, "foto_grad_st"));
    CallScope S;
    FOTO_TRY(S.init());
    const Geo g = make_geo(Nt, Nx, Ny);
    const size_t N = (size_t)Nt * g.nxy;
    double *d, *o;
    FOTO_TRY(S.up(phi, N, &d));
    FOTO_TRY(S.dev(3 * N, &o));
    FOTO_HIP_CHECK(launch_grad_st(g, d, o, o + N, o + 2 * N, S.s));
    FOTO_TRY(S.down(out3, o, 3 * N));
    return S.sync();
}

int foto_div_st(const double* w3, int Nt, int Nx, int Ny, double* out) {
    FOTO_TRY(grid_size_check(Nt, Nx, Ny, "foto_div_st"));
    CallScope S;
    FOTO_TRY(S.init());
    const Geo g = make_geo(Nt, Nx, Ny);
    const size_t N = (size_t)Nt * g.nxy;
    double *d, *o;
    FOTO_TRY(S.up(w3, 3 * N, &d));
    FOTO_TRY(S.dev(N, &o));
    FOTO_HIP_CHECK(launch_div_st(g, d, d + N, d + 2 * N, o, S.s));
    FOTO_TRY(S.down(out, o, N));
    return S.sync();
}

static int apply_common(const double* p, int Nt, int Nx, int Ny, double r, double eps, int lap, double* out) {
    FOTO_TRY(grid_size_check(Nt, Nx, Ny, lap ? "foto_laplacian_st" : "foto_apply_A"));
    CallScope S;
    FOTO_TRY(S.init());
    const Geo g = make_geo(Nt, Nx, Ny);
    const size_t N = (size_t)Nt * g.nxy;
    double *d, *o;
    FOTO_TRY(S.up(p, N, &d));
    FOTO_TRY(S.dev(N, &o));
    FOTO_HIP_CHECK(launch_apply_A(g, d, o, r, eps, lap, S.s));
    FOTO_TRY(S.down(out, o, N));
    return S.sync();
}

int foto_laplacian_st(const double* p, int Nt, int Nx, int Ny, double* out) {
    return apply_common(p, Nt, Nx, Ny, 1.0, 0.0, 1, out);
}

int foto_apply_A(const double* p, int Nt, int Nx, int Ny, double r, double eps, double* out) {
    return apply_common(p, Nt, Nx, Ny, r, eps, 0, out);
}

int foto_grad2(const double* f, int Nx, int Ny, char bc, double* out2) {
    int bcD;
    FOTO_TRY(bc_flag(bc, &bcD));
    FOTO_TRY(image_size_check(Nx, Ny, 2, "foto_grad2"));
    CallScope S;
    FOTO_TRY(S.init());
    const size_t n = (size_t)Nx * Ny;
    double *d, *o;
    FOTO_TRY(S.up(f, n, &d));
    FOTO_TRY(S.dev(2 * n, &o));
    FOTO_HIP_CHECK(launch_grad2(Nx, Ny, d, o, o + n, bcD, S.s));
    FOTO_TRY(S.down(out2, o, 2 * n));
    return S.sync();
}

int foto_div2(const double* uv, int Nx, int Ny, char bc, double* out) {
    int bcD;
    FOTO_TRY(bc_flag(bc, &bcD));
    FOTO_TRY(image_size_check(Nx, Ny, 2, "foto_div2"));
    CallScope S;
    FOTO_TRY(S.init());
    const size_t n = (size_t)Nx * Ny;
    double *d, *o;
    FOTO_TRY(S.up(uv, 2 * n, &d));
    FOTO_TRY(S.dev(n, &o));
    FOTO_HIP_CHECK(launch_div2(Nx, Ny, d, d + n, o, bcD, 1.0, S.s));
    FOTO_TRY(S.down(out, o, n));
    return S.sync();
}

int foto_grad2_forward(const double* f, int Nx, int Ny, double* out2) {
    FOTO_TRY(image_size_check(Nx, Ny, 2, "foto_grad2_forward"));
    CallScope S;
    FOTO_TRY(S.init());
    const size_t n = (size_t)Nx * Ny;
    double *d, *o;
    FOTO_TRY(S.up(f, n, &d));
    FOTO_TRY(S.dev(2 * n, &o));
    FOTO_HIP_CHECK(launch_grad2_forward(Nx, Ny, d, o, o + n, S.s));
    FOTO_TRY(S.down(out2, o, 2 * n));
    return S.sync();
}

int foto_stepB(const double* p3, int64_t M, double* q3) {
    if (M < 0 || !p3 || !q3) { set_error("bad stepB arguments"); return FOTO_ERR_ARG; }
    if (M == 0) return 0;
    CallScope S;
    FOTO_TRY(S.init());
    double *d, *o;
    FOTO_TRY(S.up(p3, 3 * (size_t)M, &d));
    FOTO_TRY(S.dev(3 * (size_t)M, &o));
    FOTO_HIP_CHECK(launch_stepB(M, d, d + M, d + 2 * M, o, o + M, o + 2 * M, S.s));
    FOTO_TRY(S.down(q3, o, 3 * (size_t)M));
    return S.sync();
}

int foto_bb_rhs(const double* mu3, const double* q3, const double* rho0, const double* rhoT, int Nt, int Nx, int Ny,
                double r, double* F) {
    FOTO_TRY(grid_size_check(Nt, Nx, Ny, "foto_bb_rhs"));
    CallScope S;
    FOTO_TRY(S.init());
    const Geo g = make_geo(Nt, Nx, Ny);
    const size_t N = (size_t)Nt * g.nxy;
    double *mu, *q, *r0, *rT, *o, *part, *gath;
    FOTO_TRY(S.up(mu3, 3 * N, &mu));
    FOTO_TRY(S.up(q3, 3 * N, &q));
    FOTO_TRY(S.up(rho0, g.nxy, &r0));
    FOTO_TRY(S.up(rhoT, g.nxy, &rT));
    FOTO_TRY(S.dev(N, &o));
    const int nb = flat_blocks((int64_t)N);
    FOTO_TRY(S.dev(nb + 8, &part));
    FOTO_TRY(S.dev(8, &gath));
    FOTO_HIP_CHECK(hipMemsetAsync(part + nb, 0, 8 * sizeof(double), S.s));
    RedBuf rb{part, (unsigned*)(part + nb), nb};
    FOTO_HIP_CHECK(launch_rhs(g, mu, mu + N, mu + 2 * N, q, q + N, q + 2 * N, r0, rT, r, o, rb, gath, 0, S.s));
    FOTO_TRY(S.down(F, o, N));
    return S.sync();
}

int foto_flow_from_phi(const double* phi, int Nt, int Nx, int Ny, double* u, double* v, double* m) {
    FOTO_TRY(grid_size_check(Nt, Nx, Ny, "foto_flow_from_phi"));
    CallScope S;
    FOTO_TRY(S.init());
    const Geo g = make_geo(Nt, Nx, Ny);
    const size_t N = (size_t)Nt * g.nxy, n = (size_t)g.nxy;
    double *d, *px, *py, *du, *dv, *dm;
    FOTO_TRY(S.up(phi, N, &d));
    FOTO_TRY(S.dev(n, &px));
    FOTO_TRY(S.dev(n, &py));
    FOTO_TRY(S.dev(n, &du));
    FOTO_TRY(S.dev(n, &dv));
    FOTO_TRY(S.dev(n, &dm));
    FOTO_HIP_CHECK(launch_traj(g, d, 0, Nt - 1, px, py, 1, S.s));
    FOTO_HIP_CHECK(launch_flow_record(Nx, Ny, px, py, du, dv, dm, FOTO_F64, 0, S.s));
    FOTO_TRY(S.down(u, du, n));
    FOTO_TRY(S.down(v, dv, n));
    FOTO_TRY(S.down(m, dm, n));
    return S.sync();
}

int foto_flow_path_from_phi(const double* phi, int Nt, int Nx, int Ny, double* u, double* v, double* m) {
    FOTO_TRY(grid_size_check(Nt, Nx, Ny, "foto_flow_path_from_phi"));
    if (!phi || !u || !v || !m) { set_error("foto_flow_path_from_phi: null pointer"); return FOTO_ERR_ARG; }
    CallScope S;
    FOTO_TRY(S.init());
    const Geo g = make_geo(Nt, Nx, Ny);
    const size_t N = (size_t)Nt * g.nxy, n = (size_t)g.nxy, R = (size_t)(Nt - 1) * n;
    double *d, *px, *py, *du, *dv, *dm;
    FOTO_TRY(S.up(phi, N, &d));
    FOTO_TRY(S.dev(n, &px));
    FOTO_TRY(S.dev(n, &py));
    FOTO_TRY(S.dev(R, &du));
    FOTO_TRY(S.dev(R, &dv));
    FOTO_TRY(S.dev(R, &dm));
    for (int k = 0; k + 1 < Nt; ++k) {   // the two launches per step of foto_bb_flow_path
        FOTO_HIP_CHECK(launch_traj(g, d, k, k + 1, px, py, k == 0, S.s));
        FOTO_HIP_CHECK(launch_flow_record(Nx, Ny, px, py, du + k * n, dv + k * n, dm + k * n, FOTO_F64, 0, S.s));
    }
    FOTO_TRY(S.down(u, du, R));
    FOTO_TRY(S.down(v, dv, R));
    FOTO_TRY(S.down(m, dm, R));
    return S.sync();
}

int foto_track_from_phi(const double* phi, int Nt, int Nx, int Ny, const double* pts, int64_t M, int all_steps,
                        double* out) {
    const char* who = "foto_track_from_phi";
    FOTO_TRY(grid_size_check(Nt, Nx, Ny, who));
    if (!phi) { set_error("%s: null pointer", who); return FOTO_ERR_ARG; }
    FOTO_TRY(track_arg_check(pts, out, M, all_steps, who));
    CallScope S;
    FOTO_TRY(S.init());
    const Geo g = make_geo(Nt, Nx, Ny);
    const size_t N = (size_t)Nt * g.nxy, np = 2 * (size_t)M, nr = np * (size_t)(all_steps ? Nt - 1 : 1);
    double *d, *dp, *dout;
    FOTO_TRY(S.up(phi, N, &d));
    FOTO_TRY(S.up(pts, np, &dp));
    FOTO_TRY(S.dev(nr, &dout));
    FOTO_HIP_CHECK(launch_track(g, d, 0, Nt - 1, dp, FOTO_F64, nullptr, nullptr, dout, FOTO_F64, M, all_steps, S.s));
    FOTO_TRY(S.down(out, dout, nr));
    return S.sync();
}

// the plane table of a contiguous phi[Nt][Ny][Nx] at d, in call scratch
static int one_buffer_table(CallScope& S, const double* d, int Nt, int64_t nxy, const double* const** table) {
    double* t = nullptr;   // (Nt pointers in Nt doubles' room)
    static_assert(sizeof(double*) == sizeof(double), "a plane pointer per double");
    FOTO_TRY(S.dev((size_t)Nt, &t));
    PlaneSegs sg;
    sg.n = 1;
    sg.base[0] = d; sg.t0[0] = 0; sg.nloc[0] = Nt;
    FOTO_HIP_CHECK(launch_plane_table(sg, nxy, (const double**)t, S.s));
    *table = (const double* const*)t;
    return 0;
}

int foto_maps_from_phi(const double* phi, int Nt, int Nx, int Ny, const double* s, int count, int inv_iters,
                       double* out) {
    const char* who = "foto_maps_from_phi";
    FOTO_TRY(grid_size_check(Nt, Nx, Ny, who));
    if (!phi) { set_error("%s: null pointer", who); return FOTO_ERR_ARG; }
    FOTO_TRY(maps_arg_check(s, out, count, inv_iters, Nt, who));
    CallScope S;
    FOTO_TRY(S.init());
    const int64_t nxy = (int64_t)Nx * Ny;
    const size_t rec = 4 * (size_t)nxy;
    double *d, *dout;
    FOTO_TRY(S.up(phi, (size_t)Nt * nxy, &d));
    FOTO_TRY(S.dev((size_t)count * rec, &dout));
    const double* const* table = nullptr;
    FOTO_TRY(one_buffer_table(S, d, Nt, nxy, &table));
    for (int k0 = 0; k0 < count; k0 += MAPS_MAX)
        FOTO_HIP_CHECK(launch_maps(table, Nt, Nx, Ny, s + k0, std::min(MAPS_MAX, count - k0), inv_iters,
                                   dout + (size_t)k0 * rec, FOTO_F64, S.s));
    FOTO_TRY(S.down(out, dout, (size_t)count * rec));
    return S.sync();
}

int foto_interp_from_phi(const double* phi, int Nt, int Nx, int Ny, const double* f0, const double* f1, int channels,
                         const double* s, int count, int inv_iters, double* out) {
    const char* who = "foto_interp_from_phi";
    FOTO_TRY(grid_size_check(Nt, Nx, Ny, who));
    if (!phi || !f0 || !f1) { set_error("%s: null pointer", who); return FOTO_ERR_ARG; }
    if (channels < 1) { set_error("%s: channels = %d must be >= 1", who, channels); return FOTO_ERR_ARG; }
    FOTO_TRY(maps_arg_check(s, out, count, inv_iters, Nt, who));
    CallScope S;
    FOTO_TRY(S.init());
    const int64_t nxy = (int64_t)Nx * Ny;
    const size_t img = (size_t)nxy * (size_t)channels;
    double *d, *d0, *d1, *dout;
    FOTO_TRY(S.up(phi, (size_t)Nt * nxy, &d));
    FOTO_TRY(S.up(f0, img, &d0));
    FOTO_TRY(S.up(f1, img, &d1));
    FOTO_TRY(S.dev((size_t)count * img, &dout));
    const double* const* table = nullptr;
    FOTO_TRY(one_buffer_table(S, d, Nt, nxy, &table));
    const foto_image i0{d0, FOTO_F64, (int64_t)Nx * channels, channels, 1.0};   // interleaved HWC
    const foto_image i1{d1, FOTO_F64, (int64_t)Nx * channels, channels, 1.0};
    for (int k0 = 0; k0 < count; k0 += MAPS_MAX)
        FOTO_HIP_CHECK(launch_interp(table, Nt, Nx, Ny, i0, 1, i1, 1, channels, s + k0, std::min(MAPS_MAX, count - k0),
                                     inv_iters, dout + (size_t)k0 * img, FOTO_F64, S.s));
    FOTO_TRY(S.down(out, dout, (size_t)count * img));
    return S.sync();
}

int foto_report_from_state(const double* mu3, const double* phi, const double* rho0, const double* rhoT, int Nt,
                           int Nx, int Ny, double* out) {
    const char* who = "foto_report_from_state";
    if (!mu3 || !phi || !rho0 || !rhoT || !out) { set_error("%s: null pointer", who); return FOTO_ERR_ARG; }
    FOTO_TRY(grid_size_check(Nt, Nx, Ny, who, 1));   // (the report's sums run on a one-voxel-wide plane too)
    CallScope S;
    FOTO_TRY(S.init());
    const Geo g = make_geo(Nt, Nx, Ny);
    const size_t N = (size_t)Nt * g.nxy, ntab = (size_t)Nt * FOTO_REPORT_COLS;
    const size_t npart = ntab * (size_t)report_pieces(g.nxy);
    double *mu, *ph, *r0, *rT, *scr;
    FOTO_TRY(S.up(mu3, 3 * N, &mu));
    FOTO_TRY(S.up(phi, N, &ph));
    FOTO_TRY(S.up(rho0, g.nxy, &r0));
    FOTO_TRY(S.up(rhoT, g.nxy, &rT));
    FOTO_TRY(S.dev(ntab + npart + (size_t)Nt, &scr));   // table | partials | tickets (one double's room each)
    unsigned* ticket = (unsigned*)(scr + ntab + npart);
    FOTO_HIP_CHECK(hipMemsetAsync(ticket, 0, (size_t)Nt * sizeof(unsigned), S.s));
    ReportIn in{};
    in.rho = mu; in.m1 = mu + N; in.m2 = mu + 2 * N; in.phi = ph;
    in.rho0 = r0; in.rhoT = rT;
    FOTO_HIP_CHECK(launch_report(g, in, scr + ntab, ticket, scr, S.s));
    FOTO_TRY(S.down(out, scr, ntab));
    return S.sync();
}

// ----------------------------------------------------------------------------- GN

int foto_gn_apply(const double* f1, const double* f2, int w, int h, double alpha, double lam, const double* x3,
                  double* y3) {
    FOTO_TRY(image_size_check(w, h, 2, "foto_gn_apply"));
    CallScope S;
    FOTO_TRY(S.init());
    const size_t n = (size_t)w * h;
    double *d1, *d2, *fx, *fy, *ft, *x, *y;
    FOTO_TRY(S.up(f1, n, &d1));
    FOTO_TRY(S.up(f2, n, &d2));
    FOTO_TRY(S.up(x3, 3 * n, &x));
    FOTO_TRY(S.dev(n, &fx));
    FOTO_TRY(S.dev(n, &fy));
    FOTO_TRY(S.dev(n, &ft));
    FOTO_TRY(S.dev(3 * n, &y));
    FOTO_HIP_CHECK(launch_gn_coeffs(w, h, d1, d2, fx, fy, ft, S.s));
    FOTO_HIP_CHECK(launch_gn_apply(w, h, fx, fy, d2, alpha, lam, x, y, S.s));
    FOTO_TRY(S.down(y3, y, 3 * n));
    return S.sync();
}

int foto_gn_rhs(const double* f1, const double* f2, int w, int h, double* b3) {
    FOTO_TRY(image_size_check(w, h, 2, "foto_gn_rhs"));
    CallScope S;
    FOTO_TRY(S.init());
    const size_t n = (size_t)w * h;
    double *d1, *d2, *fx, *fy, *ft, *b;
    FOTO_TRY(S.up(f1, n, &d1));
    FOTO_TRY(S.up(f2, n, &d2));
    FOTO_TRY(S.dev(n, &fx));
    FOTO_TRY(S.dev(n, &fy));
    FOTO_TRY(S.dev(n, &ft));
    FOTO_TRY(S.dev(3 * n, &b));
    FOTO_HIP_CHECK(launch_gn_coeffs(w, h, d1, d2, fx, fy, ft, S.s));
    FOTO_HIP_CHECK(launch_gn_rhs(w, h, fx, fy, d2, ft, b, S.s));
    FOTO_TRY(S.down(b3, b, 3 * n));
    return S.sync();
}

// classical.GLLOpticalFlow.process: PCG to rtol on the assembled-equivalent operator.
static int gn_solve_impl(const double* f1, const double* f2, int w, int h, double alpha, double lam, double rtol,
                         int maxiter, double* u, double* v, double* m, int* iterations, foto_gn_stats* st);

int foto_gn_solve(const double* f1, const double* f2, int w, int h, double alpha, double lam, double rtol,
                  int maxiter, double* u, double* v, double* m, int* iterations) {
    return gn_solve_impl(f1, f2, w, h, alpha, lam, rtol, maxiter, u, v, m, iterations, nullptr);
}

// Algorithmic HBM bytes of one MG-PCG iteration (bench.py gn_bytes_per_iteration):
// k_gnp_dir 12 n, k_gnp_upd 18 n, per level k_mg_down2 18 n_l + 3 n_l+1 and k_mg_up2 21 n_l + 3 n_l+1
// (level 0: 9 n_0 and 12 n_0, its B and D^-1 formed from fx, fy, f2; FOTO_GN_RECOMP=0 loads them
// and moves more than this counts), the coarsest level 18 n_c fp64 values; levels halve (rounding
// up) until <= 1024 cells.
static double gn_alg_bytes(int w, int h, int* levels) {
    std::vector<double> ns{(double)w * h};
    while ((double)w * h > 1024) {
        w = (w + 1) / 2;
        h = (h + 1) / 2;
        ns.push_back((double)w * h);
    }
    double v = 30.0 * ns[0];
    for (size_t l = 0; l + 1 < ns.size(); ++l) v += (l == 0 ? 21.0 : 39.0) * ns[l] + 6.0 * ns[l + 1];
    v += 18.0 * ns.back();
    if (levels) *levels = (int)ns.size();
    return 8.0 * v;
}

int foto_gn_solve_ex(const double* f1, const double* f2, int w, int h, double alpha, double lam, double rtol,
                     int maxiter, double* u, double* v, double* m, foto_gn_stats* st) {
    int its = 0;
    const auto t0 = std::chrono::steady_clock::now();
    if (st) memset(st, 0, sizeof(*st));
    const int rc = gn_solve_impl(f1, f2, w, h, alpha, lam, rtol, maxiter, u, v, m, &its, st);
    if (rc >= 0 && st) {
        st->iterations = its;
        st->info = rc;
        st->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return rc;
}

static int gn_solve_impl(const double* f1, const double* f2, int w, int h, double alpha, double lam, double rtol,
                         int maxiter, double* u, double* v, double* m, int* iterations, foto_gn_stats* st) {
    FOTO_TRY(image_size_check(w, h, 2, "foto_gn_solve"));
    if (!(alpha > 0) || !(lam > 0)) {
        set_error("GN needs alpha > 0 and lambda > 0 (the block-Jacobi preconditioner divides by them)");
        return FOTO_ERR_ARG;
    }
    if (maxiter < 0) { set_error("maxiter < 0"); return FOTO_ERR_ARG; }
    const Tuning tn = tuning_from_env();   // (a context-free entry: read here, once per call)
    if (tn.gn_mg) {   // FOTO_GN_MG=0: 3x3 block-Jacobi preconditioner (A/B runs)
        // multigrid-preconditioned CG through a plan (foto_gn.hip), cached per process like an
        // FFT plan: a call with the same (w, h, alpha, lambda, rtol, maxiter) as the previous
        // one reuses its buffers and graph (FOTO_GN_PLAN_CACHE=0: make and destroy a plan per call)
        const bool cache = tn.gn_plan_cache;
        // (the cached plan is never destroyed at process exit: the HIP runtime may be gone by then)
        static std::mutex mu;
        static foto_gn_plan* cached = nullptr;
        static double key[6] = {0, 0, 0, 0, 0, 0};
        const double k6[6] = {(double)w, (double)h, alpha, lam, rtol, (double)maxiter};
        std::lock_guard<std::mutex> lk(mu);
        int dev = 0;
        FOTO_HIP_CHECK(hipGetDevice(&dev));
        const bool reused = !(!cache || !cached || memcmp(key, k6, sizeof(k6)) != 0 || foto_gn_plan_device(cached) != dev);
        if (!reused) {
            foto_gn_plan_destroy(cached);
            cached = nullptr;
            FOTO_TRY(foto_gn_plan_create(w, h, alpha, lam, rtol, maxiter, &cached));
            memcpy(key, k6, sizeof(k6));
        }
        const int rc = foto_gn_plan_solve(cached, f1, f2, u, v, m, iterations);
        if (st && rc >= 0) {
            // (no early return here: the plan below must still be destroyed when caching is off,
            // and a timing readback cannot turn a finished solve into an error)
            double t4[4] = {0, 0, 0, 0};
            if (foto_gn_plan_timing(cached, t4) < 0) t4[0] = t4[1] = -1.0;
            st->ms_setup = t4[0];
            st->ms_pcg = t4[1];
            st->plan_reused = reused ? 1 : 0;
            st->alg_bytes_per_iter = gn_alg_bytes(w, h, &st->levels);
        }
        if (!cache || rc < 0) {
            foto_gn_plan_destroy(cached);
            cached = nullptr;
        }
        return rc;
    }
    // 3x3 block-Jacobi PCG (the first GPU version; kept for A/B runs)
    const int rc = gn_bj_solve(f1, f2, w, h, alpha, lam, rtol, maxiter, u, v, m, iterations);
    if (st && rc >= 0) {   // (no plan, no multigrid: 3 fields of 10 + 3 coefficient + 6 block-inverse values)
        st->levels = 0;
        st->alg_bytes_per_iter = 8.0 * (double)w * h * (3 * 10 + 3 + 6);
    }
    return rc;
}

}  // extern "C"
