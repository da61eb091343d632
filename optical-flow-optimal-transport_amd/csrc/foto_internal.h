// Internal declarations shared by the libfoto translation units (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/foto.h"
#include "foto_tuning.h"

namespace foto {

// ----------------------------------------------------------------------------- errors
void set_error(const char* fmt, ...);

#define FOTO_HIP_CHECK(call)                                                                  \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            ::foto::set_error("%s:%d %s: %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            return FOTO_ERR_HIP;                                                             \
        }                                                                                    \
    } while (0)

#define FOTO_TRY(expr)          \
    do {                        \
        int rc_ = (expr);       \
        if (rc_ < 0) return rc_; \
    } while (0)

// ----------------------------------------------------------------------------- streams
// Streams come from a process-wide pool (foto_host.cpp): a hipStreamCreate costs ~10 ms on the
// MI355X box (FOTO_GN_TRACE), which every BB context, GN plan and per-call scope paid -- a
// batch of solves paid it per solve.  acquire returns a stream of the current device; release
// takes back a stream with no work pending (callers synchronise first).  Never destroyed.
int stream_acquire(hipStream_t* out);
void stream_release(hipStream_t s);
int stream_device(hipStream_t s);   // the device a pooled stream belongs to (-1: not pooled)

// ----------------------------------------------------------------------------- size rules
// (foto_host.cpp) The only copies of the rules: FOTO_ERR_ARG with a message that starts with `who`.
// An image: both sides >= min_side (2 where a difference stencil or a bilinear tap runs, 1 for the
// pointwise entries) and w h < 2^31 (pixel indices are 32-bit in the kernels).
int image_size_check(int w, int h, int min_side, const char* who);
// A space-time grid: Nt >= 2, then the plane's image rule.
int grid_size_check(int Nt, int Nx, int Ny, const char* who, int min_side = 2);

// ----------------------------------------------------------------------------- geometry
// One time-slab shard of the (Nt, Ny, Nx) grid: local planes l in [0, nloc) are global
// planes t0 + l.  Every field array is allocated with one halo plane below (l = -1) and
// one above (l = nloc); the device pointer handed to kernels points at local plane 0.
struct Geo {
    int Nt, Ny, Nx;
    int t0, nloc;
    int64_t nxy;
};

constexpr int TX = 64;   // march tile width  (one wave = one 64-voxel x-row, 512 B of fp64)
constexpr int TY = 4;    // march tile height (4 waves, 256 threads)
constexpr int NT = 256;  // threads per block for every kernel

inline int march_blocks(const Geo& g) { return ((g.Nx + TX - 1) / TX) * ((g.Ny + TY - 1) / TY); }
inline int flat_blocks(int64_t n) { return (int)((n + NT - 1) / NT); }
// at least one block and at most `cap`: the kernel's grid-stride loop takes the rest
inline int capped_blocks(int64_t items, int cap) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((items + NT - 1) / NT, cap));
}
constexpr int STREAM_MAX_BLOCKS = 1 << 16;   // the streaming kernels (ingest, export, render)
constexpr int SUM_MAX_BLOCKS = 2048;         // launch_sum's partials

inline size_t dtype_bytes(int dtype) { return dtype == FOTO_U8 ? 1 : dtype == FOTO_F32 ? 4 : 8; }

inline int cus_count() {   // CUs of the current device (cached per device ordinal)
    static int cache[64] = {0};
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess) return cus;
    if (dev >= 0 && dev < 64 && cache[dev] > 0) return cache[dev];
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 256;
    if (dev >= 0 && dev < 64) cache[dev] = cus;
    return cus;
}

// Device-side CG scalars (one per shard).  Written only by the last block of a kernel
// (or by block 0 for the done flag); read by later kernels.
struct CGScal {
    double bb;     // b.b
    double atol;   // rtol * ||b||
    double rho;    // r_k . r_k of the current iteration (scipy's rho_cur)
    double pap;    // p_k . A p_k
    int done;      // converged (top-of-iteration test passed) or b == 0
    int iters;     // iteration index at which `done` was set
    int pad[2];
};

// The host loop of a CG that takes one step per launch (the stencil CG of foto_bb.cpp, the
// one-step spectral CG): step(k) enqueues iteration k; after the first `first` iterations, then
// after every 2, the scalars S are copied to the pinned hS and the host waits for them.  Ends at
// the done flag or at maxiter, with scipy's (iterations, info).
template <class Step>
int cg_poll_chunks(int first, int maxiter, Step&& step, const CGScal* S, CGScal* hS, hipStream_t s, bool* done,
                   int* iters, int* info) {
    *done = false;
    for (int k = 0; k < maxiter && !*done;) {
        const int chunk = std::min(k == 0 ? first : 2, maxiter - k);
        for (int j = 0; j < chunk; ++j, ++k) FOTO_TRY(step(k));
        FOTO_HIP_CHECK(hipMemcpyAsync(hS, S, sizeof(CGScal), hipMemcpyDeviceToHost, s));
        FOTO_HIP_CHECK(hipStreamSynchronize(s));
        *done = hS->done != 0;
    }
    *iters = *done ? hS->iters : maxiter;
    *info = *done ? 0 : maxiter;
    return 0;
}

// Per-shard reduction scratch: `partials` holds one value per block per quantity,
// `ticket` is the last-block counter, `gath` holds one slot per rank (allgathered).
struct RedBuf {
    double* partials;
    unsigned* ticket;
    int cap;   // blocks * quantities capacity
};

// ----------------------------------------------------------------------------- per-launch timing

struct KTimer {
    bool on = false;
    std::vector<hipEvent_t> pool;
    struct Pend { hipEvent_t a, b; int cls; double bytes; size_t id; };
    std::vector<Pend> pend;
    int64_t n[8] = {0};
    double ms[8] = {0};
    double bytes[8] = {0};

    hipEvent_t get() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        // timing only, no system-scope fence: a fenced record writes the L2's dirty lines back
        // before the next launch, which the untimed loop never does -- the launch after it then
        // ran on a clean L2 (k_prox_rhs 171 us against 179.5 in the loop)
        hipEvent_t e;
        if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) return nullptr;
        return e;
    }
    // returns the start event to be paired by stop()
    hipEvent_t start(hipStream_t s) {
        if (!on) return nullptr;
        hipEvent_t e = get();
        if (e) (void)hipEventRecord(e, s);
        return e;
    }
    void stop(hipEvent_t a, hipStream_t s, int cls, double by) {
        if (!on || !a) return;
        hipEvent_t b = get();
        if (!b) return;
        (void)hipEventRecord(b, s);
        pend.push_back({a, b, cls, by, next_id++});
    }
    // drop the `count` most recent pending records of class cls (launches that turned out to
    // be no-ops, e.g. s-step passes enqueued after the solve had finished)
    void discard_last(int cls, int count) {
        for (int i = (int)pend.size() - 1; i >= 0 && count > 0; --i) {
            if (pend[i].cls != cls) continue;
            pool.push_back(pend[i].a);
            pool.push_back(pend[i].b);
            pend.erase(pend.begin() + i);
            --count;
        }
    }
    // marks are record ids (records are pushed in id order; ids survive discard_last)
    size_t next_id = 0;
    size_t mark() const { return next_id; }
    size_t count_before(size_t m) const {
        size_t n = 0;
        while (n < pend.size() && pend[n].id < m) ++n;
        return n;
    }
    // drop every record from mark m on (launches of an outer iteration that was rolled back)
    void discard_from(size_t m) {
        const size_t keep = count_before(m);
        for (size_t k = keep; k < pend.size(); ++k) {
            pool.push_back(pend[k].a);
            pool.push_back(pend[k].b);
        }
        pend.resize(keep);
    }
    // the pending intervals before mark m (all complete: recorded before the last stream sync)
    void resolve_upto(size_t m) { resolve_first(count_before(m)); }
    void resolve_first(size_t n) {
        n = std::min(n, pend.size());
        for (size_t k = 0; k < n; ++k) {
            Pend& p = pend[k];
            float t = 0.f;
            if (hipEventElapsedTime(&t, p.a, p.b) == hipSuccess) {
                this->n[p.cls] += 1;
                ms[p.cls] += t;
                bytes[p.cls] += p.bytes;
            }
            pool.push_back(p.a);
            pool.push_back(p.b);
        }
        pend.erase(pend.begin(), pend.begin() + n);
    }
    void resolve() { resolve_first(pend.size()); }   // call after a stream sync
    void reset() {
        std::fill(n, n + 8, 0);
        std::fill(ms, ms + 8, 0.0);
        std::fill(bytes, bytes + 8, 0.0);
    }
    ~KTimer() {
        for (auto& p : pend) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
        for (auto e : pool) (void)hipEventDestroy(e);
    }
};


// ----------------------------------------------------------------------------- kernel launchers
// (defined in foto_kernels.hip; all enqueue on `s` and never synchronise)
struct CGArgs {
    double r, eps, rtol;
    int world, rank;
};

hipError_t launch_apply_A(const Geo& g, const double* p, double* out, double r, double eps, int lap_only,
                          hipStream_t s);
hipError_t launch_grad_st(const Geo& g, const double* phi, double* gt, double* gx, double* gy, hipStream_t s);
hipError_t launch_div_st(const Geo& g, const double* wt, const double* wx, const double* wy, double* out,
                         hipStream_t s);
hipError_t launch_grad2(int Nx, int Ny, const double* f, double* gx, double* gy, int bcD, hipStream_t s);
hipError_t launch_div2(int Nx, int Ny, const double* u, const double* v, double* out, int bcD, double sign,
                       hipStream_t s);
hipError_t launch_grad2_forward(int Nx, int Ny, const double* f, double* gx, double* gy, hipStream_t s);
hipError_t launch_stepB(int64_t M, const double* pa, const double* p1, const double* p2, double* qa,
                        double* q1, double* q2, hipStream_t s);
hipError_t launch_init_mu(const Geo& g, const double* rho0, const double* rhoT, double* mut, double* mux,
                          double* muy, double* qt, double* qx, double* qy, hipStream_t s);
// F = div_st(mu - r q) + BC, written to `F`; F.F partial -> gath[rank]
hipError_t launch_rhs(const Geo& g, const double* mut, const double* mux, const double* muy, const double* qt,
                      const double* qx, const double* qy, const double* rho0, const double* rhoT, double r,
                      double* F, RedBuf rb, double* gath, int rank, hipStream_t s);
// The transport report (foto_bb_report / _dev, foto_report_from_state): out[t][FOTO_REPORT_COLS]
// for the shard's planes t in [t0, t0 + nloc), one launch.  A block sums one piece of one plane;
// the pieces are a function of the plane size alone, so a plane's sums do not depend on the
// sharding.  part: Nt * FOTO_REPORT_COLS * report_pieces(nxy) doubles, laid out
// [plane][col][piece] (global plane); ticket: Nt counters, zero before the launch and left at zero.
constexpr int REPORT_PIECE = 2048;   // voxels of a plane per block
inline int report_pieces(int64_t nxy) { return (int)((nxy + REPORT_PIECE - 1) / REPORT_PIECE); }
struct ReportIn {
    const double *rho, *m1, *m2, *phi;   // the shard's mu and phi, at local plane 0
    // the plane below the shard's first / above its last one, from the shard that owns it (null
    // at the global ends): never mu's halo planes, which the fused path does not exchange
    const double *rho_lo, *rho_hi, *phi_lo, *phi_hi;
    const double *rho0, *rhoT;           // one plane each
};
hipError_t launch_report(const Geo& g, const ReportIn& in, double* part, unsigned* ticket, double* out,
                         hipStream_t s);
// stencil CG iteration kernels
hipError_t launch_cg_dir(const Geo& g, int k, const double* rvec, const double* pold, double* pnew,
                         const CGArgs& a, CGScal* S, RedBuf rb, const double* gath_rr, double* gath_pap,
                         int fused, hipStream_t s);
hipError_t launch_cg_pupd(const Geo& g, int k, const double* rvec, const double* pold, double* pnew,
                          CGScal* S, const double* gath_rr, const CGArgs& a, hipStream_t s);
hipError_t launch_cg_upd(const Geo& g, int k, const double* p, double* x, double* rvec, const CGArgs& a,
                         CGScal* S, RedBuf rb, const double* gath_pap, double* gath_rr, hipStream_t s);
// grad_st phi -> stepB -> mu update -> crit partial sums (num, den) -> gath[2*rank..]
hipError_t launch_prox(const Geo& g, const double* phi, double* mut, double* mux, double* muy, double* qt,
                       double* qx, double* qy, double r, RedBuf rb, double* gath, int rank, hipStream_t s,
                       const int* guard = nullptr);
// k_prox fused with the next iteration's RHS (mu -> nu, F, this rank's crit num/den ->
// gath_crit[0..1], F.F -> gath_rr[0] when non-null); needs rb.cap >= 3 * prox_rhs_blocks(g, tch).
// tch: planes per chunk (Tuning::pr_tch).
// Sharded (g.t0 > 0 or g.t0 + g.nloc < g.Nt), either: defer_lo / defer_hi = 0 -- stepB is
// recomputed on the neighbours' boundary planes: phi needs two valid halo planes on each side
// and mu one; or defer_lo / defer_hi = 1 on the sides that have a neighbour -- phi needs one
// halo plane, F of that edge plane is left to launch_rhs_edge after w_t's halo exchange
// (wt_out: a halo-padded field, planes 0, 1, nloc - 2, nloc - 1 written; edge: 2 x 4 planes).
int prox_rhs_blocks(const Geo& g, int tch);
// the fused kernel addresses a tile's phi region (12 rows) by 32-bit byte offsets: rows of up to
// ~2^25 voxels.  Wider grids take the separate k_prox + k_rhs (the same bits per voxel).
bool prox_rhs_fits(const Geo& g);
hipError_t launch_prox_rhs(const Geo& g, const double* phi, const double* mut, const double* mux, const double* muy,
                           double* nut, double* nux, double* nuy, const double* rho0, const double* rhoT, double r,
                           double* F, RedBuf rb, double* gath_crit, double* gath_rr, int tch, hipStream_t s,
                           const int* guard = nullptr, int defer_lo = 0, int defer_hi = 0, double* wt_out = nullptr,
                           double* edge = nullptr, double* hcrit = nullptr, int wt_pre = 0);
// w_t = mu'_t - r q_t of the deferred edge planes (0 if defer_lo, nloc - 1 if defer_hi) into
// wt, ahead of launch_prox_rhs (which then gets wt_pre = 1 and leaves those planes alone): the
// w_t exchange can travel while the fused kernel runs.  phi needs its halo planes.
hipError_t launch_wt_pre(const Geo& g, const double* phi, const double* mut, const double* mux, const double* muy,
                         double r, double* wt, int defer_lo, int defer_hi, hipStream_t s, const int* guard = nullptr);
// F of a deferred edge plane n (0 or nloc - 1; edge slot 0 or 1), F.F added to gath_rr[0]
hipError_t launch_rhs_edge(const Geo& g, int n, const double* wt, const double* edge, const double* rho0,
                           const double* rhoT, double r, double* F, RedBuf rb, double* gath_rr, hipStream_t s,
                           const int* guard = nullptr);
// q = Proj_K(grad_st phi + mu / r) only (the stepB output the fused kernel does not store)
hipError_t launch_q_from_phi(const Geo& g, const double* phi, const double* mut, const double* mux,
                             const double* muy, double* qt, double* qx, double* qy, double r, hipStream_t s);
// trajectory steps n in [n_lo, n_hi) using phi planes (local plane index l = n - t0)
hipError_t launch_traj(const Geo& g, const double* phi, int n_lo, int n_hi, double* px, double* py,
                       int init, hipStream_t s);
// The flow record of the positions px, py (the final flow and every record of the flow path):
// u = px - x, v = py - y, m = -div(bc 'D') [u; v] from the float64 u, v, and the export, in one
// kernel.  dtype FOTO_F32 | FOTO_F64; layout 0: ou[i], ov[i], om[i] (three planes, anywhere);
// layout 1: ou[2 i], ou[2 i + 1] = (u, v) (ov, om unused).
hipError_t launch_flow_record(int Nx, int Ny, const double* px, const double* py, void* ou, void* ov, void* om,
                              int dtype, int layout, hipStream_t s);

// Point tracking: launch_traj's steps n in [n_lo, n_hi) (within g's planes and below Nt - 1) for M
// start points pts[M][2] of FOTO_F32 | FOTO_F64, one launch.  all_steps = 1: record n -> out[n][M][2]
// (global n: `out` is the base of the whole [Nt-1][M][2] array); 0: the record of step Nt-2 ->
// out[M][2], stored by the launch that runs that step.  pos_in (null: start at pts) and pos_out
// (null: not stored) are [M][2] float64 running positions.  Records are displacements from pts.
hipError_t launch_track(const Geo& g, const double* phi, int n_lo, int n_hi, const void* pts, int pts_dtype,
                        const double* pos_in, double* pos_out, void* out, int dtype, int64_t M, int all_steps,
                        hipStream_t s);

hipError_t launch_dot_self(int64_t n, const double* x, RedBuf rb, double* gath, int rank, hipStream_t s);

// GN
hipError_t launch_gn_coeffs(int w, int h, const double* f1, const double* f2, double* fx, double* fy,
                            double* ft, hipStream_t s);
hipError_t launch_gn_rhs(int w, int h, const double* fx, const double* fy, const double* f2, const double* ft,
                         double* b, hipStream_t s);
hipError_t launch_gn_apply(int w, int h, const double* fx, const double* fy, const double* f2, double alpha,
                           double lam, const double* x, double* y, hipStream_t s);
// FOTO_GN_MG=0: the first-generation solver, CG with the 3x3 block-Jacobi preconditioner, from the
// caller's host frames to the host flow; returns 0 (converged) or maxiter, *iterations as run
int gn_bj_solve(const double* f1, const double* f2, int w, int h, double alpha, double lam, double rtol, int maxiter,
                double* u, double* v, double* m, int* iterations);

// ----------------------------------------------------------------------------- device buffers
// (foto_dev.hip; the *_dev entries of include/foto.h)
// foto_image_check's rules; `who` prefixes the message
int image_check(const foto_image* im, int w, int h, const char* who);
// image_check, then hipPointerGetAttributes: the pixels must be device memory of `device`
int image_dev_check(const foto_image* im, int w, int h, int device, const char* who);
// [p, p + bytes) is device memory of `device`
int dev_ptr_check(const void* p, size_t bytes, int device, const char* who, const char* what);
// an export target: dtype F32 | F64, layout 0 | 1, n pixels, device memory of `device`
int export_check(const void* out, int dtype, int layout, int64_t n, int device, const char* who);
// point tracking (foto_bb_track / _dev, foto_track_from_phi), host-only: non-null pointers, M in
// [1, 2^31 - 1], all_steps 0 | 1; a device array of (x, y) pairs: dtype F32 | F64, aligned to a pair
int track_arg_check(const void* pts, const void* out, int64_t M, int all_steps, const char* who);
int track_dtype_check(const void* p, int dtype, const char* who, const char* what);
// dst[row * w + col] = (double)pixel(row, col) / divisor
hipError_t launch_ingest(const foto_image& im, int w, int h, double* dst, hipStream_t s);
// tot[0] = sum of x[0..n) in a fixed order; part holds capped_blocks(n, SUM_MAX_BLOCKS) doubles
hipError_t launch_sum(int64_t n, const double* x, double* part, double* tot, hipStream_t s);
hipError_t launch_div_scalar(int64_t n, double* x, const double* S, hipStream_t s);   // x /= S[0]
// layout 0: out[3][n] = a, b, c; 1: out[n][2] = (a, b); dtype FOTO_F32 | FOTO_F64
hipError_t launch_export(int64_t n, const double* a, const double* b, const double* c, void* out, int dtype,
                         int layout, hipStream_t s);
// The frames of one k_frames launch, passed by value (no device scratch): frame k is
// scale * ((1 - w) a + w b) of two planes of n doubles; w == 0 reads a alone, w == 1 b alone.
constexpr int FRAMES_MAX = 128;
struct FrameArgs {
    const double* a[FRAMES_MAX];
    const double* b[FRAMES_MAX];
    double w[FRAMES_MAX];
};
// out[count][n] of dtype FOTO_U8 | FOTO_F32 | FOTO_F64, count <= FRAMES_MAX, one launch
hipError_t launch_frames(const FrameArgs& fa, int count, int64_t n, double scale, void* out, int dtype,
                         hipStream_t s);

// Maps and in-betweens (foto_interp.hip; foto_bb_maps / _dev, foto_bb_interp_dev, the *_from_phi
// test entries).  A launch covers count <= MAPS_MAX times, passed by value, and the pixels in
// MT_W x MT_H tiles.  Plane m of phi is table[m], a device array of Nt pointers that
// launch_plane_table fills from up to PLANE_SEGS buffers (segment k: planes [t0, t0 + nloc) at
// base; more buffers: more launches).
constexpr int MAPS_MAX = 128;
constexpr int MT_W = 32, MT_H = 8;
constexpr int PLANE_SEGS = 32;
struct MapTimes {
    double s[MAPS_MAX];
};
struct PlaneSegs {
    const double* base[PLANE_SEGS];
    int t0[PLANE_SEGS], nloc[PLANE_SEGS];
    int n;
};
hipError_t launch_plane_table(const PlaneSegs& sg, int64_t nxy, const double** table, hipStream_t s);
// out[count][4][Ny][Nx] = (a_x - x, a_y - y, b_x - x, b_y - y) of dtype FOTO_F32 | FOTO_F64; s: a host array
hipError_t launch_maps(const double* const* table, int Nt, int Nx, int Ny, const double* s, int count, int inv_iters,
                       void* out, int dtype, hipStream_t st);
// out[count][Ny][Nx][channels] of FOTO_U8 | FOTO_F32 | FOTO_F64; f0 / f1 describe channel 0, channel c
// starts c * sc0 / sc1 elements further on
hipError_t launch_interp(const double* const* table, int Nt, int Nx, int Ny, const foto_image& f0, int64_t sc0,
                         const foto_image& f1, int64_t sc1, int channels, const double* s, int count, int inv_iters,
                         void* out, int out_dtype, hipStream_t st);
// host-only rules: non-null s and out, count >= 1, inv_iters in [1, FOTO_INV_ITERS_MAX], every s[k]
// finite and in [0, Nt - 1]; a frame of `channels` channels: foto_render_warp_dev's rules
int maps_arg_check(const double* s, const void* out, int count, int inv_iters, int Nt, const char* who);
int interp_frame_check(const foto_image* f, int channels, int64_t stride_c, int w, int h, const char* who);
size_t interp_frame_bytes(const foto_image* f, int channels, int64_t stride_c, int w, int h);   // all channels
// a flow descriptor for w x h records (foto_render.hip; foto_flow_check's rules, host-only) and
// the bytes it covers
int flow_check(const foto_flow* fl, int w, int h, const char* who);
size_t flow_bytes(const foto_flow* fl, int w, int h);
inline bool overlaps(const void* a, size_t na, const void* b, size_t nb) {   // byte ranges
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

// A grow-only device scratch (the holder frees p).  Growing waits for `s` first: an earlier
// call's launches there may still read the buffer being replaced.
struct DevScratch {
    void* p = nullptr;
    size_t cap = 0;   // bytes
    int reserve(size_t bytes, hipStream_t s) {
        if (cap >= bytes) return 0;
        FOTO_HIP_CHECK(hipStreamSynchronize(s));
        if (p) FOTO_HIP_CHECK(hipFree(p));
        p = nullptr;
        cap = 0;
        FOTO_HIP_CHECK(hipMalloc(&p, bytes));
        cap = bytes;
        return 0;
    }
};

// The stream contract of every *_dev call: libfoto's streams are non-blocking, so the caller's
// stream (NULL: the legacy null stream) and the own one are ordered by two events, made once per
// context / plan.  enter: what `user` has enqueued happens before what `own` runs next;
// leave: what `own` has enqueued happens before what `user` runs next.
struct StreamLink {
    hipEvent_t in = nullptr, out = nullptr;
    int enter(hipStream_t user, hipStream_t own);
    int leave(hipStream_t own, hipStream_t user);
    ~StreamLink();
};

}  // namespace foto
