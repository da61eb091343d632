/*
 * libfoto -- MI355X-native FOTO hot path (Benamou-Brenier dynamic-OT optical flow
 * solver + the Gennert-Negahdaripour variational baseline) behind a plain C ABI.
 *
 * Every entry point takes caller-owned HOST buffers (float64, row-major, the layout
 * of the reference: voxel k = n*Nx*Ny + j*Nx + i, 3-field vectors SoA
 * [t-part; x-part; y-part]) and returns 0 on success, < 0 on error
 * (foto_last_error() has the message).  Each declaration cites the reference
 * interface it replaces (paths relative to the reference repository root).
 * The *_dev entries at the end of this header are the same calls on DEVICE memory.
 *
 * The reference is pure Python (numpy/scipy); its "FFI" for this path is the
 * Python call surface.  The binding a maintainer adds is the ctypes layer in
 * optical-flow-optimal-transport_amd/foto/_lib.py.
 */
#ifndef FOTO_H
#define FOTO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FOTO_OK 0
#define FOTO_ERR_ARG (-1)     /* bad sizes / arguments (reference: IndexError, ZeroDivisionError) */
#define FOTO_ERR_HIP (-2)     /* HIP runtime error (no device, OOM, launch failure)              */
#define FOTO_ERR_COMM (-3)    /* RCCL error                                                      */
#define FOTO_ERR_STATE (-4)   /* call out of order (e.g. flow before any iteration)              */
#define FOTO_ERR_BC (-5)      /* boundary condition not in {'N','D'}: NotImplementedError        */

const char* foto_last_error(void);
int foto_version(void);
int foto_device_count(int* n);

/* ------------------------------------------------------------------ operators
 * Matrix-free applications of the sparse operators of operators.py (h = 1).   */

/* operators.grad_st(Nt,Nx,Ny,1,1,1,'N') @ phi  (operators.py:114-127)       -> out3[3N] */
int foto_grad_st(const double* phi, int Nt, int Nx, int Ny, double* out3);
/* operators.div_st(Nt,Nx,Ny,1,1,1,'N') @ w3    (operators.py:129-142)       -> out[N]   */
int foto_div_st(const double* w3, int Nt, int Nx, int Ny, double* out);
/* operators.laplacian_st(Nt,Nx,Ny,1,1,1,'N') @ p (operators.py:144-157)     -> out[N]   */
int foto_laplacian_st(const double* p, int Nt, int Nx, int Ny, double* out);
/* (-r*L_st + r*eps*I) @ p                      (benamou_brenier.py:202-203) -> out[N]   */
int foto_apply_A(const double* p, int Nt, int Nx, int Ny, double r, double eps, double* out);
/* operators.grad(Nx,Ny,1,1,bc) @ f             (operators.py:160-169)       -> out2[2*Nx*Ny] */
int foto_grad2(const double* f, int Nx, int Ny, char bc, double* out2);
/* operators.div(Nx,Ny,1,1,bc) @ [u;v]          (operators.py:182-191)       -> out[Nx*Ny] */
int foto_div2(const double* uv, int Nx, int Ny, char bc, double* out);
/* operators.grad_forward(Nx,Ny,1,1,'N') @ f    (operators.py:171-180)       -> out2[2*Nx*Ny] */
int foto_grad2_forward(const double* f, int Nx, int Ny, double* out2);

/* ------------------------------------------------------------------ BB building blocks */

/* benamou_brenier.stepB(p, ...)  (benamou_brenier.py:93-149); M = Nt*Nx*Ny        */
int foto_stepB(const double* p3, int64_t M, double* q3);
/* RHS of solve_benamou_brenier_step: div_st(mu - r q) + temporal BC correction
 * (benamou_brenier.py:64-82)                                                       */
int foto_bb_rhs(const double* mu3, const double* q3, const double* rho0, const double* rhoT,
                int Nt, int Nx, int Ny, double r, double* F);
/* scipy.sparse.linalg.cg(A, b, rtol, maxiter) with A = -r L_st + r eps I, x0 = 0
 * (benamou_brenier.py:85).  Returns info (0 converged, maxiter otherwise) or < 0;
 * *iterations = CG iterations run.  mode: 0 = stencil CG, 1 = spectral CG,
 * 2 = spectral s-step CG, 3 = Gauss-compressed spectral CG (foto_bb_opts.cg_mode). */
int foto_cg(const double* b, int Nt, int Nx, int Ny, double r, double eps, double rtol, int maxiter,
            int mode, double* x, int* iterations);
/* utils.opticalflow_from_benamoubrenier(phi, Nt, Nx, Ny, grad('N'), div('D'))
 * (utils.py:44-99, 148-183)                                                        */
int foto_flow_from_phi(const double* phi, int Nt, int Nx, int Ny, double* u, double* v, double* m);
/* Test entry: the flow path of foto_bb_flow_path (below) from a caller's phi, without a context.
 * Record n-1 (n = 1..Nt-1) = utils.opticalflow_from_benamoubrenier(phi[: (n+1)*Nx*Ny], n+1, Nx,
 * Ny, grad('N'), div('D')): the displacement after the first n steps of
 * utils.reconstructTrajectory (utils.py:63-97) and m = -div('D')[u; v] (utils.py:181).
 * u, v, m: each [Nt-1][Ny*Nx]; record Nt-2 carries the bits of foto_flow_from_phi.       */
int foto_flow_path_from_phi(const double* phi, int Nt, int Nx, int Ny, double* u, double* v, double* m);
/* Test entry: the records of foto_bb_track (below) from a caller's phi, without a context:
 * utils.reconstructTrajectory(x, y, un, vn, Nx, Ny, n+1) (utils.py:44-99) for M start points
 * pts[M][2] = (x, y), un / vn = grad('N') of the phi planes.  out: [Nt-1][M][2] (all_steps = 1) or
 * [M][2] (all_steps = 0).  FOTO_ERR_ARG (before any device is touched): a null pointer, Nt < 2,
 * M < 1 or > 2^31 - 1, all_steps not 0 / 1.                                                      */
int foto_track_from_phi(const double* phi, int Nt, int Nx, int Ny, const double* pts, int64_t M,
                        int all_steps, double* out);
/* Test entries: the records of foto_bb_maps and the images of foto_bb_interp_dev (below, "maps and
 * in-betweens") from a caller's phi, without a context; host float64 throughout.  s: count plane
 * positions in [0, Nt-1].  Maps: out[count][4][Ny][Nx].  In-betweens: f0, f1 are [Ny][Nx][channels]
 * (HWC, divisor 1), out is [count][Ny][Nx][channels].  FOTO_ERR_ARG (before any device is touched):
 * a null pointer, Nt < 2, Nx or Ny < 2, count < 1, channels < 1, an s[k] outside [0, Nt-1] or not
 * finite, inv_iters outside [1, FOTO_INV_ITERS_MAX].                                             */
int foto_maps_from_phi(const double* phi, int Nt, int Nx, int Ny, const double* s, int count, int inv_iters,
                       double* out);
int foto_interp_from_phi(const double* phi, int Nt, int Nx, int Ny, const double* f0, const double* f1,
                         int channels, const double* s, int count, int inv_iters, double* out);

/* ------------------------------------------------------------------ BB solver context
 * benamou_brenier.solve (benamou_brenier.py:151-271) split into create / iterate /
 * flow so a caller can keep the state resident in HBM between calls.             */
typedef struct foto_bb_ctx foto_bb_ctx;

typedef struct {
    int device;           /* HIP device ordinal; -1 = current device                       */
    int cg_maxiter;       /* 1000 (benamou_brenier.py:85)                                  */
    double cg_rtol;       /* 1e-6 (benamou_brenier.py:85)                                  */
    int cg_mode;          /* 0 = stencil CG (7-point matvec), 1 = spectral CG (DCT-II      */
                          /* eigenbasis, one pass / iteration), 2 = spectral s-step CG     */
                          /* (one pass / up to 8 iterations, any world; mode 1 needs       */
                          /* world == 1; eps <= 0 selects mode 0), 3 = spectral CG on the  */
                          /* Gauss-compressed measure of b^ (one read of b^, the           */
                          /* recurrence on 2048 nodes, any world); < 0 = auto (default):   */
                          /* 0 on grids of <= 2^18 voxels (FOTO_CG_AUTO_MAX), 3 above      */
    int rank, world;      /* time-slab sharding over `world` processes (RCCL); 1 = single  */
    const void* nccl_id;  /* 128-byte ncclUniqueId (foto_nccl_unique_id on rank 0)         */
    int virtual_ranks;    /* >1: shard over this many in-process slabs on ONE device       */
                          /* (tests the sharded path without RCCL; world must be 1)       */
    int timing;           /* 1: time every kernel launch with HIP events (foto_bb_stats)   */
} foto_bb_opts;

/* per outer iteration: crit and the CG iteration count / info of that stepA */
typedef void (*foto_bb_iter_cb)(void* user, int iter, double crit, int cg_iters, int cg_info);

typedef struct {
    int outer_iters;          /* outer iterations completed so far                      */
    int64_t cg_iters_total;   /* CG iterations over all outer iterations                */
    double last_crit;
    double ms_rhs, ms_cg, ms_prox, ms_flow;   /* phase wall time (HIP events; RHS / CG / prox
                                                 only with timing = 1)                   */
    /* per kernel class (timing = 1): launches and summed device time in ms            */
    int64_t n_k[8];
    double ms_k[8];
    double bytes_k[8];        /* algorithmic HBM bytes of those launches, summed        */
    int cg_redo;              /* outer iterations whose deferred CG solve (see foto_bb.cpp) */
                              /* outran its predicted passes and re-ran prox             */
} foto_bb_stats;

/* kernel classes reported in foto_bb_stats.n_k / ms_k / bytes_k */
#define FOTO_K_CG_DIR    0   /* stencil CG: p = r + beta p, A p, p.Ap                    */
#define FOTO_K_CG_UPD    1   /* stencil CG: x += alpha p, r -= alpha A p, r.r            */
#define FOTO_K_RHS       2   /* div_st(mu - r q) + BC                                    */
#define FOTO_K_PROX      3   /* grad_st phi, stepB, mu update, crit sums                 */
#define FOTO_K_SPEC      4   /* spectral CG iteration kernel(s)                          */
#define FOTO_K_DCT       5   /* DCT-II transforms                                        */
#define FOTO_K_FLOW      6   /* trajectory integration + divergence                      */
#define FOTO_K_SLAB      7   /* sharded: the slab-side x / y DCTs (what the pipelined     */
                             /* all-to-alls overlap with communication)                  */
#define FOTO_K_OTHER     FOTO_K_SLAB   /* (older name)                                    */

int foto_bb_opts_default(foto_bb_opts* o);
int foto_bb_create(const double* rho0, const double* rhoT, int Nt, int Nx, int Ny, double r,
                   double reg_epsilon, const foto_bb_opts* opts, foto_bb_ctx** out);
/* Run up to `max_iters` outer iterations (stepA + stepB + stepC + criterion).  With
 * use_stop_rules = 1 it stops like the reference (crit <= tol, or |dcrit| < 1e-5).
 * cb (may be NULL) gets (iteration index, crit, CG iterations, CG info) after each
 * outer iteration.  Returns 1 if a stop rule fired, 0 otherwise, < 0 on error.
 * The callback runs while the NEXT outer iteration is already on the stream.  In the
 * default single-GPU loop (two iterations in flight) foto_bb_get_phi / get_state / flow
 * called from it return the state of the iteration the callback reports (kept intact for a
 * rollback); the one-in-flight loop (sharded, FOTO_PIPE=0) refuses them there with
 * FOTO_ERR_STATE (its next solve overwrites phi).  An error with iterations in flight drains
 * the stream and leaves the context refusing iterate / flow until foto_bb_reset.
 * foto_bb_reset and a nested foto_bb_iterate from the callback return FOTO_ERR_STATE.   */
int foto_bb_iterate(foto_bb_ctx* c, int max_iters, double convergence_tol, int use_stop_rules,
                    foto_bb_iter_cb cb, void* user, int* iters_done);
/* Flow (u, v, m) from the last phi: utils.opticalflow_from_benamoubrenier.
 * With world > 1 the result lands on rank 0; other ranks may pass NULL.           */
int foto_bb_flow(foto_bb_ctx* c, double* u, double* v, double* m);
/* A new pair (rho0, rhoT) of the same size on an existing context: every field, counter and
 * prediction back to what foto_bb_create leaves, so the solve is bit-identical to one on a
 * fresh context -- without its allocations, DCT plans and stream (a batch of same-size
 * frames: run.sh:81-157 runs one solve per sequence).  Also the way back after a failed
 * foto_bb_iterate (whatever it left on the stream is drained first).                     */
int foto_bb_reset(foto_bb_ctx* c, const double* rho0, const double* rhoT);
/* Copy this shard's slab range of phi / mu / q to host (t0, nloc via foto_bb_shard). */
int foto_bb_get_phi(foto_bb_ctx* c, double* phi);
int foto_bb_get_state(foto_bb_ctx* c, double* mu3, double* q3);
int foto_bb_shard(const foto_bb_ctx* c, int* t0, int* nloc);
/* Ranks of the context's RCCL communicator (ncclCommCount); 0 for a context without one (one
 * GPU, or virtual ranks in one process).                                                   */
int foto_bb_comm_size(const foto_bb_ctx* c, int* nranks);
int foto_bb_stats_get(const foto_bb_ctx* c, foto_bb_stats* st);
int foto_bb_stats_reset(foto_bb_ctx* c);
/* enable / disable per-launch HIP-event timing (foto_bb_stats.n_k / ms_k) */
int foto_bb_set_timing(foto_bb_ctx* c, int on);
int foto_bb_sync(foto_bb_ctx* c);
void foto_bb_destroy(foto_bb_ctx* c);

/* One-shot benamou_brenier.solve(rho0, rhoT, Nt, Nx, Ny, r, convergence_tol,
 * reg_epsilon, max_it) -> (u, v, m) on one GPU.                                     */
int foto_bb_solve(const double* rho0, const double* rhoT, int Nt, int Nx, int Ny, double r,
                  double convergence_tol, double reg_epsilon, int max_it, foto_bb_iter_cb cb, void* user,
                  double* u, double* v, double* m);

/* Per-solve report of foto_bb_solve_ex (outer iterations, the per-iteration
 * crit and CG counts, per-phase time and HBM bytes).  The caller owns the three arrays (any may
 * be NULL) and sets cap to their length; entries beyond cap are counted but not stored.       */
typedef struct {
    int cap;                  /* in: length of crit / cg_its / cg_info                        */
    double* crit;             /* out: crit of outer iteration i (benamou_brenier.py:249)       */
    int* cg_its;              /* out: CG iterations of that stepA (scipy cg at :85)           */
    int* cg_info;             /* out: CG info (0 converged, maxiter otherwise; :86-87 warning) */
    int outer_iters;          /* out: outer iterations run                                    */
    int stopped;              /* out: 1 if a stop rule ended the run (:253-258)               */
    int phi_t0, phi_nloc;     /* out: the time planes phi_or_null received (this rank's slab) */
    double ms_create;         /* out: host wall time of context creation (uploads, plans)     */
    double ms_loop;           /* out: host wall time of the outer-iteration loop (the metric) */
    double ms_flow;           /* out: host wall time of the flow extraction + download        */
    double alg_bytes_per_iter;/* out: algorithmic HBM bytes of one outer iteration on this
                                 rank (188 B per voxel for the default path)     */
    foto_bb_stats bb;         /* out: the context's counters (kernel classes with opts.timing) */
} foto_bb_solve_stats;

/* One-shot benamou_brenier.solve (benamou_brenier.py:151-271) with the options of a context
 * (opts may be NULL: foto_bb_opts_default; opts->world > 1: this process is rank opts->rank of
 * a time-slab sharded solve over RCCL -- config 4 -- and every rank calls it with the same
 * arguments), the reference's stop rules, and the per-solve report above.  (u, v, m) land on
 * rank 0 (other ranks may pass NULL); phi_or_null gets this rank's slab of the last phi
 * (st->phi_t0, st->phi_nloc planes; all Nt planes on one GPU).  st may be NULL.  Returns 0,
 * or < 0 on error; CG non-convergence is reported in st->cg_info (a warning, not an error). */
int foto_bb_solve_ex(const double* rho0, const double* rhoT, int Nt, int Nx, int Ny, double r,
                     double convergence_tol, double reg_epsilon, int max_it, const foto_bb_opts* opts,
                     double* u, double* v, double* m, double* phi_or_null, foto_bb_solve_stats* st);

/* RCCL unique id for foto_bb_opts.nccl_id (call on rank 0, broadcast 128 bytes). */
int foto_nccl_unique_id(void* out128);

/* Test entry (host only, no device): the point-to-point calls rank `rank` of `world` issues
 * over RCCL for one exchange of the time-sharded solve (the loop of benamou_brenier.py:204-258
 * split into time slabs), in issue order.  Each call is 5 int64:
 * {op (FOTO_CALL_*), peer, offset, count, copy destination offset}, offsets in doubles from
 * the buffer the exchange picks (send / copy: source; recv: destination).  Sends and receives
 * go in one ncclGroupStart/End; copies follow the group.  arg: the relay step j (RELAY).    */
#define FOTO_XFER_HALO 0          /* halo planes of a slab field (plane -1 / nloc)            */
#define FOTO_XFER_SLAB_TO_BOX 1   /* spectral all-to-all: time slabs -> row boxes             */
#define FOTO_XFER_BOX_TO_SLAB 2   /* spectral all-to-all: row boxes -> time slabs             */
#define FOTO_XFER_RELAY 3         /* trajectory positions rank j -> j + 1 (flow extraction)   */
#define FOTO_XFER_DELIVER 4       /* (u, v, m) last rank -> rank 0                            */
#define FOTO_XFER_HALO2 5         /* two halo planes per side (phi of the fused prox + RHS)   */
/* the pipelined all-to-alls: arg = part | parts << 8 | halo << 16 (foto_xfer.h
 * alltoall_part_xfers; the backward one with halo = 1 also delivers phi's halo planes)       */
#define FOTO_XFER_SLAB_TO_BOX_PART 6
#define FOTO_XFER_BOX_TO_SLAB_PART 7
#define FOTO_CALL_SEND 0
#define FOTO_CALL_RECV 1
#define FOTO_CALL_COPY 2
int foto_xfer_calls(int kind, int Nt, int Ny, int Nx, int world, int rank, int arg, int64_t* out, int cap,
                    int* count);

/* Test entry: the orthonormal DCT-II (inverse = 0) or DCT-III (inverse = 1) along the middle
 * axis of a C-order [outer][n][inner] array, as scipy.fft.dct(x, type=2|3, norm="ortho",
 * axis=1) -- the transform pair that diagonalises lap1d (operators.py:33-48) in the spectral
 * CG.  path 0: the FFT kernels when n has a plan, else the MFMA GEMM kernels; 1: FFT only
 * (error without a plan); 2: GEMM only.                                            */
int foto_dct(const double* in, int outer, int n, int inner, int inverse, int path, double* out);

/* Measurement entry (bench.py): the dominant s-step pass's memory traffic alone -- read and
 * write two n-double vectors, 16 B per lane, no arithmetic beyond one update -- timed over
 * `reps` back-to-back launches on this device; us[0] plain stores, us[1] write-through (sc1)
 * stores, microseconds per launch (best of 3).  n even, n * 8 < 2^31.                   */
int foto_stream_probe(int64_t n, int reps, double* us);

/* Measurement entry (bench.py): the fused prox + RHS kernel's traffic alone -- read four
 * n-double fields, write four others (64 B per voxel, the working set well beyond the
 * Infinity Cache at the bench size), one update per element -- microseconds per launch
 * (best of 3 over `reps` launches) in us[0].  n even.                                      */
int foto_stream_probe4(int64_t n, int reps, double* us);

/* ------------------------------------------------------------------ GN baseline
 * classical.GLLOpticalFlow (classical.py:25-130).                                 */
/* assemble(f1, f2).A @ x and .b (classical.py:68-111)                             */
int foto_gn_apply(const double* f1, const double* f2, int w, int h, double alpha, double lambda_,
                  const double* x3, double* y3);
int foto_gn_rhs(const double* f1, const double* f2, int w, int h, double* b3);
/* process(): spsolve replaced by CG preconditioned by one multigrid V-cycle (damped
 * block-Jacobi smoothing on each level; FOTO_GN_MG=0: the plain 3x3 block-Jacobi PCG) to rtol
 * (default 1e-10).
 * Returns 0 (converged) or maxiter (not converged), < 0 on error.  Runs on a plan (below)
 * cached per process for the last (w, h, alpha, lambda, rtol, maxiter, device), as FFT
 * libraries cache plans; FOTO_GN_PLAN_CACHE=0 makes and destroys one per call.       */
int foto_gn_solve(const double* f1, const double* f2, int w, int h, double alpha, double lambda_,
                  double rtol, int maxiter, double* u, double* v, double* m, int* iterations);

/* Per-solve report of foto_gn_solve_ex (SURVEY.md §8(b) foto_gn_stats).                      */
typedef struct {
    int iterations;           /* PCG iterations run                                            */
    int info;                 /* 0 converged, maxiter otherwise (the return value)             */
    int plan_reused;          /* 1: the cached plan of the previous call served this one       */
    int levels;               /* multigrid levels of the preconditioner                        */
    double ms_setup;          /* device time: upload, coefficients, RHS, V-cycle of r0          */
    double ms_pcg;            /* device time of the PCG iterations                             */
    double ms_total;          /* host wall time of the call                                    */
    double alg_bytes_per_iter;/* algorithmic HBM bytes of one PCG iteration   */
} foto_gn_stats;

/* foto_gn_solve with the report above (st may be NULL).                                      */
int foto_gn_solve_ex(const double* f1, const double* f2, int w, int h, double alpha, double lambda_,
                     double rtol, int maxiter, double* u, double* v, double* m, foto_gn_stats* st);

/* A reusable GLLOpticalFlow(w, h) with setAlpha/setLambda applied (classical.py:25-66): device
 * buffers, the multigrid hierarchy and the replayed PCG graph are made once; every
 * foto_gn_plan_solve is one process(f1, f2) (classical.py:68-130: coefficients, right-hand
 * side, multigrid coefficients, PCG) with the same result and return codes as foto_gn_solve.
 * Batches of same-size pairs (run.sh:81-157) reuse one plan.                       */
typedef struct foto_gn_plan foto_gn_plan;
int foto_gn_plan_create(int w, int h, double alpha, double lambda_, double rtol, int maxiter, foto_gn_plan** out);
int foto_gn_plan_solve(foto_gn_plan* p, const double* f1, const double* f2, double* u, double* v, double* m,
                       int* iterations);
/* the last solve: {ms upload + setup + V-cycle of r0, ms PCG iterations (device events),
 * iterations, iterations launched}                                                */
int foto_gn_plan_timing(const foto_gn_plan* p, double* out4);
/* the device the plan was made on (-1 for NULL)                                    */
int foto_gn_plan_device(const foto_gn_plan* p);
void foto_gn_plan_destroy(foto_gn_plan* p);

/* ------------------------------------------------------------------ evaluation
 * the warp and the error metrics of utils.py on the GPU.      */
/* utils.apply_opticalflow(f1, u, v, w, h, m) (utils.py:186-248): backward bilinear
 * warp of (1 + m) f1 (m may be NULL: f1 unscaled).  Bit-identical to the reference.
 * Deviation: a pixel with a NaN displacement is NaN, read from in-frame taps (pixel (0, 0)'s
 * row / column); the reference's int(nan) index raises.                              */
int foto_warp(const double* f1, const double* u, const double* v, const double* m, int w, int h, double* out);
/* utils.EE and utils.AE (utils.py:294-338): out4 = {AEE, SDEE, AAE, SDAE}; EE > 50 and
 * NaN angular errors are ignored as in the reference.                               */
int foto_flow_errors(const double* u, const double* v, const double* uGT, const double* vGT, int w, int h,
                     double* out4);
/* utils.IE (utils.py:340-354): RMS of 255 I - 255 IGT.                              */
int foto_intensity_error(const double* I, const double* IGT, int w, int h, double* ie);

/* ------------------------------------------------------------------ device buffers
 * The same solvers and metrics for a caller whose frames are already in HBM (a decoder, a
 * PyTorch-ROCm tensor, the output of an earlier foto_*_dev call): frames in, flow out, without
 * the round trip through host float64 arrays.  Additive: every entry above is unchanged.
 *
 * Stream contract, identical for every *_dev call: `stream` is the caller's hipStream_t (NULL:
 * the legacy null stream).  libfoto's own streams are non-blocking, so each call makes its
 * stream wait for what `stream` has enqueued before it first reads an input or writes an output,
 * and makes `stream` wait for its last write before it returns.  On return the inputs may be
 * overwritten and the outputs consumed by work queued on `stream`, with no host synchronisation
 * by the caller.  Every device pointer is checked with hipPointerGetAttributes to be device
 * memory of the context's / plan's / current device before anything is enqueued (host memory
 * or another GPU's: FOTO_ERR_ARG, never dereferenced).                                      */
#define FOTO_U8 0
#define FOTO_F32 1
#define FOTO_F64 2
/* One grey-scale frame as a strided view: what utils.openGrayscaleImage (utils.py:39-42) returns
 * -- np.float64(PIL 'L' image) / 255 -- is {u8 pixels, FOTO_U8, pitch, 1, 255.0}; a row-padded
 * frame, one channel of an interleaved [H][W][C] array and a transposed view are strides.   */
typedef struct {
    const void* data;      /* DEVICE pointer to pixel (row 0, column 0)                    */
    int dtype;             /* FOTO_U8 / FOTO_F32 / FOTO_F64                                */
    int64_t stride_y, stride_x;   /* in ELEMENTS, both > 0                                 */
    double divisor;        /* value = (double)pixel / divisor (255 for 8-bit images, 1 otherwise) */
} foto_image;

/* Host-only validation of a descriptor for a w x h frame (no HIP call): FOTO_ERR_ARG for null
 * data, a dtype outside 0..2, a stride <= 0, a divisor that is 0 or not finite, data not aligned
 * to its element size, or rows (columns, for a transposed view) that overlap.  Every entry
 * below calls it first (utils.openGrayscaleImage, utils.py:39-42, has no such view to check). */
int foto_image_check(const foto_image* im, int w, int h);

/* foto_bb_create / foto_bb_reset from device frames (w = Nx, h = Ny): the context is left in
 * exactly the state the host entries leave for rho = (double)pixel / divisor, so the solve that
 * follows is bit-identical.  normalize = 1 divides each frame by its own sum (main.py:71-74:
 * f0 / np.sum(f0)), a fixed-order device reduction, reported in sums2_or_null[0..1] ({1, 1}
 * with normalize = 0).  world == 1 only (virtual_ranks > 1 included); an RCCL context returns
 * FOTO_ERR_STATE.  An argument error leaves an existing context untouched.               */
int foto_bb_create_dev(const foto_image* f0, const foto_image* f1, int normalize, void* stream, int Nt, int Nx,
                       int Ny, double r, double reg_epsilon, const foto_bb_opts* opts, double* sums2_or_null,
                       foto_bb_ctx** out);
int foto_bb_reset_dev(foto_bb_ctx* c, const foto_image* f0, const foto_image* f1, int normalize, void* stream,
                      double* sums2_or_null);
/* foto_bb_flow into device memory `out` of dtype FOTO_F32 | FOTO_F64: layout 0 is planar
 * [3][Ny][Nx] = u, v, m; layout 1 is interleaved [Ny][Nx][2] = (u, v), the payload
 * utils.saveFlo (utils.py:273-292) writes after its 12-byte header.  (float)x rounds to nearest
 * even, as np.float32(x).  Same callback and in-flight rules as foto_bb_flow.            */
int foto_bb_flow_dev(foto_bb_ctx* c, void* out, int dtype, int layout, void* stream);

/* The transport path: what only a dynamic-OT solver has between its two frames.  Host and device
 * twins, with the rules of foto_bb_flow / foto_bb_get_state and of foto_bb_flow_dev: the data is
 * that of the last COMPLETED outer iteration (from the callback of the default single-GPU loop:
 * the iteration it reports; from the one-in-flight loop's callback FOTO_ERR_STATE); a context
 * that a failed iterate left inconsistent, and an RCCL context, return FOTO_ERR_STATE;
 * virtual_ranks > 1 works (planes and steps come from the in-process shard that owns them).
 * None of them allocates, and none changes anything the next foto_bb_iterate reads.
 *
 * Density frames: rho at plane positions s[k] (a HOST array) in [0, Nt-1]:
 * n = min((int)s, Nt-2), w = s - n, value = scale * ((1 - w) * rho_n + w * rho_{n+1}), rho_n =
 * plane n of mu's density part -- mu[n*Nx*Ny:(n+1)*Nx*Ny], the planes the commented-out export of
 * benamou_brenier.py:262-267 saved as rhon[n] -- of the last completed outer iteration (before any
 * iteration: the initial path of benamou_brenier.py:193-194).  The multiply by scale comes last,
 * so an integer s with scale == 1 reproduces plane n bit for bit; scale undoes normalize = 1 when
 * it is the frame sum from sums2.  out: [count][Ny][Nx], C-contiguous.  F32 is (float)x (to
 * nearest even, np.float32); U8 is (uint8)(255 * clip(x, 0, 1) + 0.5), NaN -> 0: to nearest, unlike
 * the truncating np.uint8(255 * np.clip(...)) of main.py:142, so that a u8 frame survives ingest
 * and export (255 * (49 / 255.0) is 48.99999999999999).  FOTO_ERR_ARG: null pointers, count <= 0,
 * an s[k] outside [0, Nt-1] or not finite, a scale not finite or <= 0, a dtype outside 0..2, an
 * `out` that is not device memory of the context's device (checked before anything is enqueued;
 * `out` is then untouched).  One kernel launch per 128 frames.                               */
int foto_bb_frames(foto_bb_ctx* c, const double* s, int count, double scale, double* out);          /* host f64 */
int foto_bb_frames_dev(foto_bb_ctx* c, const double* s, int count, double scale, void* out, int dtype,
                       void* stream);
/* Flow path: record n-1 (n = 1..Nt-1) = (u_n, v_n, m_n): the displacement after the first n steps
 * of utils.reconstructTrajectory (utils.py:63-97) and m_n = -div('D')[u_n; v_n] (utils.py:181),
 * i.e. utils.opticalflow_from_benamoubrenier(phi[: (n+1)*Nx*Ny], n+1, Nx, Ny, ...) (utils.py:148-183).
 * Record Nt-2 is foto_bb_flow's result, bit for bit.  Host: u, v, m each [Nt-1][Ny*Nx].  Device:
 * `out` holds Nt-1 consecutive records, each laid out as foto_bb_flow_dev lays out its one --
 * layout 0: [Nt-1][3][Ny][Nx], layout 1: [Nt-1][Ny][Nx][2]; dtype FOTO_F32 | FOTO_F64 (m is computed
 * from the float64 u, v).  FOTO_ERR_STATE before any outer iteration has run.               */
int foto_bb_flow_path(foto_bb_ctx* c, double* u, double* v, double* m);
int foto_bb_flow_path_dev(foto_bb_ctx* c, void* out, int dtype, int layout, void* stream);
/* Point tracking, the Lagrangian half of the flow path: utils.reconstructTrajectory(xStart, yStart,
 * un, vn, Nx, Ny, Nt) (utils.py:44-99) for M arbitrary start points instead of the pixel centres.
 * pts[M][2] = (x, y) in the reference's pixel-index coordinates (pixel (i, j) has centre (x, y) =
 * (i, j), x along Nx); sub-pixel values and values outside the frame are allowed (the reference
 * clamps the cell and extrapolates, utils.py:63-97).  Positions are carried in float64 through all
 * steps whatever the dtypes.  Record n-1 (n = 1..Nt-1) is the displacement (x_n - xStart, y_n -
 * yStart) = reconstructTrajectory(xStart, yStart, un[:n+1], vn[:n+1], Nx, Ny, n+1) (utils.py:44-99),
 * with un, vn = grad('N') of phi's planes (utils.py:148-183).  out: [R][M][2], C-contiguous, R = Nt-1
 * with all_steps = 1, R = 1 (the last record) with all_steps = 0.  For start points at pixel centres
 * record n-1 carries the bits of foto_bb_flow_path's (u, v) at that pixel, the last record those of
 * foto_bb_flow.  Deviation: a non-finite coordinate gives a non-finite record for that point alone
 * (the reference's int(nan) / int(inf) at utils.py:63-64 raise); it is neither an error nor an
 * out-of-range read.  State rules: those of foto_bb_flow_path.  Host entry (utils.py:44-99): float64
 * in and out, staged through grow-only device buffers of the context.  Device entry (utils.py:44-99):
 * pts_dtype and dtype FOTO_F32 | FOTO_F64 (float32 points widen exactly; float32 records are
 * (float)x, to nearest even); both pointers are checked to be device memory of the context's
 * device, aligned to one (x, y) pair, before anything is enqueued; one launch and no allocation on
 * a one-shard context (virtual_ranks > 1: one launch per shard, the float64 positions in between in
 * a grow-only scratch of the context).  FOTO_ERR_ARG, with `out` untouched: a null pointer, M < 1 or
 * > 2^31 - 1, all_steps not 0 / 1, a dtype outside {F32, F64}, a misaligned or non-device pointer. */
int foto_bb_track(foto_bb_ctx* c, const double* pts, int64_t M, int all_steps, double* out);          /* host f64 */
int foto_bb_track_dev(foto_bb_ctx* c, const void* pts, int pts_dtype, int64_t M, int all_steps, void* out,
                      int dtype, void* stream);

/* Maps and in-betweens: the transport read from an arbitrary time s in [0, Nt-1], in BOTH
 * directions -- which pixel of frame 1 came from where in frame 0, and the caller's own frames
 * (colour, masks, depth: anything defined on them) half-way.  No reference counterpart: utils.py
 * reads the transport from frame 0 forward only (utils.py:44-99).
 *
 * Definitions.  Pixel (i, j) has centre p = (x, y) = (i, j).  V_n(z), n = 0..Nt-2, is plane n's
 * interpolated velocity at z: exactly the pair of sums one step of utils.reconstructTrajectory
 * (utils.py:63-97) adds to (x, y) -- the truncated, clamped cell, the weights w1..w4, the grad('N')
 * taps with their zeroed border columns and rows, the sum order w1 u00 + w2 u01 + w3 u11 + w4 u10.
 *   forward step    F_n(z) = z + V_n(z)                    (the step of foto_bb_flow / _track)
 *   inverse step    inv(n, theta, p), theta in (0, 1]: z <- p, then z <- p - theta V_n(z) exactly
 *                   inv_iters times.  A fixed count, no convergence test: deterministic, and exact
 *                   to the contraction rate of theta V_n per round (DESIGN.md has measured rates).
 *                   Where theta V_n is no contraction (a velocity that changes by a pixel or more
 *                   per pixel) the rounds diverge and, the cell extrapolating bilinearly outside
 *                   the frame, may overflow: such records are non-finite, never an out-of-range read.
 *   maps at s       n = (int)s, theta = s - n (theta > 0 implies n <= Nt-2);
 *                   p_n = theta > 0 ? inv(n, theta, p) : p;
 *                   b = p_n pushed forward through the steps n, n+1, .., Nt-2 (none for n = Nt-1);
 *                   a = p_n pulled back: a <- inv(m, 1, a) for m = n-1, .., 0;
 *                   record (4 planes) = (a_x - x, a_y - y, b_x - x, b_y - y).
 * Positions are float64 throughout.  At s = 0 the a-planes are +0.0 and the b-planes are
 * foto_bb_flow's (u, v), bit for bit; at s = Nt-1 the b-planes are +0.0 and -a is the backward
 * flow, frame 1 -> frame 0, without a second solve.
 *   in-between      w_t = s / (Nt-1); per channel c:
 *                   I_s(p) = (1 - w_t) S(I0_c; a) + w_t S(I1_c; b),
 *                   S the clamped bilinear sample of the coarse-to-fine GN section below (a NaN
 *                   coordinate gives NaN, read from in-frame taps), frame values = pixel / divisor.
 *                   Output: FOTO_F64 x; FOTO_F32 (float)x; FOTO_U8 (uint8)(255 clip(x, 0, 1) + 0.5),
 *                   NaN -> 0 -- foto_bb_frames' to-nearest rule, not the renderer's truncation, so
 *                   that s = 0 and s = Nt-1 give a u8 frame back unchanged.  Both end frames come
 *                   back bit for bit (finite frames).  The weights and taps of a and b are computed
 *                   once per pixel and time and reused for every channel.
 * s is a HOST array of `count` positions; inv_iters in [1, FOTO_INV_ITERS_MAX].  One launch per 128
 * times, one thread per (pixel, time).  State rules, stream contract and pointer checks: those of
 * foto_bb_flow_path[_dev] and foto_bb_frames_dev -- the last COMPLETED outer iteration's phi (from
 * the default loop's callback: the iteration it reports; from the one-in-flight loop's callback
 * FOTO_ERR_STATE); FOTO_ERR_STATE before any outer iteration, on an RCCL or a broken context;
 * virtual_ranks > 1 works (a table of Nt plane pointers, built per call in a grow-only scratch of
 * the context, finds each plane in the shard that owns it).  Nothing the next foto_bb_iterate
 * reads is changed.
 *   foto_bb_maps       host float64 out[count][4][Ny][Nx], staged through a grow-only scratch.
 *   foto_bb_maps_dev   device out[count][4][Ny][Nx] of FOTO_F32 | FOTO_F64 ((float)x, to nearest even).
 *   foto_bb_interp_dev f0 / f1 describe channel 0 of the two device frames (w = Nx, h = Ny); channel
 *                      c starts c * stride_c0 / stride_c1 ELEMENTS further on, as in
 *                      foto_render_warp_dev; out[count][Ny][Nx][channels] of out_dtype, which must
 *                      not overlap a frame.
 * FOTO_ERR_ARG, with `out` untouched and nothing enqueued: a null pointer, count < 1, an s[k] outside
 * [0, Nt-1] or not finite, inv_iters outside [1, FOTO_INV_ITERS_MAX], a dtype outside {F32, F64}
 * (maps) or 0..2 (in-betweens), channels < 1, a stride_c <= 0, anything foto_image_check rejects for
 * any channel, an `out` not aligned to its element, a pointer that is not device memory of the
 * context's device, an `out` that overlaps a frame.                                               */
#define FOTO_INV_ITERS_MAX 64
#define FOTO_INV_ITERS_DEFAULT 6
int foto_bb_maps(foto_bb_ctx* c, const double* s, int count, int inv_iters, double* out);          /* host f64 */
int foto_bb_maps_dev(foto_bb_ctx* c, const double* s, int count, int inv_iters, void* out, int dtype, void* stream);
int foto_bb_interp_dev(foto_bb_ctx* c, const foto_image* f0, const foto_image* f1, int channels, int64_t stride_c0,
                       int64_t stride_c1, const double* s, int count, int inv_iters, void* out, int out_dtype,
                       void* stream);

/* Transport report: how good the transport behind the exports above is, and what it costs -- per
 * time plane n = 0..Nt-1 the sums, over the plane's Nx*Ny voxels, of FOTO_REPORT_COLS terms of the
 * last completed outer iteration's mu = (rho, m1, m2) and g = (g_t, g_x, g_y) = grad_st phi
 * (operators.py:114-127), h = dt = 1.  out: C-contiguous double[Nt][FOTO_REPORT_COLS].  Per voxel,
 * in exactly this operation order (every term is bit-identical to its numpy restatement; only the
 * sums are taken in another -- fixed -- order):
 *   MASS    rho                                   np.sum(rhon[n,:]), benamou_brenier.py:266
 *   KINETIC rho > 0 ? (m1*m1 + m2*m2) / (rho + rho) : 0       the action density |m|^2 / (2 rho)
 *   VACUUM  rho > 0 ? 0 : (m1*m1 + m2*m2)         momentum left where the clamp of :232 emptied
 *                                                 the density (a NaN rho lands here, and in MASS)
 *   CONT    c*c, c = row k of div_st @ mu (operators.py:129-142, COO order t, x, y), then
 *           c -= (rho0 - rho) on plane 0 and c += (rhoT - rho) on plane Nt-1: the F of
 *           solve_benamou_brenier_step (benamou_brenier.py:64-82) with q = 0, the bits of
 *           foto_bb_rhs(mu, 0, ...) -- the continuity equation and the two boundary frames
 *   HJ_NUM  rho * fabs(g_t + 0.5 * (g_x*g_x + g_y*g_y))       benamou_brenier.py:246-247
 *   HJ_DEN  rho * (g_x*g_x + g_y*g_y)                         benamou_brenier.py:248
 *   DUAL    plane 0: -(phi * rho0); plane Nt-1: phi * rhoT; other planes: 0
 *   DIST_T  (rho - rhoT) * (rho - rhoT)           utils.IE(Nx, Ny, rhoT, rhon[n]) of :265 is
 *                                                 255 * sqrt(DIST_T / (Nx*Ny))
 * sqrt(sum_n HJ_NUM / (sum_n HJ_DEN + 1e-10)) is the crit of that iteration (:249), up to
 * summation order.  sum_n DUAL = sum phi_{Nt-1} rhoT - sum phi_0 rho0 is the dual estimate of the
 * action that the trapezoid of KINETIC over n estimates primally; the two agree only at
 * convergence and for equal masses of rho0 and rhoT -- neither is the other's check.
 * One kernel launch per in-process shard, one read of the four fields; a plane's eight sums are
 * reduced in an order that depends on (Nx, Ny) alone -- the same bits for any virtual_ranks, from
 * call to call, and a function of that plane's data and its t-neighbours only.  State rules: those
 * of foto_bb_flow_path (FOTO_ERR_STATE before any outer iteration, from the one-in-flight loop's
 * callback, on an RCCL or a broken context).  Neither entry changes statistics or anything a later
 * foto_bb_iterate reads; the scratch is a grow-only buffer of the context, made on first use.
 * Host entry: one device-to-host copy of Nt * 64 bytes.  Device entry: the stream contract of the
 * device-buffer section; `out` is checked to be 8-byte-aligned device memory of the context's
 * device before anything is enqueued (FOTO_ERR_ARG, `out` untouched); the kernels write `out`
 * directly, without a host synchronisation.  FOTO_ERR_ARG: a null pointer.                       */
#define FOTO_REPORT_COLS 8
#define FOTO_REPORT_MASS 0
#define FOTO_REPORT_KINETIC 1
#define FOTO_REPORT_VACUUM 2
#define FOTO_REPORT_CONT 3
#define FOTO_REPORT_HJ_NUM 4
#define FOTO_REPORT_HJ_DEN 5
#define FOTO_REPORT_DUAL 6
#define FOTO_REPORT_DIST_T 7
int foto_bb_report(foto_bb_ctx* c, double* out);                          /* host [Nt][8]   */
int foto_bb_report_dev(foto_bb_ctx* c, double* out, void* stream);        /* device [Nt][8] */
/* Test entry, no context: the same kernel on one shard from host arrays (mu3 = [rho; m1; m2], each
 * Nt*Nx*Ny; phi; rho0, rhoT: Nx*Ny) -- benamou_brenier.py:64-82, 246-248, 262-267 as above.
 * FOTO_ERR_ARG before any device is touched: a null pointer, Nt < 2, Nx < 1 or Ny < 1.           */
int foto_report_from_state(const double* mu3, const double* phi, const double* rho0, const double* rhoT, int Nt,
                           int Nx, int Ny, double* out);

/* foto_gn_plan_solve (classical.py:68-130) on device frames, the solution exported to `out` as
 * foto_bb_flow_dev does (planar: u, v, m).  Same PCG launches, prediction, result and return
 * codes as foto_gn_plan_solve; it neither makes nor touches the plan's pinned host staging.  */
int foto_gn_plan_solve_dev(foto_gn_plan* p, const foto_image* f1, const foto_image* f2, void* out, int dtype,
                           int layout, void* stream, int* iterations);

/* ------------------------------------------------------------------ coarse-to-fine GN
 * The GN brightness equation fx u + fy v + ft - f2 m = 0 is a linearisation: it holds for
 * displacements of about a pixel and returns too short a flow for larger ones.  The pyramid
 * solves on an image pyramid and, per level, warps the second frame by the flow found so far and
 * re-solves for the increment, regularising the TOTAL flow (DESIGN.md has the algorithm):
 *   level sizes   (w_0, h_0) = (w, h); level l + 1 exists while l + 1 < levels and
 *                 min(w_l, h_l) >= 2 min_size, with w_{l+1} = ceil(w_l / 2), h likewise;
 *   restrict      c[j][i] = 0.25 (((f[J0][I0] + f[J0][I1]) + f[J1][I0]) + f[J1][I1]), I0 = 2 i,
 *                 I1 = min(2 i + 1, w - 1), J likewise;
 *   sample        S(f; x, y): bilinear, x clamped to [0, w - 1], i0 = min(floor(x), w - 2); a NaN
 *                 coordinate gives NaN, read from in-frame taps (foto_warp's rule);
 *   prolong       P(c)[j][i] = S(c; (i + 1/2) wc / w - 1/2, (j + 1/2) hc / h - 1/2), then
 *                 u <- (w / wc) P(u), v <- (h / hc) P(v), m <- P(m);
 *   warp          g[j][i] = (1 - m[j][i]) S(f2_l; i + u[j][i], j + v[j][i]);
 *   increment     A(f1_l, g) d = b(f1_l, g) - [alpha N u; alpha N v; lambda N m] with A, b of
 *                 foto_gn_apply / foto_gn_rhs and N = -Lambda2 the operator's Laplacian part; then
 *                 (u, v, m) += d;
 *   loop          coarsest level to level 0, `warps` increment solves per level; the very first
 *                 solve has no prior (g = f2_l, b untouched), so levels = 1, warps = 1 is
 *                 foto_gn_plan_solve, bit for bit.
 * The flow is the reference's: f1(x) ~ (1 - m) f2(x + u); that foto_warp / foto_render_warp_dev
 * draw it as ((1 + m) f1)(x - u) ~ f2 is a first-order identification.                        */
#define FOTO_GN_PYR_MAX_LEVELS 16
/* Host only (no HIP call): the level sizes, finest first, into wl / hl (cap entries each) and
 * their count into *n.  FOTO_ERR_ARG: a null pointer, w or h < 2, levels < 1, min_size < 2,
 * cap smaller than the count.                                                              */
int foto_gn_pyr_sizes(int w, int h, int levels, int min_size, int* wl, int* hl, int cap, int* n);

typedef struct {
    int levels;      /* levels asked for (the sizes rule may build fewer)            default 4 */
    int warps;       /* increment solves per level                                   default 3 */
    int min_size;    /* a level is halved only while both extents are >= 2 min_size  default 16 */
    double rtol;     /* every solve's PCG relative residual                      default 1e-10 */
    int maxiter;     /* every solve's PCG cap                                   default 200000 */
} foto_gn_pyr_opts;
int foto_gn_pyr_opts_default(foto_gn_pyr_opts* o);

/* Report of one pyramid solve.  The caller sizes its / info (cap entries each, either may be
 * NULL); solves are listed in the order run, coarsest level first.                          */
typedef struct {
    int cap;                  /* in: entries of its / info                                    */
    int* its;                 /* per solve: PCG iterations                                    */
    int* info;                /* per solve: 0 converged, maxiter otherwise                    */
    int levels;               /* levels built                                                 */
    int solves;               /* solves run = levels * warps                                  */
    int wl[FOTO_GN_PYR_MAX_LEVELS], hl[FOTO_GN_PYR_MAX_LEVELS];   /* level sizes, finest first */
    double ms_level[FOTO_GN_PYR_MAX_LEVELS];   /* device time per level (index = level; the
                                 coarsest level's includes the ingest and the restrictions)   */
    double ms_new;            /* device time of the pyramid's own steps between the solves: the
                                 restrictions, prolongations, warps and flow copies (event pairs
                                 around them); the prior term and the add-back run inside a solve */
    double ms_total;          /* host wall time of the call                                   */
} foto_gn_pyr_stats;

/* One plan per level on one stream, the level images and the flow buffers, made once.
 * FOTO_ERR_ARG (nothing made, nothing enqueued): a null pointer, w or h < 2, alpha or lambda
 * <= 0, levels < 1, warps < 1, min_size < 2, maxiter < 0.  opts NULL: the defaults.          */
typedef struct foto_gn_pyr foto_gn_pyr;
int foto_gn_pyr_create(int w, int h, double alpha, double lambda_, const foto_gn_pyr_opts* opts, foto_gn_pyr** out);
void foto_gn_pyr_destroy(foto_gn_pyr* p);
int foto_gn_pyr_device(const foto_gn_pyr* p);
/* Host float64 frames in, u, v, m out (w * h each).  Returns 0, or the number of solves that hit
 * maxiter, < 0 on error.  stats may be NULL.                                                */
int foto_gn_pyr_solve(foto_gn_pyr* p, const double* f1, const double* f2, double* u, double* v, double* m,
                      foto_gn_pyr_stats* stats);
/* The same on device frames, exported like foto_gn_plan_solve_dev (same checks, same stream
 * contract): `out` is a buffer foto_flow describes.  With stats the call waits for the last
 * level's event to read the times.                                                          */
int foto_gn_pyr_solve_dev(foto_gn_pyr* p, const foto_image* f1, const foto_image* f2, void* out, int dtype,
                          int layout, void* stream, foto_gn_pyr_stats* stats);

/* The pyramid's pieces on host arrays (tests).  foto_pyr_down: both frames of a w x h level to
 * ceil(w/2) x ceil(h/2) in one launch (w, h >= 1).  foto_pyr_up: u, v, m from wc x hc to w x h
 * with the scales above (all extents >= 2).  foto_gn_warp_prior: g from f2 and a prior (w, h >=
 * 2).  foto_gn_solve_prior: one increment solve of A(f1, g) with the prior (u0, v0, m0) -- all
 * three NULL: no prior, foto_gn_plan_solve -- returning the total flow; 0 or maxiter.        */
int foto_pyr_down(const double* f1, const double* f2, int w, int h, double* c1, double* c2);
int foto_pyr_up(const double* u, const double* v, const double* m, int wc, int hc, int w, int h, double* uo,
                double* vo, double* mo);
int foto_gn_warp_prior(const double* f2, const double* u, const double* v, const double* m, int w, int h, double* g);
int foto_gn_solve_prior(const double* f1, const double* g, int w, int h, double alpha, double lambda_, double rtol,
                        int maxiter, const double* u0, const double* v0, const double* m0, double* u, double* v,
                        double* m, int* iterations);

/* ------------------------------------------------------------------------- TV-L1 flow
 * Duality-based TV-L1 optical flow (Zach, Pock & Bischof 2007) with the illumination channel of
 * Chambolle & Pock 2011: the classical baseline that keeps motion boundaries sharp, where GN's
 * quadratic prior smears them.  Pointwise arithmetic plus a 3-point stencil, no linear solve, and
 * every count fixed: the result is a function of the frames and the options alone.  Float64.
 * The flow convention is the pyramid's, f1(x) ~ (1 - m) f2(x + u).  Unknowns per pixel
 * U = (u, v, w); the reported luminosity is m = gamma w.
 *   pyramid     the sizes of foto_gn_pyr_sizes, the restriction, S and the prolongation above;
 *               coarsest level first, from U = 0; every other level from the prolonged (u, v, w),
 *               u and v scaled by the size ratio, w unscaled; the dual variables P (two per
 *               channel) start at zero on every level and are kept across the warps of a level;
 *   per warp    at the current U0: g = S(f2; x + u0, y + v0), a1 = S(Gx f2; .), a2 = S(Gy f2; .)
 *               at the same positions, a3 = -gamma g, n2 = (a1^2 + a2^2) + a3^2,
 *               rc = ((g - f1) - a1 u0) - a2 v0; Gx f [j][i] = 0.5 (f[j][i+1] - f[j][i-1]), zero
 *               in the first and last column, Gy likewise in y;
 *   per inner   rho = ((rc + a1 u) + a2 v) + a3 w, from all three channels before any changes;
 *   iteration   k = lambda theta where rho < -lambda theta n2, -lambda theta where
 *               rho > lambda theta n2, elsewhere -rho / n2 if n2 > 1e-12, else 0; then for each
 *               channel d: U_d <- (U_d + k a_d) + theta div(P_d); (dx, dy) = fwd(U_d);
 *               P_d <- (P_d + (tau / theta) (dx, dy)) / (1 + (tau / theta) sqrt(dx^2 + dy^2));
 *   fwd, div    fwd: the forward difference, zero in the last column / row; div = minus its
 *               adjoint: px[0] in the first column, px[i] - px[i-1] inside, -px[w-2] in the last
 *               one, the same in y, x part + y part.
 * lambda is for frames in [0, 1] (the paper's 0.15 is for [0, 255]).  gamma = 0 switches the
 * illumination channel off and leaves w, and so m, exactly zero.                              */
typedef struct {
    double lambda;   /* data weight                                                   default 38 */
    double theta;    /* coupling of the flow and its auxiliary                       default 0.3 */
    double tau;      /* dual step                                                   default 0.25 */
    double gamma;    /* illumination coupling; 0: the channel is off                 default 0.1 */
    int levels;      /* levels asked for (the sizes rule may build fewer)              default 4 */
    int warps;       /* linearisations per level                                       default 5 */
    int iters;       /* inner iterations per warp                                     default 30 */
    int min_size;    /* as foto_gn_pyr_opts                                           default 16 */
    int per_launch;  /* inner iterations per kernel launch, 1 .. FOTO_TVL1_MAX_PER_LAUNCH: 1 is
                        one launch per iteration on global memory, more is that many iterations on
                        LDS tiles with a halo of as many pixels; the result has the same bits for
                        every value (DESIGN.md has the measurements)                   default 5 */
} foto_tvl1_opts;
#define FOTO_TVL1_MAX_PER_LAUNCH 8
int foto_tvl1_opts_default(foto_tvl1_opts* o);

/* Report of one solve.  The caller sizes wl / hl / launches / ms_level (cap entries each, any may
 * be NULL; index = level, finest first).                                                       */
typedef struct {
    int cap;                  /* in: entries of the four arrays                                */
    int* wl;                  /* level sizes                                                   */
    int* hl;
    int* launches;            /* kernels launched on the level: its prolongation, `warps`
                                 coefficient launches, warps * ceil(iters / per_launch)
                                 iteration launches                                            */
    double* ms_level;         /* device time per level (the coarsest level's includes the ingest
                                 and the restrictions)                                         */
    int levels;               /* levels built                                                  */
    int launches_total;       /* the sum of `launches` over all levels                          */
    double ms_total;          /* host wall time of the call                                    */
} foto_tvl1_stats;

/* The level frames, two copies of U and P and the coefficients, one stream, made once.
 * FOTO_ERR_ARG (nothing made, nothing enqueued): a null pointer, w or h < 2, theta or tau not
 * positive and finite, lambda or gamma negative or not finite, levels, warps or iters < 1,
 * min_size < 2, per_launch outside 1 .. FOTO_TVL1_MAX_PER_LAUNCH.  opts NULL: the defaults.    */
typedef struct foto_tvl1 foto_tvl1;
int foto_tvl1_create(int w, int h, const foto_tvl1_opts* opts, foto_tvl1** out);
void foto_tvl1_destroy(foto_tvl1* p);
int foto_tvl1_device(const foto_tvl1* p);
/* Host float64 frames in, u, v, m out (w * h each).  Returns 0, < 0 on error.  stats may be NULL. */
int foto_tvl1_solve(foto_tvl1* p, const double* f1, const double* f2, double* u, double* v, double* m,
                    foto_tvl1_stats* stats);
/* The same on device frames, exported like foto_gn_pyr_solve_dev (same checks, same stream
 * contract): `out` is a buffer foto_flow describes; its float64 values are foto_tvl1_solve's bit
 * for bit.  With stats the call waits for the last level's event to read the times.            */
int foto_tvl1_solve_dev(foto_tvl1* p, const foto_image* f1, const foto_image* f2, void* out, int dtype, int layout,
                        void* stream, foto_tvl1_stats* stats);

/* The solver's two kernels on host arrays (tests; w, h >= 2).  foto_tvl1_coeffs: one warp's
 * out5 = [5][w h] = a1, a2, a3, n2, rc from the frames and U0 = (u, v).  foto_tvl1_iterate:
 * n >= 1 inner iterations on coef5 = [5][w h] as above, U3 = [3][w h] = u, v, w and
 * P6 = [6][w h] = (px, py) of u, of v, of w, both updated in place, at most per_launch
 * (1 .. FOTO_TVL1_MAX_PER_LAUNCH) of them in one kernel launch.                               */
int foto_tvl1_coeffs(const double* f1, const double* f2, const double* u, const double* v, int w, int h,
                     double gamma, double* out5);
int foto_tvl1_iterate(const double* coef5, double* U3, double* P6, int w, int h, double lambda, double theta,
                      double tau, int n, int per_launch);

/* foto_warp / foto_flow_errors / foto_intensity_error (utils.py:186-248, 294-354) on contiguous
 * float64 DEVICE arrays of w * h elements: the same kernels and reduction order without the
 * uploads.  `out` of the warp is a device array (not aliasing an input); the metrics return
 * host scalars (the call waits for them).                                                 */
int foto_warp_dev(const double* f1, const double* u, const double* v, const double* m, int w, int h, double* out,
                  void* stream);
int foto_flow_errors_dev(const double* u, const double* v, const double* uGT, const double* vGT, int w, int h,
                         double* out4, void* stream);
int foto_intensity_error_dev(const double* I, const double* IGT, int w, int h, double* ie, void* stream);

/* Device memory of the current device for callers without another GPU library (the ctypes
 * binding, the tests): hipMalloc / hipFree / a blocking hipMemcpy on the null stream.
 * kind: 0 host -> device, 1 device -> host, 2 device -> device.                          */
int foto_dev_malloc(size_t bytes, void** out);
int foto_dev_free(void* p);
int foto_dev_memcpy(void* dst, const void* src, size_t bytes, int kind);

/* ------------------------------------------------------------------ rendering
 * The last stage of a device pipeline: what main.py:107-146 and run.sh:104,115 do with a flow --
 * the clipped 8-bit reconstruction, the luminosity map, the colour code -- on the flow buffers
 * the *_dev entries above write, for one or many records at once, without leaving HBM.  Additive.
 * Every entry obeys the stream contract of the device-buffer section, unchanged; every device
 * pointer is checked for the CURRENT device before anything is enqueued; an argument error leaves
 * `out` untouched.  None of them synchronises with the host.
 *
 * FOTO_ERR_ARG before any device call: a null pointer, w or h < 1, channels < 1, stride_c <= 0,
 * anything foto_image_check rejects for any channel, a flow dtype outside {F32, F64}, a layout
 * outside {0, 1}, records < 1, flow data not aligned to its element, use_m = 1 or the luminosity
 * with layout 1 (it carries no m), an out_dtype outside 0..2, a non-finite maxmotion, a misaligned
 * out / maxrad.  FOTO_ERR_ARG after the pointer queries: a pointer that is not device memory of the
 * current device, an `out` (or maxrad) whose byte range overlaps the frame or the flow (the warp
 * gathers, as in foto_warp_dev).  All index arithmetic is int64_t: records * h * w * channels may
 * pass 2^31.                                                                                  */
/* A flow buffer exactly as foto_bb_flow_dev / foto_bb_flow_path_dev / foto_gn_plan_solve_dev
 * write it (utils.saveFlo's payload, utils.py:273-292, for layout 1)                          */
typedef struct {
    const void* data;   /* DEVICE pointer                                                      */
    int dtype;          /* FOTO_F32 | FOTO_F64                                                  */
    int layout;         /* 0: [records][3][h][w] = u, v, m;  1: [records][h][w][2] = (u, v)     */
    int records;        /* >= 1                                                                */
} foto_flow;

/* Host-only validation of a flow descriptor for w x h records (no HIP call): the flow rules of
 * the list above.  Every entry below calls it first (utils.openFlo, utils.py:250-271, checks only
 * the file's magic number).                                                                   */
int foto_flow_check(const foto_flow* fl, int w, int h);

/* main.py:109-110,142 on utils.apply_opticalflow (utils.py:186-248): for record k, channel c,
 *   x = clip(apply_opticalflow(src_c / divisor, u_k, v_k, w, h, m_k), 0, 1).
 * `src` describes channel 0; channel c starts c * stride_c ELEMENTS further on (interleaved HWC:
 * stride_x = C, stride_c = 1; planar CHW: stride_c = the plane pitch; row-padded and transposed
 * views are strides).  Flow values widen to double exactly and the arithmetic is foto_warp's,
 * operation for operation; the weights and the four clamped taps are computed once per pixel and
 * record and reused for every channel.  use_m = 0 leaves the frame unscaled (foto_warp with m =
 * NULL); use_m = 1 needs layout 0.  out: C-contiguous [records][h][w][channels] of out_dtype:
 * FOTO_U8 is the reference's TRUNCATING np.uint8(255 * x) (main.py:142) -- not the rounding to
 * nearest of foto_bb_frames, which serves another purpose (a u8 frame surviving ingest and
 * export); FOTO_F32 is (float)x; FOTO_F64 is x.  Deviation: a NaN x gives 0 in a uint8 output and
 * stays NaN in a float output (np.clip keeps NaN; np.uint8(nan) is platform-defined); the taps of
 * a pixel with a NaN displacement are pixel (0, 0)'s row / column, never out of range (the
 * reference's int(nan) index raises).  One launch for all records and channels.               */
int foto_render_warp_dev(const foto_image* src, int channels, int64_t stride_c, const foto_flow* fl, int use_m,
                         int w, int h, void* out, int out_dtype, void* stream);
/* main.py:146: out = uint8 [records][h][w] = np.uint8(255 * np.clip((m + 1) / 2, 0, 1)), truncating,
 * NaN -> 0.  Needs layout 0.                                                                  */
int foto_render_lum_dev(const foto_flow* fl, int w, int h, void* out, void* stream);
/* run.sh:104,115 (the prebuilt bin/color_flow), by the algorithm bin/color_flow.py:23-63 restates:
 * out = uint8 [records][h][w][3], RGB.  Unknown flow (|u| > 1e9, |v| > 1e9 or NaN) is black; rad =
 * sqrt(u u + v v); maxrad = the maximum of rad over the known pixels of the record, replaced by
 * maxmotion when maxmotion > 0, and 1 when it is <= 0; fx, fy = u, v / maxrad; the 55-entry wheel;
 * hue from atan2(-fy, -fx) / pi; k0 = (int)fk, k1 = (k0 + 1) % 55, f = fk - k0; col = (1 - f) col0 +
 * f col1; r <= 1 ? 1 - r (1 - col) : 0.75 col; (int)(255 col).  The arithmetic is FLOAT64 on the
 * widened flow, in flow_to_color's order -- not the tool's float32: everything in this library is
 * float64, and the image then depends on the device's atan2 at the last-ulp level only (sqrt and
 * the divisions are correctly rounded).  Against the float32 tool, measured on the CPU with numpy
 * on a 37x29 and a 64x48 random flow: maxmotion = 0 gave the same image from the float32 and the
 * float64 restatement; maxmotion = 2 differed by one level on 1 sample of 3219 and 1 of 9216.
 * The maximum is order-independent, hence deterministic: a block reduction, then one vector atomic
 * max per block on the bit pattern of the non-negative double.  maxrad_or_null: a DEVICE
 * double[records] that receives the value actually used; NULL: a grow-only per-device scratch of
 * the library holds it.                                                                       */
int foto_render_color_dev(const foto_flow* fl, int w, int h, double maxmotion, void* out, double* maxrad_or_null,
                          void* stream);

/* ------------------------------------------------------------------ scoring
 * The evaluation stage on the buffers the entries above leave in HBM: utils.EE / AE / IE
 * (utils.py:294-354) for every record of a flow buffer at once, with the robustness measures R(t),
 * the accuracy percentiles A(p) and the normalised interpolation error NE of the Middlebury
 * evaluation (Baker et al. 2011).  Additive: foto_flow_errors / foto_intensity_error are unchanged.
 * The *_dev entries obey the stream contract of the device-buffer section and never synchronise
 * with the host (but for a library scratch that has to grow); every device pointer is checked for
 * the CURRENT device before anything is enqueued; an argument error leaves the outputs untouched.
 *
 * Definitions.  Values widen to double exactly; per pixel, in foto_flow_errors' operations,
 *   EE = sqrt((u - uGT)^2 + (v - vGT)^2),
 *   AE = acos((1 + u uGT + v vGT) / (sqrt(1 + u^2 + v^2) sqrt(1 + uGT^2 + vGT^2)))   (radians).
 * A pixel is VALID if the mask (when given) is non-zero there and the ground truth is known:
 * |uGT| <= 1e9, |vGT| <= 1e9 and neither is NaN (foto_render_color_dev's rule).  EE is KEPT where
 * the pixel is valid and EE <= ee_cap (the reference's 50: a NaN EE drops out); AE is kept where
 * the pixel is valid and AE is not NaN.  Deviation: on unknown-flow pixels the reference's AE keeps
 * a finite, meaningless value; here they are not valid.  With no unknown pixel and no mask the
 * means and standard deviations are the reference's.
 *   R(t) = the fraction of the kept errors strictly above t.
 *   A(p) = the k-th smallest kept error, k = max(1, ceil(p n / 100)) evaluated in float64 on the
 *          device (n is known only there): an order statistic, an actual sample, found exactly by
 *          a radix select on the bit pattern of the non-negative double.
 * Table row of a record, FOTO_SCORE_COLS doubles:
 *    0 n_valid   1 n_EE   2 EE mean   3 EE standard deviation (population)   4 EE max
 *    5-8 R(ee_thr[i])   9-12 A(pct[j]) of EE
 *   13 n_AE   14 AE mean   15 AE standard deviation   16 AE max
 *   17-20 R(ae_thr[i])   21-24 A(pct[j]) of AE   25-31 zero.
 * Unused R and A slots are NaN; with n = 0 every statistic of that quantity is NaN.  Sums are
 * fixed-order reductions, counts and order statistics integer work: the same call gives the same
 * bits.                                                                                        */
#define FOTO_SCORE_COLS 32
#define FOTO_SCORE_MAX_RECORDS 65535
typedef struct {
    double ee_cap;        /* EE above it is not kept; > 0 or +inf; default 50                  */
    int n_ee_thr;         /* 0..4 thresholds of R for EE; default 3: 0.5, 1, 2                 */
    int n_ae_thr;         /* 0..4 thresholds of R for AE, radians; default 3: 2.5, 5, 10 degrees */
    int n_pct;            /* 0..4 percentiles of A, for EE and AE alike; default 3: 50, 75, 95  */
    int reserved;         /* 0                                                                 */
    double ee_thr[4];     /* finite, >= 0                                                      */
    double ae_thr[4];     /* finite, >= 0                                                      */
    double pct[4];        /* in (0, 100]                                                       */
} foto_score_opts;
int foto_score_opts_default(foto_score_opts* o);
/* Host-only validation (no HIP call) of everything foto_score_flow / _dev take by descriptor:
 * FOTO_ERR_ARG for a null fl or gt, anything foto_flow_check rejects for either, fl records above
 * FOTO_SCORE_MAX_RECORDS, gt records that are neither 1 nor fl's, anything foto_image_check rejects
 * for the mask, a count outside 0..4, a threshold that is negative or not finite, a percentile
 * outside (0, 100], an ee_cap that is not > 0 (+inf is allowed, NaN is not).                    */
int foto_score_check(const foto_flow* fl, const foto_flow* gt, const foto_image* mask_or_null, int w, int h,
                     const foto_score_opts* opts_or_null);
/* Scores every record of `fl` against `gt`: 1 record, broadcast, or as many as fl (a .flo payload
 * as utils.openFlo reads it is {FOTO_F32, layout 1, 1 record}).  mask: a strided image, non-zero =
 * evaluate.  table: DEVICE double [records][FOTO_SCORE_COLS].  maps_or_null: DEVICE
 * [records][2][h][w] of maps_dtype FOTO_F32 | FOTO_F64 = EE, AE per pixel, NaN where the pixel is
 * not valid.  FOTO_ERR_ARG also for a null table, a misaligned table / maps, a maps_dtype outside
 * {F32, F64}, a pointer that is not device memory of the current device, and an output that
 * overlaps an input or the other output.  Launches: the moments (one read of flow, ground truth and
 * mask: counts, sums, maxima, threshold counts, maps, and the kept errors into a library scratch of
 * 16 bytes per pixel and record), the squared deviations around the device-resident means, and one
 * histogram + one scan launch per digit of the select, all records on a grid axis.               */
int foto_score_flow_dev(const foto_flow* fl, const foto_flow* gt, const foto_image* mask_or_null, int w, int h,
                        const foto_score_opts* opts_or_null, double* table, void* maps_or_null, int maps_dtype,
                        void* stream);
/* The same on HOST arrays behind the same descriptors (table and maps host arrays too): uploaded
 * into the library's scratch, scored by the same launches, downloaded; waits once, at the end.   */
int foto_score_flow(const foto_flow* fl, const foto_flow* gt, const foto_image* mask_or_null, int w, int h,
                    const foto_score_opts* opts_or_null, double* table, void* maps_or_null, int maps_dtype);
/* Scores `count` grey frames against one ground-truth frame: `frames` describes record 0, record k
 * starts k * stride_rec ELEMENTS further on (the output of foto_bb_interp_dev, foto_bb_frames_dev
 * or foto_render_warp_dev); value = (double)pixel / divisor for frames and truth alike.  table4:
 * DEVICE double [count][4] = {n, IE, NE, max |255 I - 255 T|} over the n pixels the mask keeps
 * (all, without one): IE = sqrt(mean(d^2)) (utils.IE), NE = sqrt(mean(d^2 / (gx^2 + gy^2 +
 * ne_eps))), d = 255 I - 255 T, (gx, gy) the gradient of 255 T, central in the interior and
 * one-sided at the border (np.gradient's default; 0 along an axis of length 1).  n = 0: NaN.
 * FOTO_ERR_ARG: a null pointer, count outside 1..FOTO_SCORE_MAX_RECORDS, stride_rec <= 0, anything
 * foto_image_check rejects, an ne_eps that is negative or not finite, a pointer that is not device
 * memory of the current device, a table that overlaps an input.                                 */
int foto_score_frames_dev(const foto_image* frames, int count, int64_t stride_rec, const foto_image* truth,
                          const foto_image* mask_or_null, int w, int h, double ne_eps, double* table4, void* stream);

/* ------------------------------------------------------------------ flow algebra
 * For a caller with K + 1 frames and K pair flows: the composed flow frame 0 -> frame k, the
 * backward flow of a forward flow, and the forward-backward cross-check whose mask is the one
 * foto_score_flow_dev takes (non-zero = evaluate).  Per-pixel gathers on the foto_flow buffers the
 * entries above leave in HBM; nothing in the solvers is involved.  Additive.  The *_dev entries obey
 * the stream contract of the device-buffer section and never synchronise with the host (but for a
 * library scratch that has to grow); every device pointer is checked for the CURRENT device before
 * anything is enqueued; an argument error leaves the outputs untouched.
 *
 * Definitions.  Flow values widen to double exactly and all arithmetic is float64.  Pixel p =
 * (i, j) (column, row) has position (x, y) = (i, j).  S(f; x, y) is the clamped bilinear sample
 * of a w x h field, w, h >= 2: the coordinate is clamped into the frame, a NaN coordinate gives
 * NaN (read from in-frame taps), value = (1 - ay) ((1 - ax) f00 + ax f01) + ay ((1 - ax) f10 +
 * ax f11) on the cell that holds the clamped coordinate (the sample of the coarse-to-fine GN and
 * of the in-betweens).  The cell and the fractions are computed once per position and serve u, v
 * and m.  Flow outputs are FOTO_F32 ((float)x, to nearest even) or FOTO_F64, layout 0 or 1, all
 * index arithmetic int64_t.  The operations are + - * sqrt, comparisons, floor and min / max, so
 * a restatement in the same order gives the same bits.
 *
 * FOTO_ERR_ARG before any device call: anything foto_flow_check rejects for a flow, w or h < 2,
 * backward records that are neither 1 nor the forward flow's, iters outside [1,
 * FOTO_INV_ITERS_MAX], an alpha that is negative or not finite, a dtype outside {F32, F64}, a
 * layout outside {0, 1}, last_only outside {0, 1}, a null or misaligned output (valid and table
 * are required, err is optional).  FOTO_ERR_ARG after the pointer queries: a pointer that is not
 * device memory of the current device, an output that overlaps an input or another output (all
 * three kernels gather: overlap would corrupt the result).                                      */
/* Host-only validation (no HIP call): foto_flow_check of `a` (and of `b`, when given) for w x h
 * records, w, h >= 2, and b's records 1 or a's.                                                  */
int foto_chain_check(const foto_flow* a, const foto_flow* b_or_null, int w, int h);
/* Record k of `fl` is the flow frame k -> frame k + 1, K = fl->records.  The composed flows
 *   C_0(p) = F_0(p),   C_k(p) = C_{k-1}(p) + S(F_k; p + C_{k-1}(p))   (u, then v),
 * one thread per pixel walking the records in order, one launch.  last_only = 0: out holds K
 * records C_0 .. C_{K-1}; 1: one record, C_{K-1}.  The m plane of a layout-0 output: with layout-0
 * input the brightness gains multiply along the path,
 *   M_0 = m_0,   M_k(p) = (1 + M_{k-1}(p)) * (1 + S(m_k; p + C_{k-1}(p))) - 1,
 * which is a definition of this library, not of the reference (which has no sequences): its
 * reconstruction scales a frame by (1 + m) (utils.apply_opticalflow), so gains along a path
 * multiply.  With layout-1 input the m plane is +0.0.  K = 1 copies the input: bit for bit from
 * F64 to F64, NaN payloads included.  A NaN in a record makes NaN exactly the composed values
 * whose path samples it.                                                                         */
int foto_flow_compose_dev(const foto_flow* fl, int w, int h, int last_only, void* out, int out_dtype, int out_layout,
                          void* stream);
/* The backward flow B of every record F of `fl`, F(p + B(p)) + B(p) = 0: B <- 0, then
 * B <- -S(F; p + B) exactly `iters` times (FOTO_INV_ITERS_DEFAULT is the usual choice).  A fixed
 * count and no convergence test, the rule of the inverse step of foto_bb_maps: the result is a
 * function of the inputs alone; it converges where F is a contraction (Jacobian norm L < 1: the
 * residual falls like L^iters), and elsewhere it is still inside every bound above.  One thread
 * per (pixel, record).  The m plane of a layout-0 output is +0.0.                              */
int foto_flow_invert_dev(const foto_flow* fl, int w, int h, int iters, void* out, int out_dtype, int out_layout,
                         void* stream);
/* The forward-backward cross-check of forward records F and backward records B (as many as F, or
 * one for every record).  Per pixel: q = p + F(p), Bq = S(B; q), e = (F_u + Bq_u)^2 + (F_v +
 * Bq_v)^2, and the class is the first that applies of
 *   3  not finite: one of F_u, F_v, Bq_u, Bq_v is NaN or +-inf;
 *   2  leaves the frame: q_x < 0, q_x > w - 1, q_y < 0 or q_y > h - 1;
 *   1  inconsistent: e > alpha1 ((F_u^2 + F_v^2) + (Bq_u^2 + Bq_v^2)) + alpha2;
 *   0  consistent.
 * alpha1 = 0.01, alpha2 = 0.5 are the values of Sundaram, Brox, Keutzer (ECCV 2010).
 * valid_u8: DEVICE uint8 [records][h][w], 1 for class 0 and 0 otherwise.  err_or_null: DEVICE
 * [records][h][w] of err_dtype FOTO_F32 | FOTO_F64 = sqrt(e), NaN for class 3.  table: DEVICE
 * double [records][4], the number of pixels of class 0, 1, 2, 3: integer counts summed in a fixed
 * order, the same bits from call to call.                                                       */
#define FOTO_CONSISTENCY_ALPHA1 0.01
#define FOTO_CONSISTENCY_ALPHA2 0.5
int foto_flow_consistency_dev(const foto_flow* fwd, const foto_flow* bwd, int w, int h, double alpha1, double alpha2,
                              void* valid_u8, void* err_or_null, int err_dtype, double* table, void* stream);

/* ------------------------------------------------------------------ flow filtering
 * The last stage of a classical flow pipeline on the foto_flow buffers the entries above leave in
 * HBM: the edge-aware weighted median of Sun, Roth and Black ("Secrets of optical flow estimation",
 * CVPR 2010), guided by an image, and the same operator with unusable pixels given weight zero,
 * which fills holes -- the pixels the mask of foto_flow_consistency_dev rejects -- from their usable
 * neighbours.  Additive; nothing in the solvers is involved and the reference has no such stage.
 * foto_flow_median_dev obeys the stream contract of the device-buffer section and never
 * synchronises with the host (but for a library scratch that has to grow); every device pointer is
 * checked for the CURRENT device before anything is enqueued; an argument error leaves the outputs
 * untouched.
 *
 * Inputs.  A foto_flow (F32 / F64, layout 0 / 1, K records) of w x h pixels, w, h >= 1.  An optional
 * guide: a foto_image that describes channel 0, `channels` >= 1 and stride_c as in
 * foto_render_warp_dev; a guide value is (double)pixel / divisor.  An optional mask, a foto_image,
 * non-zero = usable (foto_score_flow_dev's rule: the valid_u8 of foto_flow_consistency_dev goes in
 * as it is).  Guide and mask serve every record.
 *
 * Per record, rounds t = 1 .. rounds.  F_0 is the input widened exactly to double.  A pixel q is
 * USABLE in V_0 iff u_q and v_q are both finite and the mask, when given, is non-zero at q.
 *   window   for pixel p = (i, j) the q = (i + dx, j + dy), |dx|, |dy| <= R, that lie inside the
 *            frame: windows are truncated at the border, nothing is padded or mirrored.
 *   weight   a uint32: w(p, q) = spatial[dy + R][dx + R] * G(p, q) if q is usable in V_{t-1}, else
 *            0.  Without a guide G = 1.  With one, d = max over the channels of |I_c(q) - I_c(p)|
 *            (NaN if any of them is NaN), idx = min(n_range - 1, (int64)floor(d * range_scale +
 *            0.5)), a NaN d gives n_range - 1, and G = range[idx].  `spatial` and `range` are the
 *            caller's uint16 tables: the device never evaluates exp.
 *   median   T = the sum of w(p, q) over the window, an exact integer (at most 225 * 65535^2 <
 *            2^40).  For u and v separately the candidates are ordered by the monotone 64-bit key
 *            of the double, key = bits ^ (sign ? ~0 : 1 << 63), so -0.0 < +0.0 and no tie is
 *            ambiguous; the result is the value of the smallest key k among the usable candidates
 *            with 2 * (the sum of w(p, q) over key_q <= k) >= T: the LOWER weighted median, one of
 *            the samples, whatever the order of summation or the selection algorithm.
 *   T = 0    p is UNFILLED: F_t(p) = F_{t-1}(p) and p is not in V_t.
 *   T > 0    p is in V_t and F_t(p) is the median; with fill_only = 1 a p already in V_{t-1} keeps
 *            F_{t-1}(p) bit for bit and only unusable pixels are replaced.
 * foto_filter_check enforces spatial[R][R] > 0 and range[0] > 0, so a usable pixel always has T > 0
 * and V only grows.  The round count is fixed: no convergence test and no host synchronisation
 * (foto_flow_invert_dev's rule).  Between the rounds the flow lives as float64 with its mask in a
 * grow-only scratch of the library (17 bytes per pixel and record, twice); the conversion to
 * out_dtype happens after the last round only.
 *
 * Outputs.  out: K records of out_dtype FOTO_F32 ((float)x) or FOTO_F64, layout 0 or 1, = F_rounds.
 * The m plane of a layout-0 output is the input's m passed through (F64 to F64 bit for bit; the
 * filter acts on the motion only); of a layout-1 input, +0.0.  valid_out_or_null: DEVICE uint8
 * [K][h][w] = V_rounds.  table_or_null: DEVICE double [K][4] = {usable in V_0, filled (not in V_0,
 * in V_rounds), unfilled (not in V_rounds), 0}: integer counts summed in a fixed order, the same
 * bits from call to call.
 *
 * FOTO_ERR_ARG before any device call: anything foto_flow_check rejects, anything
 * foto_image_check rejects for the mask or a guide channel, channels < 1 or stride_c <= 0 with a
 * guide, a null opts, radius outside [1, FOTO_MEDIAN_MAX_RADIUS], rounds outside [1,
 * FOTO_MEDIAN_MAX_ROUNDS], fill_only outside {0, 1}, n_range outside [1, FOTO_MEDIAN_MAX_RANGE], a
 * range_scale that is not finite and > 0, spatial[R][R] = 0 or range[0] = 0, an out_dtype outside
 * {F32, F64}, an out_layout outside {0, 1}, a null or misaligned out, a misaligned table.
 * FOTO_ERR_ARG after the pointer queries: a pointer that is not device memory of the current
 * device, an output that overlaps an input or another output (the kernel gathers).  All index
 * arithmetic is int64_t.
 *
 * The kernel works on FOTO_MEDIAN_TILE_W x FOTO_MEDIAN_TILE_H pixel tiles, each staged on chip
 * with its R-wide halo (csrc/foto_filter.hip); the constants are here for the tests,
 * whose frame sizes derive from them, and are no part of the contract.                          */
#define FOTO_MEDIAN_MAX_RADIUS 7
#define FOTO_MEDIAN_MAX_ROUNDS 64
#define FOTO_MEDIAN_MAX_RANGE 256
#define FOTO_MEDIAN_TILE_W 32
#define FOTO_MEDIAN_TILE_H 8
typedef struct {
    int radius;          /* 1..7                                                      default 2 */
    int rounds;          /* 1..64                                                     default 1 */
    int fill_only;       /* 0 | 1                                                     default 0 */
    int n_range;         /* 1..256 entries of range[] in use                          default 1 */
    double range_scale;  /* finite, > 0: guide difference -> index of range[]       default 255 */
    uint16_t spatial[15 * 15];   /* row-major [2R+1][2R+1], the first (2R+1)^2 entries: default 1 */
    uint16_t range[256];         /*                                                   default 1 */
} foto_median_opts;
/* R = 2, 1 round, fill_only = 0, n_range = 1, range_scale = 255, every weight 1.                */
int foto_median_opts_default(foto_median_opts* o);
/* Host-only validation (no HIP call) of everything foto_flow_median_dev takes by descriptor: the
 * first list above up to range[0].                                                             */
int foto_filter_check(const foto_flow* fl, const foto_image* guide_or_null, int channels, int64_t stride_c,
                      const foto_image* mask_or_null, int w, int h, const foto_median_opts* opts);
/* The filter defined above, all records and one round per launch.  The options travel to the
 * kernel by value as a kernel argument: no upload, no wait.                                    */
int foto_flow_median_dev(const foto_flow* fl, const foto_image* guide_or_null, int channels, int64_t stride_c,
                         const foto_image* mask_or_null, int w, int h, const foto_median_opts* opts,
                         void* out, int out_dtype, int out_layout, void* valid_out_or_null, double* table_or_null,
                         void* stream);

/* ------------------------------------------------------------------ frame preparation
 * The stages BEFORE a solve, on device frames: what the reference does to a frame before main.py
 * sees it -- utils.openGrayscaleImage's convert('L') (utils.py:39-42), the halving of run.sh:18-30,
 * bin/create_lum_dataset.py, bin/normalize_image.py, bin/data_diff.py -- and the way back: a flow
 * solved at a reduced size resized to the size of the caller's frames.  A caller whose frames come
 * out of a decoder as RGB in HBM prepares them without a round trip through the host.  Additive.
 * Every *_dev entry obeys the stream contract of the device-buffer section, unchanged; every
 * device pointer is checked (for the plan's device, or the CURRENT one for the entries without a
 * plan) before anything is enqueued; all argument checks that need no device come before any HIP
 * call; an argument error leaves the outputs untouched.  Frames are foto_image views (channel 0;
 * channel c starts c * stride_c ELEMENTS further on, as in foto_render_warp_dev), flows are
 * foto_flow buffers, outputs are C-contiguous and may not overlap an input.
 *
 * Output rule of the pointwise stages (illuminate, normalise, difference), value x in float64:
 * FOTO_U8 is the reference's TRUNCATING np.uint8(255 * np.clip(x, 0, 1)), NaN -> 0 (the rule of
 * foto_render_warp_dev); FOTO_F32 is (float)x and FOTO_F64 is x, neither clipped.  A frame value
 * is (double)pixel / divisor.                                                                    */

/* PIL's convert('L') (utils.py:39-42) of a frame of 3 or 4 channels (R, G, B[, A]; alpha is
 * ignored).  out: [h][w] of the frame's dtype.  FOTO_U8: (19595 R + 38470 G + 7471 B + 0x8000) >> 16,
 * PIL's bits.  FOTO_F32 / FOTO_F64: ((19595 / 65536) R + (38470 / 65536) G) + (7471 / 65536) B in
 * float64 on the raw pixel values (the divisor is not applied), written in the frame's dtype.
 * FOTO_ERR_ARG: a null pointer, channels not 3 or 4, stride_c <= 0, anything foto_image_check
 * rejects for any channel, a misaligned out; then a non-device pointer, an out that overlaps.     */
int foto_prep_gray_dev(const foto_image* src, int channels, int64_t stride_c, int w, int h, void* out, void* stream);

/* Separable resize, bit for bit Pillow's Image.resize (Resample.c) for modes 'L' (FOTO_U8) and 'F'
 * (FOTO_F32), and the same in float64.  Per axis, n_in -> n_out and a filter of support S:
 *   scale = n_in / n_out, fs = max(1, scale), support = S fs, ksize = 2 ceil(support) + 1;
 *   output xx: center = (xx + 0.5) scale, first = max(0, (int)(center - support + 0.5)),
 *   count = min(n_in, (int)(center + support + 0.5)) - first,
 *   k[t] = filter((t + first - center + 0.5) / fs) (as (..) * (1 / fs)), t < count, then divided by
 *   their sum when it is not 0 (taps are clipped at the border and renormalised).
 * Filters (Resample.c): box (-0.5 < x <= 0.5), bilinear, bicubic with a = -0.5, Lanczos
 * sinc(x) sinc(x / 3) on [-3, 3) with the C library's sin.  (Hamming is left out: Pillow evaluates
 * it with float literals, and a double restatement is 1 ulp off in mode 'F'.)
 * The horizontal pass runs first, then the vertical one; a pass whose size does not change is
 * skipped; equal sizes return the input's bits.
 *   FOTO_U8        coefficients (int)(+-0.5 + k 2^22); an int32 accumulator from 2^21 plus pixel *
 *                  coefficient in tap order; each pass writes clip(acc >> 22, 0, 255) as uint8.
 *   FOTO_F32 / F64 a double accumulator from 0 plus (double)pixel * k in tap order; float32 writes
 *                  (float)acc after each pass (mode 'F'), float64 writes acc.
 * The divisor of the frame plays no part: pixels in, pixels out.
 * foto_resize_coeffs: the tables of one axis on the host, no GPU: *ksize always; bounds
 * [n_out][2] = (first, count), kk [n_out][ksize] (zero beyond count) and kk_int, the 22-bit
 * table, when non-null; cap = the entries kk / kk_int hold (FOTO_ERR_ARG when < n_out * ksize).   */
#define FOTO_FILTER_BOX 0        /* support 0.5 */
#define FOTO_FILTER_BILINEAR 1   /* support 1   */
#define FOTO_FILTER_BICUBIC 2    /* support 2   */
#define FOTO_FILTER_LANCZOS 3    /* support 3   */
int foto_resize_coeffs(int n_in, int n_out, int filter, int* ksize, int* bounds, double* kk, int32_t* kk_int, int cap);
/* A plan for (w, h) -> (ow, oh) and a filter on the current device: both axes' tables, computed
 * once on the host and uploaded once, a stream, and a grow-only scratch for the image between the
 * passes; reused for every frame of a video.  FOTO_ERR_ARG (nothing made): a null pointer, a size
 * < 1 or w h >= 2^31, a filter outside 0..3, an axis whose table n_out * ksize exceeds
 * FOTO_RESIZE_MAX_TABLE entries (foto_resize_coeffs likewise: nothing that large is allocated).  foto_resize_plan_info: info8 = {w, h, ow, oh,
 * filter, ksize of x, ksize of y, the widest input span of a horizontal tile}.
 * The horizontal pass works on tiles of FOTO_PREP_TILE_X outputs and stages a tile's input span on
 * chip; where the widest span exceeds the staging (512 elements: large reduction ratios, where an
 * output takes hundreds of taps -- 551 for 640 -> 7) it reads its taps from memory instead.  Both
 * routes do the same arithmetic and give the same bits.  route:
 * FOTO_RESIZE_ROUTE_AUTO picks, _LDS and _DIRECT force one (tests, timing; _LDS with a span that
 * does not fit is FOTO_ERR_ARG).  The tile width is here for the tests, whose sizes derive from it.*/
#define FOTO_PREP_TILE_X 64
#define FOTO_RESIZE_MAX_TABLE (1 << 22)
#define FOTO_RESIZE_ROUTE_AUTO 0
#define FOTO_RESIZE_ROUTE_LDS 1
#define FOTO_RESIZE_ROUTE_DIRECT 2
typedef struct foto_resize_plan foto_resize_plan;
int foto_resize_plan_create(int w, int h, int ow, int oh, int filter, foto_resize_plan** out);
void foto_resize_plan_destroy(foto_resize_plan* p);
int foto_resize_plan_device(const foto_resize_plan* p);   /* -1 for NULL */
int foto_resize_plan_info(const foto_resize_plan* p, int* info8);
/* A frame of `channels` channels (w x h, the plan's) -> out of the frame's dtype, [oh][ow][channels]
 * (out_planar = 0) or [channels][oh][ow] (out_planar = 1), every channel in the same launches.
 * FOTO_ERR_ARG: a null pointer, channels < 1, stride_c <= 0, anything foto_image_check rejects for
 * any channel, a misaligned out, an out_planar outside {0, 1}, a route
 * outside 0..2 or an LDS route that does not fit; then a pointer that is not device memory of
 * the plan's device, an out that overlaps the frame.                                             */
int foto_resize_dev(foto_resize_plan* p, const foto_image* src, int channels, int64_t stride_c, void* out,
                    int out_planar, int route, void* stream);
/* Every record and plane of a flow buffer of w x h records through the float path of the same
 * plan -> `out`, a buffer of the same dtype, layout and record count with ow x oh records.  In
 * the last pass that runs, before the final rounding, the accumulator of u is multiplied by
 * (double)ow / w and that of v by (double)oh / h; m is not scaled.  With it a solve at half
 * resolution answers at the size of the caller's frames and ground truth.  FOTO_ERR_ARG: a null
 * pointer, anything foto_flow_check rejects, a misaligned out, the route rules above; then a
 * pointer that is not device memory of the plan's device, an out that overlaps the flow.         */
int foto_flow_resize_dev(foto_resize_plan* p, const foto_flow* fl, void* out, int route, void* stream);

/* bin/normalize_image.py:20-26 on a pair: per frame one fixed-order sum S of the float64 values
 * (the order of normalize = 1 of foto_bb_create_dev: the same bits from call to call) and the
 * maximum; scale = max(max0 / S0, max1 / S1); out_k = (v / S_k) / scale by the output rule above.
 * out0, out1: [h][w] of out_dtype.  stats4 (HOST, required) = {S0, S1, max0, max1}: the call
 * waits for it.  A NaN pixel never wins the maximum.  Temporaries (both frames as float64) live
 * for the call.  FOTO_ERR_ARG: a null pointer, w or h < 1, anything foto_image_check rejects, an
 * out_dtype outside 0..2, a misaligned output; then a non-device pointer, an output that overlaps
 * a frame or the other output.                                                                   */
int foto_prep_normalize_pair_dev(const foto_image* f0, const foto_image* f1, int w, int h, void* out0, void* out1,
                                 int out_dtype, double* stats4, void* stream);

/* bin/create_lum_dataset.py:8-21: up to FOTO_PREP_MAX_SHAPES rectangles and discs added to the
 * frame's float64 values per pixel (i, j) = (column, row), in list order:
 *   FOTO_LUM_RECT    p = {L_x, L_y, r_x, r_y}: += v where (int)(r_x - L_x / 2) <= i < (int)(r_x +
 *                    L_x / 2) and likewise j (the reference's range(); here clipped to the frame,
 *                    where the reference's flat index would wrap into a neighbouring row or raise);
 *   FOTO_LUM_CIRCLE  p = {R, c_x, c_y, unused}: += v where (i - c_x)^2 + (j - c_y)^2 < R^2.
 * out: [h][w] of out_dtype by the output rule above.  FOTO_ERR_ARG: a null pointer, count outside
 * 0..FOTO_PREP_MAX_SHAPES, a kind outside {0, 1}, a parameter or value that is not finite (a
 * rectangle bound beyond 1e9), the image and output rules above.                                 */
#define FOTO_PREP_MAX_SHAPES 8
#define FOTO_LUM_RECT 0
#define FOTO_LUM_CIRCLE 1
typedef struct {
    int kind;        /* FOTO_LUM_RECT | FOTO_LUM_CIRCLE                                          */
    int reserved;    /* 0                                                                        */
    double p[4];     /* see above                                                                */
    double v;        /* the value added                                                          */
} foto_lum_shape;
int foto_prep_illuminate_dev(const foto_image* src, int w, int h, const foto_lum_shape* shapes, int count, void* out,
                             int out_dtype, void* stream);

/* bin/data_diff.py:35-39: d = v1 - v0 in float64, its minimum and maximum (order-independent; a
 * NaN never wins), out = (d - min) / (max - min) by the output rule above: [h][w] of out_dtype.  A
 * constant difference gives 0 / 0: 0 as uint8, NaN as float.  minmax2_or_null (HOST) = {min, max}.
 * Temporaries live for the call, which waits for them.  Argument rules: those of the pair above. */
int foto_prep_diff_dev(const foto_image* f0, const foto_image* f1, int w, int h, void* out, int out_dtype,
                       double* minmax2_or_null, void* stream);

/* ------------------------------------------------------------------ sparse tracking
 * Feature points and a classical sparse tracker on device frames: Shi-Tomasi corners (Shi & Tomasi
 * 1994), pyramidal Lucas-Kanade with fixed counts (Lucas & Kanade 1981; Bouguet 2001), and a dense
 * flow sampled at points.  No reference counterpart (the reference tracks pixel centres through
 * the transport only, utils.py:44-99); tests/sparse_ref.py restates the arithmetic below in numpy
 * and the device equals it bit for bit.  Additive.  Everything is float64 on the device; frames
 * are foto_image views, widened as (double)pixel / divisor like every *_dev entry; points are
 * [M][2] = (x, y) in foto_bb_track's coordinates (x along w).  Every entry obeys the stream
 * contract of the device-buffer section; argument checks that need no device come before any HIP
 * call, every device pointer is checked before anything is enqueued, and an argument error leaves
 * the outputs untouched.  None of them waits for the device, but foto_corners_dev with a host
 * count.  Gx, Gy below are central differences, zero in the first and last column / row (the
 * gradients of the TV-L1 solver); S(f; x, y) is the clamped bilinear sample of the pyramid.
 *
 * Corners.  Box sums a, b, cc of Gx Gx, Gx Gy, Gy Gy over (2 c + 1)^2 pixels, a plane counting as
 * +0.0 outside the frame: first H[j][i] = sum over dx = -c..c of P[j][i + dx], in increasing dx
 * from the first term, then the sum over dy = -c..c of H[j + dy][i], in increasing dy.
 *   R = 0.5 ((a + cc) - sqrt((a - cc) (a - cc) + 4.0 (b b)))
 * Rmax = the largest finite positive R of the frame (0 when there is none).  A pixel is a
 * candidate when R is finite and > 0, R >= quality Rmax, the pixel is at least `margin` pixels
 * from every border, and R is the maximum of its (2 s + 1)^2 neighbourhood truncated at the frame,
 * ties going to the earlier pixel in raster order (R > every earlier neighbour, R >= every later
 * one; a NaN neighbour fails both).  Of the candidates the max_count strongest are kept (R
 * descending, then index ascending) and written in raster order; rows from the count on are NaN.
 * The count goes to count_dev (a device int32) and, when count_host_or_null is given, to the host:
 * only then does the call wait.  response_or_null: a device double[h][w] that receives R.        */
#define FOTO_CORNER_MAX_WINDOW 7
#define FOTO_CORNER_MAX_NMS 15
typedef struct {
    double quality;   /* in [0, 1]                                                              */
    int window;       /* c: the box radius, 1 .. FOTO_CORNER_MAX_WINDOW                          */
    int nms;          /* s: the suppression radius, 1 .. FOTO_CORNER_MAX_NMS                     */
    int margin;       /* >= 0                                                                    */
    int reserved;     /* 0                                                                       */
} foto_corner_opts;
/* quality 0.01, window 3, nms 5, margin 8 */
int foto_corner_opts_default(foto_corner_opts* o);
/* opts NULL: the defaults.  pts: [max_count][2] of pts_dtype FOTO_F32 | FOTO_F64 (an index is
 * exact in either).  FOTO_ERR_ARG: a null pointer, w or h < 2 or w h >= 2^31, anything
 * foto_image_check rejects, an option outside its range, max_count < 1, a dtype outside {F32,
 * F64}, a misaligned pointer; then a pointer that is not device memory of the current device.    */
int foto_corners_dev(const foto_image* frame, int w, int h, const foto_corner_opts* opts, int max_count, void* pts,
                     int pts_dtype, int32_t* count_dev, int* count_host_or_null, double* response_or_null,
                     void* stream);

/* Pyramidal Lucas-Kanade.  The plan owns both frames' pyramids: the levels of foto_gn_pyr_sizes(w,
 * h, levels, min_size), built by foto_lk_set_frames_dev with the GN pyramid's restriction
 * (foto_pyr_down); any number of track calls may follow.  A point (x, y) of level 0 is carried to
 * level l by repeating x <- (x + 0.5) ((double)w_{l+1} / (double)w_l) - 0.5 (y with h); d starts
 * at 0 on the coarsest level and is scaled by (double)w_l / (double)w_{l+1} (h for d_y) on
 * entering level l.  At a level, over the window offsets (ax, ay) in [-R, R]^2, element e = (ay +
 * R) (2 R + 1) + (ax + R), n = (2 R + 1)^2:
 *   T_e = S(f; x + ax, y + ay), Gx_e = S(Gx f; .), Gy_e = S(Gy f; .)       (f: the template frame)
 *   gxx = sum Gx_e^2, gxy = sum Gx_e Gy_e, gyy = sum Gy_e^2, det = gxx gyy - gxy gxy,
 *   mineig = 0.5 ((gxx + gyy) - sqrt((gxx - gyy) (gxx - gyy) + 4.0 (gxy gxy))) / n;
 *   unless mineig > min_eig the level is skipped (d unchanged; at level 0 status gets FLAT);
 *   otherwise exactly `iters` times, with no stop test:
 *     r_e = T_e - S(g; (x + d_x) + ax, (y + d_y) + ay)                     (g: the search frame)
 *     bx = sum r_e Gx_e, by = sum r_e Gy_e,
 *     d_x += (gyy bx - gxy by) / det, d_y += (gxx by - gxy bx) / det.
 * Every sum over e has one order: lane p of 64 adds its slots e = p, p + 64, p + 128, p + 192 (0.0
 * for a slot >= n) as ((s0 + s1) + s2) + s3; the 64 partials go through the tree a[p] += a[p + o],
 * p < o, for o = 32, 16, .., 1.  After level 0: err = sum |r_e| / n at the final d (one more
 * residual pass).  Status bits: FLAT; OUT: the start point or the end point is not inside [0, w-1]
 * x [0, h-1]; NONFINITE: a NaN or Inf coordinate or result -- for that point alone d and err are
 * NaN (and OUT is set); it is neither an error nor an out-of-range read.
 * direction 0: template f0, search f1; 1: the roles swapped.  prior_or_null: a device [M][2] of
 * `dtype`; with it the start point is pts + prior, fb = sqrt(sx sx + sy sy) with s = prior + d goes
 * to fb_or_null, and the status buffer is not overwritten: INCONSISTENT is OR-ed into it unless fb
 * <= fb_tol.  The backward call (direction 1, prior = the forward call's `out`, the forward
 * call's status) after a forward call is therefore the whole forward-backward check, with
 * nothing downloaded.  out: [M][2] = d (x_end - x_start, foto_bb_track's convention) of dtype
 * FOTO_F32 | FOTO_F64; status: uint8[M]; err_or_null, fb_or_null: double[M].
 * FOTO_ERR_ARG: a null pointer, the size rules of foto_gn_pyr_sizes, radius outside 1 ..
 * FOTO_LK_MAX_RADIUS, iters < 1, min_eig negative or not finite, M < 1 or > 2^31 - 1, a dtype
 * outside {F32, F64}, a pair array not aligned to a pair, a direction outside {0, 1}, fb without
 * a prior, a NaN fb_tol with a prior; then a pointer that is not device memory of the plan's
 * device, an `out` that overlaps pts or prior.  FOTO_ERR_STATE: a track before any frames.       */
#define FOTO_LK_MAX_RADIUS 7
#define FOTO_LK_FLAT 1
#define FOTO_LK_OUT 2
#define FOTO_LK_NONFINITE 4
#define FOTO_LK_INCONSISTENT 8
typedef struct {
    int radius;       /* R: 1 .. FOTO_LK_MAX_RADIUS                                              */
    int levels;       /* >= 1 (foto_gn_pyr_sizes)                                                */
    int min_size;     /* >= 2 (foto_gn_pyr_sizes)                                                */
    int iters;        /* >= 1                                                                    */
    double min_eig;   /* finite, >= 0                                                            */
} foto_lk_opts;
/* radius 7, levels 4, min_size 16, iters 10, min_eig 1e-7 */
int foto_lk_opts_default(foto_lk_opts* o);
typedef struct foto_lk foto_lk;
int foto_lk_create(int w, int h, const foto_lk_opts* opts, foto_lk** out);
void foto_lk_destroy(foto_lk* p);
int foto_lk_device(const foto_lk* p);   /* -1 for NULL */
int foto_lk_set_frames_dev(foto_lk* p, const foto_image* f0, const foto_image* f1, void* stream);
int foto_lk_track_dev(foto_lk* p, const void* pts, int pts_dtype, int64_t M, int direction, const void* prior_or_null,
                      double fb_tol, void* out, int dtype, unsigned char* status, double* err_or_null,
                      double* fb_or_null, void* stream);

/* A dense flow read at points: out[r][p] = (S(u_r; x_p, y_p), S(v_r; x_p, y_p)) for every record r
 * of a flow buffer of w x h records (values widened exactly) -- a dense solver's flow, a ground
 * truth and the LK tracks on the same points.  out: [records][M][2] of dtype FOTO_F32 | FOTO_F64.
 * A NaN coordinate gives NaN, read from in-frame taps.  FOTO_ERR_ARG: anything foto_flow_check
 * rejects, w or h < 2, the point rules above; then a pointer that is not device memory of the
 * current device, an out that overlaps an input.                                                 */
int foto_flow_sample_dev(const foto_flow* fl, int w, int h, const void* pts, int pts_dtype, int64_t M, void* out,
                         int dtype, void* stream);

/* ------------------------------------------------------------------ global motion
 * The one parametric motion that dominates a set of tracks or a dense flow: a RANSAC fit (Fischler
 * & Bolles 1981) of a translation, similarity, affine map or homography in frame-normalised
 * coordinates (Hartley & Zisserman 2004, 4.4), refined by least squares over its inliers; the
 * model's flow field, and a flow with that field removed.  No reference counterpart;
 * tests/motion_ref.py restates the arithmetic below in numpy and the device equals it bit for bit.
 * Additive.  Everything is float64 on the device, inputs widened exactly.  Every entry obeys the
 * stream contract of the device-buffer section; argument checks that need no device come before
 * any HIP call, every device pointer is checked (for the CURRENT device) before anything is
 * enqueued, and an argument error leaves the outputs untouched.  No entry waits for the device:
 * the best hypothesis is chosen there and every result stays in device memory.  (A sample table
 * that differs from the one of the previous call is uploaded first, which may wait for that
 * previous call's work; a scratch that has to grow waits likewise.)
 *
 * Models.  A model maps a start point to an end point and is a row-major 3 x 3 matrix m[9] with
 * m[8] = 1, in pixel coordinates for the caller ((x, y), x along w) and in normalised coordinates
 * inside the fit.  k = the minimal sample, P = the parameters p:
 *   TRANSLATION k 1, P 2   m = (1, 0, p0;  0, 1, p1;  0, 0, 1)
 *   SIMILARITY  k 2, P 4   m = (p0, -p1, p2;  p1, p0, p3;  0, 0, 1)
 *   AFFINE      k 3, P 6   m = (p0, p1, p2;  p3, p4, p5;  0, 0, 1)
 *   HOMOGRAPHY  k 4, P 8   m = (p0, p1, p2;  p3, p4, p5;  p6, p7, 1)
 * A correspondence (x, y) -> (X, Y) gives two rows r1, r2 of length P with right-hand sides b1, b2:
 *   TRANSLATION  r1 = (1, 0), b1 = X - x;  r2 = (0, 1), b2 = Y - y
 *   SIMILARITY   r1 = (x, -y, 1, 0), b1 = X;  r2 = (y, x, 0, 1), b2 = Y
 *   AFFINE       r1 = (x, y, 1, 0, 0, 0), b1 = X;  r2 = (0, 0, 0, x, y, 1), b2 = Y
 *   HOMOGRAPHY   r1 = (x, y, 1, 0, 0, 0, -(X x), -(X y)), b1 = X;  r2 = (0, 0, 0, x, y, 1, -(Y x), -(Y y)), b2 = Y
 * (the homography in its inhomogeneous form, X (p6 x + p7 y + 1) = p0 x + p1 y + p2).
 *
 * Elimination.  An n x n system A p = b: for c = 0 .. n - 1 the pivot row is the row r >= c with the
 * largest |A[r][c]|, the lowest such row on a tie; unless |A[r][c]| > 1e-12 the system is
 * DEGENERATE; rows c and r are exchanged; then for r = c + 1 .. n - 1: f = A[r][c] / A[c][c], A[r][j]
 * = A[r][j] - f A[c][j] for j = c + 1 .. n - 1, b[r] = b[r] - f b[c].  Back: for r = n - 1 .. 0, s =
 * b[r], s = s - A[r][j] p[j] for j = r + 1 .. n - 1 in increasing j, p[r] = s / A[r][r].
 *
 * The fit.  1. s = 0.5 max(w, h), cx = 0.5 (w - 1), cy = 0.5 (h - 1).  Correspondence i with start
 * (px, py) and displacement (dx, dy) is VALID when the four numbers are finite and its status byte
 * (when there is a status array) is 0; x = (px - cx) / s, y = (py - cy) / s, X = ((px + dx) - cx) /
 * s, Y = ((py + dy) - cy) / s.  2. The valid correspondences, in index order, form the list q = 0 ..
 * n_valid - 1.  3. Hypothesis j < H takes the list entries ((uint64)samples[j][i] n_valid) >> 32, i <
 * k, stacks their rows (entry i: rows 2 i, 2 i + 1) and solves; with n_valid < k, or a degenerate
 * system, the hypothesis is degenerate and scores -1.  4. With wv = (m6 x + m7 y) + 1, ex = ((m0 x +
 * m1 y) + m2) - X wv, ey = ((m3 x + m4 y) + m5) - Y wv and t = threshold / s, a list entry is an
 * INLIER of m when wv > 0 and ex ex + ey ey <= (t t) (wv wv).  The score of a hypothesis is its
 * inlier count; the winner has the highest score, the lowest j on a tie.  When the winner's score
 * is below max(k, min_inliers): FOTO_MOTION_NONE -- the model is the identity, the mask 0, inliers
 * 0, the winner -1, rms NaN: a result, not an error.  5. Otherwise exactly `rounds` times: with
 * fewer than k inliers of the current model m, or a degenerate system, m stays and status gains
 * FOTO_MOTION_KEPT; else m becomes the solution of N p = g, N[a][b] = sum (r1[a] r1[b] + r2[a]
 * r2[b]) (a <= b, mirrored), g[a] = sum (r1[a] b1 + r2[a] b2) over the inliers of m.  6. The mask is
 * 1 at the inliers of the final m; rms = s sqrt(S / inliers), S = sum (rx rx + ry ry), rx = ((m0 x +
 * m1 y) + m2) / wv - X, ry likewise.  The pixel matrix: with A[i][0] = m[i][0] / s, A[i][1] = m[i][1]
 * / s, A[i][2] = (m[i][2] - (m[i][0] cx) / s) - (m[i][1] cy) / s, B[0][j] = s A[0][j] + cx A[2][j],
 * B[1][j] = s A[1][j] + cy A[2][j], B[2][j] = A[2][j]: out[i][j] = B[i][j] / B[2][2], out[2][2] = 1.
 * Every floating-point sum of 5 and 6 has one order, fixed by M alone: the list, followed by +0.0
 * terms (an entry that is no inlier is a +0.0 term too), in ceil(M / FOTO_MOTION_TILE) tiles of
 * FOTO_MOTION_TILE = 1024 entries; in a tile thread p of 256 adds its entries p, p + 256, p + 512,
 * p + 768 as ((s0 + s1) + s2) + s3, the 64 partials of each of the four waves go through the tree
 * a[p] += a[p + o], p < o, o = 32, 16, .., 1, the four wave sums add as ((w0 + w1) + w2) + w3, and
 * the tile sums are added to 0.0 in tile order.  Counts are integers.
 *
 * samples: a HOST uint32[H][4] (foto.motion.samples draws it with numpy; the device draws no random
 * number); the index rule above is in range for every n_valid, so the table depends on neither M
 * nor a count that only the device knows.
 * Outputs (device): model double[9]; inliers uint8[M] (0 for an invalid correspondence); info
 * int64[4] = (inliers, n_valid, winner, status bits); rms double[1].
 * FOTO_ERR_ARG: a null pointer (status excepted), M < 1 or > 2^31 - 1, H < 1, a model outside the
 * four, a threshold that is not finite and > 0, rounds < 0, min_inliers < 0, w or h < 2, a dtype
 * outside {F32, F64}, a pair array not aligned to a pair, a misaligned output; then a pointer that
 * is not device memory of the current device, an output that overlaps an input or another output. */
#define FOTO_MOTION_TRANSLATION 0
#define FOTO_MOTION_SIMILARITY 1
#define FOTO_MOTION_AFFINE 2
#define FOTO_MOTION_HOMOGRAPHY 3
#define FOTO_MOTION_NONE 1   /* status bit: no hypothesis reached max(k, min_inliers) inliers      */
#define FOTO_MOTION_KEPT 2   /* status bit: a refinement round kept the model it started from     */
#define FOTO_MOTION_TILE 1024
typedef struct {
    int model;          /* FOTO_MOTION_TRANSLATION .. FOTO_MOTION_HOMOGRAPHY; the default leaves -1 */
    int rounds;         /* refinement rounds, >= 0                                                 */
    int min_inliers;    /* >= 0                                                                    */
    int reserved;       /* 0                                                                       */
    double threshold;   /* the inlier distance in pixels, finite and > 0                           */
} foto_motion_opts;
/* model -1 (the caller chooses), rounds 3, min_inliers 0, threshold 1.0 */
int foto_motion_opts_default(foto_motion_opts* o);
/* pts, disp: [M][2] of FOTO_F32 | FOTO_F64, what foto_corners_dev and foto_lk_track_dev /
 * foto_flow_sample_dev write; status_or_null: uint8[M], non-zero = unusable (LK's status byte). */
int foto_motion_fit_dev(const void* pts, int pts_dtype, const void* disp, int disp_dtype,
                        const unsigned char* status_or_null, int64_t M, int w, int h, const foto_motion_opts* opts,
                        const uint32_t* samples, int H, double* model, unsigned char* inliers, int64_t* info,
                        double* rms, void* stream);
/* The same fit on record `record` of a flow buffer of w x h records: the correspondences are the
 * lattice pixels (i stride, j stride), i < lw = (w - 1) / stride + 1, j < lh = (h - 1) / stride + 1,
 * number j lw + i, M = lw lh, with the flow there as displacement; valid when u and v are finite and
 * mask_or_null (uint8[h][w], foto_flow_consistency_dev's `valid`: non-zero = usable) allows the
 * pixel.  inliers: uint8[lh][lw].  FOTO_ERR_ARG: the rules above, anything foto_flow_check
 * rejects, a record outside the buffer, stride < 1.                                              */
int foto_motion_fit_flow_dev(const foto_flow* fl, int record, int w, int h, int stride,
                             const unsigned char* mask_or_null, const foto_motion_opts* opts, const uint32_t* samples,
                             int H, double* model, unsigned char* inliers, int64_t* info, double* rms, void* stream);
/* The flow field of `count` pixel models (device double[count][9]): record r of `out`, a flow buffer
 * of `dtype`, `layout` and count records, is at pixel (x, y): wv = (m6 x + m7 y) + m8, u = ((m0 x +
 * m1 y) + m2) / wv - x, v = ((m3 x + m4 y) + m5) / wv - y, both NaN unless wv > 0; m = 0 (planar).
 * What foto_render_warp_dev, foto_flow_compose_dev and foto_score_flow_dev take as it is.
 * FOTO_ERR_ARG: a null pointer, count < 1, w or h < 1 or w h >= 2^31, a dtype outside {F32, F64}, a
 * layout outside {0, 1}, a misaligned pointer; then non-device memory, an overlap.               */
int foto_motion_field_dev(const double* models, int count, int w, int h, void* out, int dtype, int layout,
                          void* stream);
/* flow - field per record, the motion left once the global one is removed: `out` has the flow's
 * dtype, layout and record count; u_out = u - field u, v_out = v - field v in float64 (NaN where
 * the field is), m copied.  count: 1 (one model for every record) or fl->records.                */
int foto_motion_residual_dev(const foto_flow* fl, const double* models, int count, int w, int h, void* out,
                             void* stream);

/* ------------------------------------------------------------------ feature matching
 * Wide-baseline correspondences, the stage between foto_corners_dev and foto_motion_fit_dev that
 * needs no small displacement: a 256-bit binary descriptor of the neighbourhood of each point
 * (BRIEF, Calonder et al. 2010, test pairs G II; with an intensity-centroid orientation, Rublee et
 * al. 2011), the nearest and second-nearest descriptor under the Hamming distance with the usual
 * rejections (a distance bound, Lowe's ratio, a spatial gate), and the mutual check.  No reference
 * counterpart; tests/match_ref.py restates the arithmetic below in numpy and the device equals it
 * bit for bit.  Additive.  Frames are foto_image views, widened as (double)pixel / divisor like
 * every *_dev entry; points are [M][2] = (x, y), x along w.  Every entry obeys the stream contract
 * of the device-buffer section; argument checks that need no device come before any HIP call,
 * every device pointer is checked (for the CURRENT device) before anything is enqueued, and an
 * argument error leaves the outputs untouched.  No entry waits for the device.  (Tables that
 * differ from those of the previous call are uploaded first, which may wait for that previous
 * call's work; a scratch that has to grow waits likewise.)
 *
 * Tables (HOST, copied by the call; the device draws no random number and evaluates no sin, cos
 * or atan2).  pattern: int8 [K][256][4] = (ax, ay, bx, by), the 256 test pairs of each of the K =
 * `orientations` bins, every end inside the disc ax ax + ay ay <= patch patch (foto.match.pattern
 * draws bin 0 and rotates it into the others).  directions: float64 [K][2] = (C[k], S[k]) = (cos,
 * sin)(2 pi k / K) (foto.match.directions).
 *
 * Descriptors.  The smoothed plane B is the box sum of the widened frame F over (2 blur + 1)^2
 * pixels, F counting as +0.0 outside the frame, not divided: H[j][i] = sum over dx = -blur .. blur
 * of F[j][i + dx], in increasing dx from the first term, then B[j][i] = sum over dy = -blur .. blur
 * of H[j + dy][i], in increasing dy from the first term (the corner detector's box sums).  blur = 0:
 * B = F.  The keypoint pixel of a point (x, y) is (i, j) = (floor(x + 0.5), floor(y + 0.5)), in
 * double.  state: FOTO_MATCH_NONFINITE | FOTO_MATCH_OUT for a NaN or Inf coordinate; FOTO_MATCH_OUT
 * unless patch <= i <= w - 1 - patch and patch <= j <= h - 1 - patch; in either case the
 * descriptor is four zero words and bin = -1, and nothing is read for the point.  Otherwise state
 * = 0 and:
 *   orientation (K > 1): m10 = sum ax F[j + ay][i + ax], m01 = sum ay F[j + ay][i + ax] over the
 *   elements e = (ay + patch) (2 patch + 1) + (ax + patch), e < n = (2 patch + 1)^2, a term being
 *   +0.0 where ax ax + ay ay > patch patch; lane p of 64 adds its slots e = p, p + 64, p + 128, ..
 *   (ceil(n / 64) of them, +0.0 for e >= n) in increasing e from the first term, and the 64 partials
 *   go through the tree a[p] += a[p + o], p < o, for o = 32, 16, .., 1.  bin = the k that maximises
 *   m10 C[k] + m01 S[k] (two products, one sum, each rounded), the lowest such k: bin = 0, then k
 *   = 1 .. K - 1 replaces it when its value is > the value held (false for a NaN: a NaN moment
 *   gives bin 0).  K = 1: bin = 0 and no moment is computed.
 *   bits: for t = 0 .. 255 with (ax, ay, bx, by) = pattern[bin][t]: bit t = B[j + ay][i + ax] < B[j +
 *   by][i + bx] (false for a NaN), bit t % 64 of word t / 64.
 * desc: uint64[M][4]; state: uint8[M]; bin_or_null: int32[M].
 * FOTO_ERR_ARG: a null pointer (bin excepted), w or h < 2 patch + 1 or w h >= 2^31, anything
 * foto_image_check rejects, blur outside 0 .. FOTO_MATCH_MAX_BLUR, patch outside 2 ..
 * FOTO_MATCH_MAX_PATCH, orientations outside 1 .. FOTO_MATCH_MAX_ORIENT, a pattern entry outside
 * the disc of `patch`, M < 1 or > 2^31 - 1, a dtype outside {F32, F64}, a misaligned pointer; then a
 * pointer that is not device memory of the current device, an output that overlaps an input or
 * another output.
 *
 * Matching.  Train entry j < N1 is a CANDIDATE of query i < N0 when state1[j] == 0 and either
 * max_disp == 0 or both |x1_j - x0_i| <= max_disp and |y1_j - y0_i| <= max_disp, on coordinates
 * widened to double (false for a NaN).  d(i, j) = the number of set bits of desc0[i] XOR desc1[j]
 * over the four words.  The best candidate j1 has the smallest key (d, j) -- ties go to the lower j
 * -- and d1 = d(i, j1); d2 is the smallest d over the other candidates; 257 stands for "none" in
 * either place.  An order of the reduction does not enter: the minimum of an ordered integer key
 * has none.  For a query with state0[i] != 0: status = state0[i], idx = -1, dist = (257, 257).
 * Otherwise dist = (d1, d2), idx = j1, status = 0, and
 *   FOTO_MATCH_NONE is set, and idx = -1, when there is no candidate or d1 > max_dist (dist keeps
 *   what was found);
 *   FOTO_MATCH_AMBIGUOUS is set unless ratio == 0 or d1 256 < ratio d2 (integers; d = 257 where
 *   there is none, so a query without any candidate carries both bits).
 * disp (optional): pts1[idx] - pts0[i] per component, in double, narrowed; NaN where idx < 0.
 * idx: int32[N0]; dist: int32[N0][2]; status: uint8[N0]; disp_or_null: [N0][2] of disp_dtype.
 * FOTO_ERR_ARG: a null pointer (disp excepted), N0 or N1 < 1 or > 2^31 - 1, max_disp negative, NaN
 * or infinite, max_dist outside 0 .. 256, ratio outside 0 .. 256, a dtype outside {F32, F64}, a
 * misaligned pointer (desc0, desc1: 16 bytes, one vector load per half descriptor; a pair array: a
 * pair); then non-device memory, an output that overlaps an input or another output.
 *
 * The mutual check.  foto_match_cross_dev ORs FOTO_MATCH_NOT_MUTUAL into status[i] where idx01[i]
 * >= 0 and idx10[idx01[i]] != i (an idx01[i] >= N1 counts as not mutual and reads nothing); like
 * LK's INCONSISTENT it overwrites nothing else.  Two foto_match_dev calls (0 -> 1, 1 -> 0) and this
 * one, on one stream, are the whole check with nothing downloaded.  The status byte is what
 * foto_motion_fit_dev takes: non-zero = unusable.                                                 */
#define FOTO_MATCH_MAX_PATCH 31
#define FOTO_MATCH_MAX_ORIENT 32
#define FOTO_MATCH_MAX_BLUR 7
#define FOTO_MATCH_NONE 1         /* no candidate, or the best one farther than max_dist           */
#define FOTO_MATCH_OUT 2          /* the patch leaves the frame (FOTO_LK_OUT's value)              */
#define FOTO_MATCH_NONFINITE 4    /* a NaN or Inf coordinate (FOTO_LK_NONFINITE's value)           */
#define FOTO_MATCH_NOT_MUTUAL 8   /* the best match's best match is another query                  */
#define FOTO_MATCH_AMBIGUOUS 16   /* the second best is too close (Lowe's ratio)                   */
#define FOTO_MATCH_TILE 256       /* train descriptors per LDS tile: the tests' sizes derive from   */
#define FOTO_MATCH_QUERIES 512    /* queries per block; and from the blocks a launch aims at        */
#define FOTO_MATCH_BLOCKS 1024
typedef struct {
    int blur;           /* the box radius of the smoothed plane, 0 .. FOTO_MATCH_MAX_BLUR          */
    int patch;          /* the disc's radius, 2 .. FOTO_MATCH_MAX_PATCH                            */
    int orientations;   /* K, 1 .. FOTO_MATCH_MAX_ORIENT                                           */
    int reserved;       /* 0                                                                       */
} foto_describe_opts;
/* blur 2, patch 15, orientations 1 */
int foto_describe_opts_default(foto_describe_opts* o);
typedef struct {
    double max_disp;    /* the spatial gate in pixels, finite and >= 0; 0: no gate                 */
    int max_dist;       /* 0 .. 256                                                                */
    int ratio;          /* 0 .. 256, in 1 / 256; 0: no ratio test                                  */
    int reserved[2];    /* 0                                                                       */
} foto_match_opts;
/* max_disp 0, max_dist 64, ratio 205 (Lowe's 0.8) */
int foto_match_opts_default(foto_match_opts* o);
/* opts NULL: the defaults.  pattern, directions: the HOST tables above for opts->orientations. */
int foto_describe_dev(const foto_image* frame, int w, int h, const void* pts, int pts_dtype, int64_t M,
                      const foto_describe_opts* opts, const int8_t* pattern, const double* directions,
                      uint64_t* desc, unsigned char* state, int32_t* bin_or_null, void* stream);
/* opts NULL: the defaults.  The train set is split over blocks so that about FOTO_MATCH_BLOCKS
 * blocks run whatever N0 is; the partial minima are merged in a second launch.                   */
int foto_match_dev(const uint64_t* desc0, const unsigned char* state0, const void* pts0, int pts0_dtype, int64_t N0,
                   const uint64_t* desc1, const unsigned char* state1, const void* pts1, int pts1_dtype, int64_t N1,
                   const foto_match_opts* opts, int32_t* idx, int32_t* dist, unsigned char* status,
                   void* disp_or_null, int disp_dtype, void* stream);
int foto_match_cross_dev(const int32_t* idx01, int64_t N0, const int32_t* idx10, int64_t N1, unsigned char* status,
                         void* stream);

/* ------------------------------------------------------------------ entropic transport
 * The static counterpart of the BB solver: entropic optimal transport between two frames on the
 * pixel grid (Cuturi 2013; Solomon et al. 2015, "Convolutional Wasserstein distances") with the
 * cost c(x, y) = |x - y|^2 / 2.  The Gibbs kernel exp(-c / eps) is a separable Gaussian of variance
 * eps px^2, truncated here to the (2 R + 1)^2 box |dx|, |dy| <= R; one Sinkhorn half-iteration is
 * one separable convolution and one division per pixel.  The plan's barycentric projection is a
 * flow, its cost a W2.  No reference counterpart; tests/sinkhorn_ref.py restates the arithmetic
 * below in numpy and the device equals it bit for bit.  Additive.  Everything is float64 on the
 * device.  Every *_dev entry obeys the stream contract of the device-buffer section; argument
 * checks that need no device come before any HIP call, device pointers are checked for the
 * context's device before anything is enqueued.  No entry but foto_sinkhorn_solve waits for the
 * device: every count is fixed, there is no stop test.
 *
 * Frames.  mu (frame 0) and nu (frame 1) are h x w; an input pixel that is negative or not finite
 * counts as 0 and is counted in `bad`.  The solver equalises nothing: the masses are the caller's
 * (foto_prep_normalize_pair_dev) and the record reports both.
 * Tables.  A HOST float64 [3][R + 1], d = 0 .. R: k[d] = exp(-d d / (2 eps)), k1[d] = d k[d],
 * k2[d] = (0.5 (d d)) k[d] (foto.sinkhorn.tables makes it with numpy; the device never evaluates
 * exp).  The entries for negative d are k[|d|], -k1[|d|], k2[|d|].
 * Convolution conv(p, q, z) with row table p and column table q:
 *   t(j, i) = sum_{d = -R .. R} p[d] z(j, i + d),   s(j, i) = sum_{d = -R .. R} q[d] t(j + d, i),
 * each sum sequential in ascending d from 0.0, the product rounded before the add; a tap outside
 * the frame is 0.0.  div(m, s) = m / s where m > 0 and s > 0, else 0.
 * Iterations.  From a = 0, b = 1, one iteration is a = div(mu, conv(k, k, b)), then b = div(nu,
 * conv(k, k, a)).
 * Flow, frame 0 -> frame 1 (direction 0).  With s = conv(k, k, b): u = conv(k1, k, b) / s, v =
 * conv(k, k1, b) / s where mu > 0 and s > 0 (valid = 1); elsewhere u = v = 0 and valid = 0.  m = 0
 * everywhere.  Direction 1 (frame 1 -> frame 0) is the same with a, nu in place of b, mu.
 * The record, float64[8]: sum mu, sum nu, the marginal error sum |a s - mu|, the sharp cost sum a
 * (conv(k2, k, b) + conv(k, k2, b)), bad, unreachable (pixels with mu > 0 and s = 0), iterations
 * done, 0.  The sums have one order fixed by w h (they keep their bits from call to call), which
 * the tests do not rely on beyond the bound of any order, w h 2^-53 sum |terms|.
 *
 * FOTO_ERR_ARG (nothing made, nothing enqueued): a null pointer (valid_or_null excepted), w or h <
 * 1 or w h >= 2^31, radius outside 0 .. FOTO_SINKHORN_MAX_RADIUS, eps not finite and > 0, n < 0, a
 * direction outside {0, 1}, anything foto_image_check or the export rules reject, a pointer that is
 * not device memory of the context's device.  FOTO_ERR_STATE: iterate, flow, info or scalings
 * before any frames.                                                                             */
#define FOTO_SINKHORN_MAX_RADIUS 32
#define FOTO_SINKHORN_TILE_W 64   /* the fused kernel's tile: the tests' frame sizes derive from it */
#define FOTO_SINKHORN_TILE_H 32
typedef struct {
    int radius;                /* R, 0 .. FOTO_SINKHORN_MAX_RADIUS                                 */
    int per_launch_reserved;   /* 0                                                               */
    double eps;                /* the kernel's variance in px^2, finite and > 0                   */
} foto_sinkhorn_opts;
/* eps 2, radius 16 */
int foto_sinkhorn_opts_default(foto_sinkhorn_opts* o);
typedef struct foto_sinkhorn foto_sinkhorn;
/* opts NULL: the defaults.  tables: the host [3][radius + 1] above, copied.  FOTO_SK_FUSED is read
 * here, once.                                                              */
int foto_sinkhorn_create(int w, int h, const foto_sinkhorn_opts* opts, const double* tables, foto_sinkhorn** out);
void foto_sinkhorn_destroy(foto_sinkhorn* c);
/* The two frames; a = 0, b = 1 and the iteration count 0 again. */
int foto_sinkhorn_set_frames_dev(foto_sinkhorn* c, const foto_image* f0, const foto_image* f1, void* stream);
/* n more iterations (n = 0: nothing), four launches each (two with FOTO_SK_FUSED=1). */
int foto_sinkhorn_iterate_dev(foto_sinkhorn* c, int n, void* stream);
/* out: a flow record as foto_flow describes it (dtype FOTO_F32 | FOTO_F64, layout 0 planar u, v, m
 * or 1 interleaved (u, v)); valid_or_null: uint8[h][w].                                          */
int foto_sinkhorn_flow_dev(foto_sinkhorn* c, int direction, void* out, int dtype, int layout,
                           unsigned char* valid_or_null, void* stream);
/* info8: DEVICE float64[8], the record. */
int foto_sinkhorn_info_dev(foto_sinkhorn* c, double* info8, void* stream);
/* a_out, b_out: DEVICE float64[h][w]. */
int foto_sinkhorn_scalings_dev(foto_sinkhorn* c, double* a_out, double* b_out, void* stream);
/* One shot: the frames set, n iterations, the forward flow.  Host arrays of w h float64 (waits for
 * the result), or device frames and a device flow record (does not). */
int foto_sinkhorn_solve(foto_sinkhorn* c, const double* f0, const double* f1, int n, double* u, double* v, double* m);
int foto_sinkhorn_solve_dev(foto_sinkhorn* c, const foto_image* f0, const foto_image* f1, int n, void* out, int dtype,
                            int layout, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FOTO_H */
