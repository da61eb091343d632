// The run-time knobs of libfoto, read from the environment once: when a
// BB context or a GN plan is built, or at the C entry of a call that has neither.  Everything
// below those points takes the values; nothing re-reads the environment under a live context
// (sharded ranks derive their collective sequences from these values, so they must not move).
// Two reads stay outside: FOTO_GQ_KLIM (a test hook, read per Gauss solve in foto_spectral.hip)
// and FOTO_GN_TRACE (stderr tracing, foto_gn.hip).
#pragma once

#include <climits>
#include <cstdlib>

namespace foto {

struct Tuning {
    static constexpr int AUTO = INT_MIN;   // "not set": the code's own rule decides

    // ---- BB context (foto_bb.cpp)
    bool fuse_pr = true;        // FOTO_FUSE_PR=0: separate k_prox / k_rhs
    bool pipe = true;           // FOTO_PIPE=0: one outer iteration in flight
    bool host_crit = true;      // FOTO_HOST_CRIT=0: crit pair and Gauss header by copy launches
    bool phase_ev = false;      // FOTO_PHASE_EV=1: phase events even without kernel timing
    bool cg_defer = true;       // FOTO_CG_DEFER=0: always wait for the solve before prox
    bool pr_edge = true;        // FOTO_PR_EDGE=0: sharded fused prox recomputes the neighbours' edge stepB
    int pr_tch = 16;            // FOTO_PR_TCH: planes per chunk of k_prox_rhs (<= 0: 16)
    long long cg_auto_max = 1LL << 18;   // FOTO_CG_AUTO_MAX: cg_mode < 0 takes the stencil CG up to this many voxels
    // sharding
    bool comm_stream = true;    // FOTO_COMM_STREAM=0: every RCCL call on the compute stream
    int a2a_parts = AUTO;       // FOTO_A2A_PARTS, clamped to 1..8; AUTO: by plane size (2 for >= 2^19 voxels, 1 below)
    int a2a_halo = AUTO;        // FOTO_A2A_HALO: 0 off, other on; AUTO: by plane size
    bool wt_overlap = true;     // FOTO_WT_OVERLAP=0: exchange w_t after k_prox_rhs
    bool wt_pre = false;        // FOTO_WT_PRE=1: virtual ranks run k_wt_pre as RCCL ranks do

    // ---- spectral plan (foto_spectral.hip, foto_dct.hip)
    bool ring = true;           // FOTO_RING=0: register-fed s-step pass
    bool tcol = true;           // FOTO_TCOL=0: t axis by dct_pass + separate INIT / xhat passes
    bool dct_fft = true;        // FOTO_DCT_FFT=0: GEMM kernels on every axis
    bool sadapt = true;         // FOTO_SADAPT=0: whole-spectrum interval for every pass
    bool gq_cgtab = true;       // FOTO_GQ_CGTAB=0: k_gq_cg, then k_gq_qtab
    int gq_exact = AUTO;        // FOTO_GQ_EXACT: largest exact bin (capped at GQ_XS); AUTO: GQ_M
    int cg_margin = 2;          // FOTO_CG_MARGIN: passes launched beyond the previous solve's count

    // ---- GN (foto_gn.hip, foto_capi.cpp)
    bool gn_mg = true;          // FOTO_GN_MG=0: block-Jacobi PCG instead of the multigrid plan
    bool gn_plan_cache = true;  // FOTO_GN_PLAN_CACHE=0: foto_gn_solve builds a plan per call
    bool gn_setup_fuse = true;  // FOTO_GN_SETUP_FUSE=0: B and block inverses in separate passes
    bool gn_recomp = true;      // FOTO_GN_RECOMP=0: level-0 legs load B, D^-1
    bool gn_exact = true;       // FOTO_GN_EXACT=0: whole graphs instead of the exact predicted count
    bool gn_fold = true;        // FOTO_GN_FOLD=0: k_gnp_upd not folded into the level-0 down leg
    bool mg_ltail = true;       // FOTO_MG_LTAIL=0: the three level kernels instead of k_mg_ltail
    int gn_host_threads = 4;    // FOTO_GN_HOST_THREADS: host copy workers, clamped to 0..16

    // ---- entropic transport (foto_sinkhorn.hip)
    bool sk_fused = false;      // FOTO_SK_FUSED=1: a half-iteration as one LDS-tiled launch, not a row + a column / divide kernel
};

// the one place that reads the environment: the value of `name` as an integer, dflt when unset
inline long long env_int(const char* name, long long dflt) {
    const char* e = getenv(name);
    return e ? atoll(e) : dflt;
}

inline Tuning tuning_from_env() {
    Tuning t;
    t.fuse_pr = env_int("FOTO_FUSE_PR", 1) != 0;
    t.pipe = env_int("FOTO_PIPE", 1) != 0;
    t.host_crit = env_int("FOTO_HOST_CRIT", 1) != 0;
    t.phase_ev = env_int("FOTO_PHASE_EV", 0) == 1;
    t.cg_defer = env_int("FOTO_CG_DEFER", 1) != 0;
    t.pr_edge = env_int("FOTO_PR_EDGE", 1) != 0;
    t.pr_tch = (int)env_int("FOTO_PR_TCH", 16);
    if (t.pr_tch <= 0) t.pr_tch = 16;
    t.cg_auto_max = env_int("FOTO_CG_AUTO_MAX", 1LL << 18);
    t.comm_stream = env_int("FOTO_COMM_STREAM", 1) != 0;
    t.a2a_parts = (int)env_int("FOTO_A2A_PARTS", Tuning::AUTO);
    t.a2a_halo = (int)env_int("FOTO_A2A_HALO", Tuning::AUTO);
    t.wt_overlap = env_int("FOTO_WT_OVERLAP", 1) != 0;
    t.wt_pre = env_int("FOTO_WT_PRE", 0) == 1;
    t.ring = env_int("FOTO_RING", 1) != 0;
    t.tcol = env_int("FOTO_TCOL", 1) != 0;
    t.dct_fft = env_int("FOTO_DCT_FFT", 1) != 0;
    t.sadapt = env_int("FOTO_SADAPT", 1) != 0;
    t.gq_cgtab = env_int("FOTO_GQ_CGTAB", 1) != 0;
    t.gq_exact = (int)env_int("FOTO_GQ_EXACT", Tuning::AUTO);
    t.cg_margin = (int)env_int("FOTO_CG_MARGIN", 2);
    t.gn_mg = env_int("FOTO_GN_MG", 1) != 0;
    t.gn_plan_cache = env_int("FOTO_GN_PLAN_CACHE", 1) != 0;
    t.gn_setup_fuse = env_int("FOTO_GN_SETUP_FUSE", 1) != 0;
    t.gn_recomp = env_int("FOTO_GN_RECOMP", 1) != 0;
    t.gn_exact = env_int("FOTO_GN_EXACT", 1) != 0;
    t.gn_fold = env_int("FOTO_GN_FOLD", 1) != 0;
    t.mg_ltail = env_int("FOTO_MG_LTAIL", 1) != 0;
    t.gn_host_threads = (int)env_int("FOTO_GN_HOST_THREADS", 4);
    t.gn_host_threads = t.gn_host_threads < 0 ? 0 : t.gn_host_threads > 16 ? 16 : t.gn_host_threads;
    t.sk_fused = env_int("FOTO_SK_FUSED", 0) != 0;
    return t;
}

}  // namespace foto
