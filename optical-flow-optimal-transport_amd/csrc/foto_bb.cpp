// libfoto host side: the Benamou-Brenier solver context, the device-resident CG driver,
// time-slab sharding (RCCL across processes, or in-process virtual ranks on one device
// for testing the sharded path), and the BB part of the C ABI (include/foto.h).
//
// Reference: benamou_brenier.solve (benamou_brenier.py:151-271).  One outer iteration =
//   stepA: F = div_st(mu - r q) + BC (k_rhs), phi = cg(A, F) (k_cg_dir / k_cg_upd loop)
//   stepB: q = Proj_K(grad_st phi + mu / r); stepC: mu += r (grad phi - q), mu_rho >= 0;
//   crit = sqrt(num / (den + 1e-10))  (all fused in k_prox)
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <memory>
#include <utility>

#include "foto_devmem.h"
#include "foto_internal.h"
#include "foto_spectral.h"
#include "foto_xfer.h"

namespace foto {

#define FOTO_NCCL_CHECK(call)                                                                 \
    do {                                                                                     \
        ncclResult_t r_ = (call);                                                            \
        if (r_ != ncclSuccess) {                                                             \
            ::foto::set_error("%s:%d %s: %s", __FILE__, __LINE__, #call, ncclGetErrorString(r_)); \
            return FOTO_ERR_COMM;                                                            \
        }                                                                                    \
    } while (0)

// ----------------------------------------------------------------------------- shards

// The pointers an outer iteration rotates: which buffer holds the current mu, phi and the fused
// prox's pair.  One record, so the snapshot an enqueued iteration keeps (foto_bb_ctx::Enq), the
// rollback that restores it and the completed iteration's state the exports read (Completed) are
// whole-record assignments: a pointer added here is in all of them.
// (fields: halo-padded planes (l = -1 .. nloc), pointers at local plane 0)
struct Rot {
    double* mu[3] = {nullptr, nullptr, nullptr};
    double* nu[3] = {nullptr, nullptr, nullptr};   // second mu buffer of the fused prox + RHS
    double* xi[3] = {nullptr, nullptr, nullptr};   // third mu buffer (two outer iterations in flight)
    double* phi = nullptr;   // CG iterate x (two halo planes per side: the fused prox reads them)
    double* phi_alt = nullptr;   // the other phi of the pipelined loop
    // the last fused prox + RHS launch's mu in / out (fz_src is the mu stepB of phi used)
    double* fz_src[3] = {nullptr, nullptr, nullptr};
    double* fz_dst[3] = {nullptr, nullptr, nullptr};
};

struct Shard : Rot {
    Geo g{};
    int rank = 0;
    Rot& rot() { return *this; }
    double* q[3] = {nullptr, nullptr, nullptr};
    // sharded fused prox with deferred edges: w_t next to the slab edges (halo-padded) and the
    // edge planes' (w_x, w_y, mu'_t, q_t), slot 0 = plane 0, slot 1 = plane nloc - 1
    double* wt = nullptr;
    double* edge = nullptr;
    double* rv = nullptr;    // CG residual (starts as F)
    double* p[2] = {nullptr, nullptr};
    double* rho0 = nullptr;
    double* rhoT = nullptr;
    double* px = nullptr;    // trajectory positions
    double* py = nullptr;
    double* fu = nullptr;    // flow output (last rank)
    double* fv = nullptr;
    double* fm = nullptr;
    RedBuf rb{};
    double* gath = nullptr;  // [0,W) rr | [W,2W) pap | [2W,4W) crit num/den
    CGScal* S = nullptr;
    // the buffers a new context starts from zero in, as allocated: foto_bb_reset zeroes this list
    // again (rezero), so it cannot miss one
    std::vector<std::pair<void*, size_t>> zeroed;   // (base, bytes)
    std::unique_ptr<SpectralPlan> spec;
    DevArena mem;   // declared after spec: the shard's blocks are freed before the plan goes

    double* gath_rr() { return gath; }
    double* gath_pap(int W) { return gath + W; }
    double* gath_crit(int W) { return gath + 2 * W; }

    template <class T>
    int alloc(size_t bytes, T** out) {
        return mem.alloc(bytes, (void**)out);
    }
    // zeroed on the context's stream: a hipMemset (null stream) is not ordered with the
    // non-blocking stream the kernels run on -- it raced with k_init_mu
    template <class T>
    int alloc_zeroed(size_t bytes, T** out, hipStream_t st) {
        FOTO_TRY(alloc(bytes, out));
        FOTO_HIP_CHECK(hipMemsetAsync(*out, 0, bytes, st));
        zeroed.push_back({*out, bytes});
        return 0;
    }
    // (nloc + 2 h) planes (h halo planes per side)
    int alloc_field(double** out, hipStream_t st, int h = 1) {
        FOTO_TRY(alloc_zeroed((size_t)(g.nloc + 2 * h) * (size_t)g.nxy * sizeof(double), out, st));
        *out += (size_t)h * g.nxy;
        return 0;
    }
    int rezero(hipStream_t st) {
        for (const auto& z : zeroed) FOTO_HIP_CHECK(hipMemsetAsync(z.first, 0, z.second, st));
        return 0;
    }
};

}  // namespace foto

using namespace foto;

// ----------------------------------------------------------------------------- context

struct foto_bb_ctx {
    int Nt = 0, Nx = 0, Ny = 0;
    double r = 1, eps = 1e-3;
    foto_bb_opts o{};
    Tuning tn;            // the environment's knobs as bb_create found them: fixed for the context's life
    int W = 1;            // total ranks (processes * virtual)
    bool rccl = false;
    ncclComm_t nc = nullptr;
    hipStream_t s = nullptr;
    // RCCL: every collective and send / receive group goes on its own stream, ordered against
    // the compute stream s by events (comm_fork / comm_join), so a group can travel while s
    // transforms the next part of the slab (the pipelined all-to-alls below)
    hipStream_t sc = nullptr;
    hipEvent_t cfork = nullptr, cjoin = nullptr;
    hipEvent_t cpart[8] = {};      // the backward all-to-all's parts, landed
    bool phi_halo = false;         // phi's halo planes came with the backward all-to-all
    // the w_t halo of the deferred slab edges, issued on sc before k_prox_rhs (wt_overlap); the
    // next forward finishes the edge planes' F (k_rhs_edge) from it
    bool wt_pending = false;       // issued on sc by prox_rhs, not yet consumed
    bool wt_guarded = false;       // (the prox it belongs to was launched behind a solve's done flag)
    std::vector<std::unique_ptr<Shard>> sh;   // local shards
    CGScal* hS = nullptr;                     // pinned host mirror of shard 0's CG scalars
    int last_cg = 0;
    int have_phi = 0;
    // prox fused with the next RHS (k_prox_rhs); F in rv is then produced by the previous
    // outer iteration (f_ready), mu rotates through Shard::mu / nu (/ xi)
    bool fuse = false;
    bool f_ready = false;
    // Two outer iterations in flight (single shard, fused, Gauss CG; FOTO_PIPE=0: one): the
    // host enqueues iteration i + 1 before it waits for iteration i's crit, so the GPU never
    // idles while the host wakes up and launches.  mu rotates through three buffers and phi
    // alternates between two, so an iteration the stop rules turn out not to want is dropped
    // (rollback) with iteration i's state intact; a failed Gauss solve is redone after its
    // successor, which its done-flag chain kept from touching the state, is dropped.
    bool pipe = false;
    struct Enq {            // an outer iteration on the stream (outer_tail -> outer_complete)
        int par = 0;        // its event / readback slot
        SpectralPlan* dsp = nullptr;   // deferred solve to finish (single shard)
        bool sdefer = false;           // sharded Gauss solve enqueued without a host wait
        int its = 0, info = 0;         // a synchronous solve's result
        size_t kmark = 0;              // KTimer mark before its launches
        // host state before it (restored by a rollback)
        Rot before;                    // shard 0's rotating pointers
        bool f_ready;
        int hpar;
        bool pev;                      // phase events recorded (ph[par][0..3])
    };
    std::vector<Enq> inflight;   // oldest first
    // an iterate call failed with iterations on the stream: they were drained (drain_inflight),
    // the host state no longer matches the device's, so only foto_bb_reset brings it back
    bool broken = false;
    // inside foto_bb_iterate (its callback runs with iterations on the stream): reset and a
    // nested iterate are refused there instead of resetting state under the running loop
    bool in_iterate = false;
    // bookkeeping
    double prev_crit = -1;
    foto_bb_stats st{};
    KTimer kt;
    hipEvent_t ph[2][4] = {};      // per slot: RHS start | CG start | prox start | crit readback
    hipEvent_t fin[2] = {};        // per slot: crit readback without timing (phase events off)
    hipEvent_t fl[2] = {};         // flow extraction
    double* hgath[2] = {nullptr, nullptr};   // pinned host mirrors of gath, per slot
    double* dgath[2] = {nullptr, nullptr};   // their device addresses (coherent host memory)
    bool hcrit = false;            // single shard, fused prox: the kernel writes crit to hgath itself
    bool phase_force = false;      // FOTO_PHASE_EV=1: phase events even without kernel timing
    int hpar = 0;                  // slot of the last head
    // device-buffer entries (foto_bb_*_dev): the events that order the caller's stream with s,
    // and the scratch of normalize = 1 ({S0, ST, block partials}, made on first use)
    StreamLink link;
    double* nrm = nullptr;
    double hsum[2] = {0, 0};
    // point tracking (foto_bb_track / _dev), grow-only device scratch: the host entry's staged
    // points [M][2] and records [R][M][2], and the running float64 positions [M][2] that travel
    // between the launches of a path whose planes lie in several shards (virtual ranks)
    enum { TRK_PTS = 0, TRK_OUT = 1, TRK_POS = 2 };
    DevScratch trk[3];
    // the transport report (foto_bb_report / _dev), grow-only, made on first use: the host entry's
    // staged table [Nt][8] | the plane partials [Nt][8][pieces] | Nt tickets (zero between launches)
    DevScratch rep;
    // maps and in-betweens (foto_bb_maps / _dev, foto_bb_interp_dev), grow-only, made on first use:
    // the table of Nt phi plane pointers, rebuilt by every call from the completed iteration's
    // state, and the host entry's staged records [count][4][Ny][Nx]
    enum { ITP_TAB = 0, ITP_OUT = 1 };
    DevScratch itp[2];
    ~foto_bb_ctx() {
        if (sc) (void)hipStreamSynchronize(sc);
        if (s) (void)hipStreamSynchronize(s);   // (before the shards free their buffers)
        sh.clear();
        for (DevScratch& b : trk) if (b.p) (void)hipFree(b.p);
        if (rep.p) (void)hipFree(rep.p);
        for (DevScratch& b : itp) if (b.p) (void)hipFree(b.p);
        if (nc) (void)ncclCommDestroy(nc);
        if (hS) (void)hipHostFree(hS);
        for (double* h : hgath) if (h) (void)hipHostFree(h);
        for (auto& p : ph)
            for (auto e : p) if (e) (void)hipEventDestroy(e);
        for (auto e : fl) if (e) (void)hipEventDestroy(e);
        for (auto e : fin) if (e) (void)hipEventDestroy(e);
        for (auto e : {cfork, cjoin}) if (e) (void)hipEventDestroy(e);
        for (auto e : cpart) if (e) (void)hipEventDestroy(e);
        if (sc) {
            (void)hipStreamSynchronize(sc);
            stream_release(sc);
        }
        if (s) {
            (void)hipStreamSynchronize(s);
            stream_release(s);
        }
    }
};

namespace foto {

// ----------------------------------------------------------------------------- communication
// Every exchange between shards is a list of point-to-point transfers (foto_xfer.h), built by
// the same code on every rank and for every transport; only its execution differs:
//   virtual ranks (one process, all shards on one device and stream): one device copy per
//   transfer, in list order;
//   RCCL (one shard per process): the calls rccl_calls() lists -- in one group, ncclSend for
//   each transfer from this rank and ncclRecv for each transfer to it (pairs match in list
//   order, which is the same on every rank), then a device copy for each transfer to itself.
// Offsets are in doubles from the pointer a picker returns for the shard (negative: the halo
// plane below).  The virtual-rank GPU tests therefore run the very lists RCCL executes, and
// tests/test_xfer.py checks the RCCL call sequences of every rank against each other.
// compute stream -> communication stream: what s has enqueued so far happens before what sc
// runs next (RCCL only; virtual ranks run everything on s)
static int comm_fork(foto_bb_ctx* c) {
    if (!c->sc) return 0;
    FOTO_HIP_CHECK(hipEventRecord(c->cfork, c->s));
    FOTO_HIP_CHECK(hipStreamWaitEvent(c->sc, c->cfork, 0));
    return 0;
}
// communication stream -> compute stream
static int comm_join(foto_bb_ctx* c) {
    if (!c->sc) return 0;
    FOTO_HIP_CHECK(hipEventRecord(c->cjoin, c->sc));
    FOTO_HIP_CHECK(hipStreamWaitEvent(c->s, c->cjoin, 0));
    return 0;
}

// one list, issued on the communication stream (RCCL) or as copies on s (virtual ranks); the
// caller orders it against s (exchange() below does, the pipelined all-to-alls do per part)
template <class SrcPick, class DstPick>
static int exchange_raw(foto_bb_ctx* c, const std::vector<Xfer>& xs, SrcPick sp, DstPick dp) {
    if (!c->rccl) {
        for (const Xfer& x : xs)
            FOTO_HIP_CHECK(hipMemcpyAsync(dp(*c->sh[x.dst]) + x.doff, sp(*c->sh[x.src]) + x.soff,
                                          (size_t)x.n * sizeof(double), hipMemcpyDeviceToDevice, c->s));
        return 0;
    }
    hipStream_t st = c->sc ? c->sc : c->s;
    Shard& s = *c->sh[0];
    const std::vector<Call> cs = rccl_calls(xs, s.rank);
    const bool grouped = !cs.empty() && cs.front().op != CALL_COPY;
    if (grouped) FOTO_NCCL_CHECK(ncclGroupStart());
    bool open = grouped;
    for (const Call& k : cs) {
        if (k.op == CALL_COPY && open) {
            FOTO_NCCL_CHECK(ncclGroupEnd());
            open = false;
        }
        if (k.op == CALL_SEND)
            FOTO_NCCL_CHECK(ncclSend(sp(s) + k.off, (size_t)k.n, ncclDouble, k.peer, c->nc, st));
        else if (k.op == CALL_RECV)
            FOTO_NCCL_CHECK(ncclRecv(dp(s) + k.off, (size_t)k.n, ncclDouble, k.peer, c->nc, st));
        else
            FOTO_HIP_CHECK(hipMemcpyAsync(dp(s) + k.doff, sp(s) + k.off, (size_t)k.n * sizeof(double),
                                          hipMemcpyDeviceToDevice, st));
    }
    if (open) FOTO_NCCL_CHECK(ncclGroupEnd());
    return 0;
}

template <class SrcPick, class DstPick>
static int exchange(foto_bb_ctx* c, const std::vector<Xfer>& xs, SrcPick sp, DstPick dp) {
    FOTO_TRY(comm_fork(c));
    FOTO_TRY(exchange_raw(c, xs, sp, dp));
    return comm_join(c);
}

// each rank's `cnt` doubles at slot [rank] of the picked array to every rank's same slot
// (RCCL: one ncclAllGather, in place; virtual ranks: the equivalent copies)
template <class Pick>
static int allgather(foto_bb_ctx* c, Pick pick, int cnt) {
    if (c->W == 1) return 0;
    if (c->rccl) {
        Shard& s = *c->sh[0];
        double* base = pick(s);
        FOTO_TRY(comm_fork(c));
        FOTO_NCCL_CHECK(ncclAllGather(base + (size_t)s.rank * cnt, base, cnt, ncclDouble, c->nc, c->sc ? c->sc : c->s));
        return comm_join(c);
    }
    return exchange(c, allgather_xfers(c->W, cnt), pick, pick);
}

template <class Pick>
static int halo(foto_bb_ctx* c, Pick pick) {
    if (c->W == 1) return 0;
    return exchange(c, halo_xfers(c->Nt, (int64_t)c->Nx * c->Ny, c->W), pick, pick);
}

// ----------------------------------------------------------------------------- context setup

// Where a context's two densities come from: the caller's host arrays (foto_bb_create / reset),
// or two device images (foto_bb_create_dev / reset_dev).  The two uploads are the only
// difference between the entries: everything around load_rho is shared, so the state it leaves
// is the one the host entries leave for rho = (double)pixel / divisor.
struct RhoSrc {
    const double* h0 = nullptr;
    const double* hT = nullptr;
    const foto_image* i0 = nullptr;
    const foto_image* iT = nullptr;
    int normalize = 0;
    hipStream_t user = nullptr;
};

static int load_rho(foto_bb_ctx* c, Shard& s, const RhoSrc& src) {
    const int64_t nxy = (int64_t)c->Nx * c->Ny;
    if (!src.i0) {
        FOTO_HIP_CHECK(hipMemcpyAsync(s.rho0, src.h0, nxy * sizeof(double), hipMemcpyHostToDevice, c->s));
        FOTO_HIP_CHECK(hipMemcpyAsync(s.rhoT, src.hT, nxy * sizeof(double), hipMemcpyHostToDevice, c->s));
        return 0;
    }
    if (!c->sh.empty() && c->sh[0].get() != &s) {   // (virtual ranks: every further shard gets its copy)
        FOTO_HIP_CHECK(hipMemcpyAsync(s.rho0, c->sh[0]->rho0, nxy * sizeof(double), hipMemcpyDeviceToDevice, c->s));
        FOTO_HIP_CHECK(hipMemcpyAsync(s.rhoT, c->sh[0]->rhoT, nxy * sizeof(double), hipMemcpyDeviceToDevice, c->s));
        return 0;
    }
    FOTO_TRY(c->link.enter(src.user, c->s));   // (before the first read of an input)
    FOTO_HIP_CHECK(launch_ingest(*src.i0, c->Nx, c->Ny, s.rho0, c->s));
    FOTO_HIP_CHECK(launch_ingest(*src.iT, c->Nx, c->Ny, s.rhoT, c->s));
    if (src.normalize) {   // each frame over its own sum (main.py:71-74), the sum in a fixed order
        if (!c->nrm) {
            FOTO_TRY(s.alloc(sizeof(double) * (2 + (size_t)capped_blocks(nxy, SUM_MAX_BLOCKS)), &c->nrm));
        }
        double* const rho[2] = {s.rho0, s.rhoT};
        for (int k = 0; k < 2; ++k) {
            FOTO_HIP_CHECK(launch_sum(nxy, rho[k], c->nrm + 2, c->nrm + k, c->s));
            FOTO_HIP_CHECK(launch_div_scalar(nxy, rho[k], c->nrm + k, c->s));
        }
        FOTO_HIP_CHECK(hipMemcpyAsync(c->hsum, c->nrm, 2 * sizeof(double), hipMemcpyDeviceToHost, c->s));
    }
    return 0;
}

// what ctx_init and bb_reset end a shard's setup with: the densities, then mu and q from them
static int init_fields(foto_bb_ctx* c, Shard& s, const RhoSrc& src) {
    FOTO_TRY(load_rho(c, s, src));
    FOTO_HIP_CHECK(launch_init_mu(s.g, s.rho0, s.rhoT, s.mu[0], s.mu[1], s.mu[2], s.q[0], s.q[1], s.q[2], c->s));
    return 0;
}

// the _dev entries' source, and what they do once the context's stream has read it (create and
// reset both end with a stream synchronise: the sums are on the host)
static RhoSrc dev_src(const foto_image* f0, const foto_image* f1, int normalize, void* stream) {
    RhoSrc src;
    src.i0 = f0;
    src.iT = f1;
    src.normalize = normalize != 0;
    src.user = (hipStream_t)stream;
    return src;
}
static int dev_src_done(foto_bb_ctx* c, const RhoSrc& src, double* sums2_or_null) {
    FOTO_TRY(c->link.leave(c->s, src.user));
    if (sums2_or_null) {
        sums2_or_null[0] = src.normalize ? c->hsum[0] : 1.0;
        sums2_or_null[1] = src.normalize ? c->hsum[1] : 1.0;
    }
    return 0;
}

static int ctx_init(foto_bb_ctx* c, const RhoSrc& src) {
    const int64_t nxy = (int64_t)c->Nx * c->Ny;
    if (c->o.device >= 0) FOTO_HIP_CHECK(hipSetDevice(c->o.device));
    FOTO_TRY(stream_acquire(&c->s));
    FOTO_HIP_CHECK(hipHostMalloc((void**)&c->hS, sizeof(CGScal)));
    const int W = c->W;
    for (int k = 0; k < 2; ++k) {
        FOTO_HIP_CHECK(hipHostMalloc((void**)&c->hgath[k], sizeof(double) * 4 * W,
                                     hipHostMallocMapped | hipHostMallocCoherent));
        FOTO_HIP_CHECK(hipHostGetDevicePointer((void**)&c->dgath[k], c->hgath[k], 0));
    }
    for (auto& p : c->ph)
        for (int k = 0; k < 4; ++k)   // (phase boundaries: timing only; the crit event keeps the fence)
            FOTO_HIP_CHECK(hipEventCreateWithFlags(&p[k], k < 3 ? hipEventDisableSystemFence : hipEventDefault));
    for (auto& e : c->fl) FOTO_HIP_CHECK(hipEventCreate(&e));
    if (c->rccl) {
        ncclUniqueId id;
        memcpy(&id, c->o.nccl_id, sizeof(id));
        FOTO_NCCL_CHECK(ncclCommInitRank(&c->nc, W, id, c->o.rank));
        // FOTO_COMM_STREAM=0: every RCCL call on the compute stream (A/B runs)
        if (c->tn.comm_stream) {
            FOTO_TRY(stream_acquire(&c->sc));
            FOTO_HIP_CHECK(hipEventCreateWithFlags(&c->cfork, hipEventDisableTiming));
            FOTO_HIP_CHECK(hipEventCreateWithFlags(&c->cjoin, hipEventDisableTiming));
            for (auto& e : c->cpart) FOTO_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
    }
    const int nlocal = c->rccl ? 1 : W;
    {
        Geo plane{};
        plane.Nx = c->Nx;
        // FOTO_FUSE_PR=0: separate k_prox / k_rhs (A/B runs; rows beyond the fused kernel's offsets)
        c->fuse = c->tn.fuse_pr && prox_rhs_fits(plane);
        // FOTO_PIPE=0: one outer iteration in flight (A/B runs)
        c->pipe = W == 1 && c->fuse && c->o.cg_mode == 3 && c->tn.pipe;
        // the crit readback as two stores of k_prox_rhs's last block into the slot (a copy launch
        // on the stream costs ~4 us; FOTO_HOST_CRIT=0: the copy)
        // phase events (the RHS / CG / prox split of foto_bb_stats) only with kernel timing on:
        // three timed event records per outer iteration cost ~13 us of GPU time at the bench
        // grid (1561-1572 vs 1603-1616 it/s, same box), and the crit sync uses a timing-free one
        c->phase_force = c->tn.phase_ev;
        c->hcrit = W == 1 && c->fuse && c->tn.host_crit;
        // the crit sync: with the crit pair and the Gauss header stored into coherent host memory
        // by the kernels themselves (fenced there), the event needs no system-scope fence of its
        // own -- a fenced record writes the L2's dirty lines back once per outer iteration
        const unsigned ff = c->hcrit ? hipEventDisableSystemFence : 0u;
        for (auto& e : c->fin) FOTO_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming | ff));
    }
    for (int j = 0; j < nlocal; ++j) {
        auto sp = std::make_unique<Shard>();
        Shard& s = *sp;
        s.rank = c->rccl ? c->o.rank : j;
        s.g.Nt = c->Nt; s.g.Ny = c->Ny; s.g.Nx = c->Nx; s.g.nxy = nxy;
        if (split_planes(c->Nt, W, s.rank, &s.g.t0, &s.g.nloc) != 0) {
            set_error("world size %d exceeds Nt = %d (each rank needs >= 1 time slab)", W, c->Nt);
            return FOTO_ERR_ARG;
        }
        for (int f = 0; f < 3; ++f) { FOTO_TRY(s.alloc_field(&s.mu[f], c->s)); FOTO_TRY(s.alloc_field(&s.q[f], c->s)); }
        if (c->fuse)
            for (int f = 0; f < 3; ++f) FOTO_TRY(s.alloc_field(&s.nu[f], c->s));
        if (c->pipe) {
            for (int f = 0; f < 3; ++f) FOTO_TRY(s.alloc_field(&s.xi[f], c->s));
            FOTO_TRY(s.alloc_field(&s.phi_alt, c->s, 2));
        }
        if (c->fuse && W > 1) {
            FOTO_TRY(s.alloc_field(&s.wt, c->s));
            FOTO_TRY(s.alloc_zeroed(sizeof(double) * 8 * nxy, &s.edge, c->s));
        }
        FOTO_TRY(s.alloc_field(&s.phi, c->s, 2));
        FOTO_TRY(s.alloc_field(&s.rv, c->s));
        FOTO_TRY(s.alloc_field(&s.p[0], c->s));
        FOTO_TRY(s.alloc_field(&s.p[1], c->s));
        for (double** plane : {&s.rho0, &s.rhoT, &s.px, &s.py, &s.fu, &s.fv, &s.fm})
            FOTO_TRY(s.alloc(nxy * sizeof(double), plane));
        const int64_t nb = std::max<int64_t>(march_blocks(s.g), flat_blocks((int64_t)s.g.nloc * nxy));
        s.rb.cap = (int)std::max<int64_t>(2 * nb, 3 * (int64_t)prox_rhs_blocks(s.g, c->tn.pr_tch));
        FOTO_TRY(s.alloc(sizeof(double) * s.rb.cap, &s.rb.partials));
        FOTO_TRY(s.alloc_zeroed(sizeof(unsigned) * 64, &s.rb.ticket, c->s));
        FOTO_TRY(s.alloc_zeroed(sizeof(double) * 4 * W, &s.gath, c->s));
        FOTO_TRY(s.alloc_zeroed(sizeof(CGScal), &s.S, c->s));
        FOTO_TRY(init_fields(c, s, src));
        if (c->o.cg_mode >= 1 && c->o.cg_mode <= 3) {
            s.spec.reset(new SpectralPlan());
            FOTO_TRY(s.spec->init(s.g, s.rank, W, c->r, c->eps, c->o.cg_mode, c->tn, c->s));
        }
        c->sh.push_back(std::move(sp));
    }
    // the Gauss CG may fall back to the s-step CG for boxes its voxel list cannot pack
    if (c->pipe && !(c->sh[0]->spec && c->sh[0]->spec->gauss())) c->pipe = false;
    FOTO_HIP_CHECK(hipStreamSynchronize(c->s));
    return 0;
}

// ----------------------------------------------------------------------------- CG driver

static CGArgs cg_args(foto_bb_ctx* c, const Shard& s) {
    CGArgs a;
    a.r = c->r;
    a.eps = c->eps;
    a.rtol = c->o.cg_rtol;
    a.world = c->W;
    a.rank = s.rank;
    return a;
}

static int cg_iteration(foto_bb_ctx* c, int k) {
    const int W = c->W;
    const bool fused = (W == 1);
    if (!fused)
        for (auto& sp : c->sh) {
            Shard& s = *sp;
            FOTO_HIP_CHECK(launch_cg_pupd(s.g, k, s.rv, s.p[k & 1], s.p[(k + 1) & 1], s.S, s.gath_rr(), cg_args(c, s),
                                          c->s));
        }
    if (!fused) FOTO_TRY(halo(c, [k](Shard& s) { return s.p[(k + 1) & 1]; }));
    for (auto& sp : c->sh) {
        Shard& s = *sp;
        const CGArgs a = cg_args(c, s);
        const double nv = (double)s.g.nloc * (double)s.g.nxy;
        hipEvent_t e = c->kt.start(c->s);
        FOTO_HIP_CHECK(launch_cg_dir(s.g, k, s.rv, s.p[k & 1], s.p[(k + 1) & 1], a, s.S, s.rb, s.gath_rr(),
                                     s.gath_pap(W), fused ? 1 : 0, c->s));
        c->kt.stop(e, c->s, FOTO_K_CG_DIR, fused ? (k == 0 ? 16.0 : 24.0) * nv : 8.0 * nv);
    }
    FOTO_TRY(allgather(c, [W](Shard& s) { return s.gath_pap(W); }, 1));
    for (auto& sp : c->sh) {
        Shard& s = *sp;
        const CGArgs a = cg_args(c, s);
        const double nv = (double)s.g.nloc * (double)s.g.nxy;
        hipEvent_t e = c->kt.start(c->s);
        FOTO_HIP_CHECK(launch_cg_upd(s.g, k, s.p[(k + 1) & 1], s.phi, s.rv, a, s.S, s.rb, s.gath_pap(W),
                                     s.gath_rr(), c->s));
        c->kt.stop(e, c->s, FOTO_K_CG_UPD, (k == 0 ? 32.0 : 40.0) * nv);
    }
    FOTO_TRY(allgather(c, [](Shard& s) { return s.gath_rr(); }, 1));
    return 0;
}

// The slab <-> row-box all-to-alls (foto_xfer.h), pipelined in parts: the forward one sends a
// part of every slab once its x / y DCTs have run, while the compute stream transforms the next
// part; the backward one lands in parts and each part's inverse y / x DCTs start as soon as it
// is in, while the next part travels.  The backward one also delivers phi's halo planes (a2a_halo)
// -- rows of the neighbours' boundary planes from every box owner, over all links, transformed
// here with the own planes -- so the fused prox + RHS needs no separate one-plane phi exchange
// over the single link to each neighbour.  Virtual ranks run the same lists as copies on s.
// Both pay off where a plane is large against the compute it adds (two planes of inverse x / y
// DCT for the halo, twice the DCT launches for two parts): by default they are on for planes of
// >= 2^19 voxels (C4's 1024 x 1024: 8.4 MB per plane, 131 us over one link; 2 parts, the halo
// inside) and off below (the bench grid's 640 x 480: 2.5 MB, where the compute-only proxy gave
// 0.337 against 0.300 ms per rank at W = 8 with them on, profiles/r05_proxy_scaling.txt).
// FOTO_A2A_PARTS (1..8) and FOTO_A2A_HALO (0 / 1) override (A/B runs, tests).
static bool a2a_big_planes(const foto_bb_ctx* c) { return (int64_t)c->Nx * c->Ny >= (1 << 19); }

static int a2a_parts(const foto_bb_ctx* c) {
    const int v = c->tn.a2a_parts != Tuning::AUTO ? c->tn.a2a_parts : (a2a_big_planes(c) ? 2 : 1);
    return std::max(1, std::min(8, v));
}

static int a2a_halo(const foto_bb_ctx* c) {
    if (c->W == 1) return 0;
    if (c->tn.a2a_halo != Tuning::AUTO ? c->tn.a2a_halo == 0 : !a2a_big_planes(c)) return 0;
    // the deferred-edge fused prox (and the unfused prox) read one phi halo plane per side; the
    // edge-recompute variant (FOTO_PR_EDGE=0) reads two and keeps its own exchange
    return (c->fuse && !c->tn.pr_edge) ? 0 : 1;
}

// F on the deferred edge planes of every local shard, from its w_t halo (k_rhs_edge)
static int wt_edges(foto_bb_ctx* c, bool guarded) {
    for (auto& sp : c->sh) {
        Shard& s = *sp;
        const int dlo = s.g.t0 > 0, dhi = s.g.t0 + s.g.nloc < c->Nt;
        double* rr = c->o.cg_mode == 0 ? s.gath_rr() + s.rank : nullptr;
        const int* gd = guarded ? s.spec->done_flag() : nullptr;
        if (dlo)
            FOTO_HIP_CHECK(launch_rhs_edge(s.g, 0, s.wt, s.edge, s.rho0, s.rhoT, c->r, s.rv, s.rb, rr, c->s, gd));
        if (dhi && !(dlo && s.g.nloc == 1))
            FOTO_HIP_CHECK(launch_rhs_edge(s.g, s.g.nloc - 1, s.wt, s.edge + 4 * s.g.nxy, s.rho0, s.rhoT, c->r, s.rv,
                                           s.rb, rr, c->s, gd));
    }
    return 0;
}

// (round 5) the w_t exchange overlapped with k_prox_rhs: k_wt_pre computes the edge planes' w_t
// first, the exchange travels on the communication stream while k_prox_rhs runs, and the next
// forward finishes the edge planes' F (k_rhs_edge) before transforming them.  RCCL on its own
// stream, a spectral CG (the stencil CG needs F.F at once), slabs of >= 3 planes;
// FOTO_WT_OVERLAP=0: exchange and finish the edges after k_prox_rhs
static bool slabs_of_3(const foto_bb_ctx* c) {
    // all ranks decide alike (the call sequences stay identical whichever way, tests/test_xfer.py),
    // so the rule rests on the smallest slab of the split
    for (int r = 0; r < c->W; ++r) {
        int t0 = 0, nl = 0;
        if (split_planes(c->Nt, c->W, r, &t0, &nl) != 0 || nl < 3) return false;
    }
    return true;
}
static bool wt_overlap(const foto_bb_ctx* c) {
    return c->rccl && c->sc && c->o.cg_mode != 0 && c->sh.size() == 1 && slabs_of_3(c) && c->tn.wt_overlap;
}

// k_wt_pre ahead of k_prox_rhs: RCCL where wt_overlap holds; virtual ranks with FOTO_WT_PRE=1
// (the same kernel sequence, exchanged by copies on s -- tests, tools/proxy_scaling.py)
static bool wt_pre_on(const foto_bb_ctx* c) {
    if (c->rccl) return wt_overlap(c);
    return c->W > 1 && c->o.cg_mode != 0 && c->tn.wt_pre && slabs_of_3(c);
}

// a w_t exchange that no forward will consume (a new prox supersedes it): forget or wait for it
static int wt_drop(foto_bb_ctx* c) {
    if (!c->wt_pending) return 0;
    c->wt_pending = false;
    return comm_join(c);
}

// Spectral CG over time-slab shards, in phases: x/y DCTs on the own planes, all-to-all to row
// boxes and the t-DCT (sharded_fwd); the Gauss-compressed CG -- one all-gather of the boxes'
// histograms, summed in rank order on every rank, and the small serial solve on every rank
// (sharded_gauss) -- or the s-step CG from b^ with one NACC-double all-gather per pass (moments
// summed in rank order, so all ranks plan identically; sharded_sstep); then x^, the inverse
// t-DCT, the all-to-all back and the inverse x/y DCTs (sharded_inv).
static int sharded_fwd(foto_bb_ctx* c) {
    KTimer* kt = &c->kt;
    const int parts = a2a_parts(c);
    // the slab side is the shard's RHS buffer: fwd_local leaves the x / y DCTs of F there
    auto sbuf = [](Shard& s) { return s.rv; };
    auto rbuf = [](Shard& s) { return s.spec->box_in(); };
    // w_t exchanged behind k_prox_rhs (wt_overlap; landed by now: the crit all-gather queued
    // behind it on sc was joined): the edge planes' F before their x / y DCTs
    if (c->wt_pending) {
        FOTO_TRY(comm_join(c));
        c->wt_pending = false;
        FOTO_TRY(wt_edges(c, c->wt_guarded));
    }
    for (int p = 0; p < parts; ++p) {
        for (auto& sp : c->sh) {
            int lo, hi;
            split_part(sp->g.nloc, parts, p, &lo, &hi);
            if (hi > lo) FOTO_TRY(sp->spec->fwd_local(sp->rv, lo, hi, kt, c->s));
        }
        FOTO_TRY(comm_fork(c));
        FOTO_TRY(exchange_raw(c, alltoall_part_xfers(c->Nt, c->Ny, c->Nx, c->W, true, p, parts, 0), sbuf, rbuf));
    }
    FOTO_TRY(comm_join(c));
    for (auto& sp : c->sh) FOTO_TRY(sp->spec->fwd_t(kt, c->s));
    return 0;
}

static int sharded_gauss(foto_bb_ctx* c) {
    KTimer* kt = &c->kt;
    for (auto& sp : c->sh) FOTO_TRY(sp->spec->gauss_measure(kt, c->s));
    FOTO_TRY(allgather(c, [](Shard& s) { return s.spec->gauss_hist(); }, SpectralPlan::gauss_hist_size()));
    for (auto& sp : c->sh) FOTO_TRY(sp->spec->gauss_solve(c->o.cg_rtol, c->o.cg_maxiter, kt, c->s));
    return 0;
}

static int sharded_inv(foto_bb_ctx* c) {
    KTimer* kt = &c->kt;
    for (auto& sp : c->sh) FOTO_TRY(sp->spec->inv_t(kt, c->s));
    const int parts = a2a_parts(c), halo = a2a_halo(c);
    // inv_local takes the inverse's slab (and halo planes) from the RHS buffer (F is consumed by then)
    auto sbuf = [](Shard& s) { return s.spec->box_out(); };
    auto rbuf = [](Shard& s) { return s.rv; };
    FOTO_TRY(comm_fork(c));
    for (int p = 0; p < parts; ++p) {
        FOTO_TRY(exchange_raw(c, alltoall_part_xfers(c->Nt, c->Ny, c->Nx, c->W, false, p, parts, halo), sbuf, rbuf));
        if (c->sc) FOTO_HIP_CHECK(hipEventRecord(c->cpart[p], c->sc));
    }
    for (int p = 0; p < parts; ++p) {
        if (c->sc) FOTO_HIP_CHECK(hipStreamWaitEvent(c->s, c->cpart[p], 0));
        for (auto& sp : c->sh) {
            int lo, hi;
            alltoall_part_planes(c->Nt, c->W, sp->rank, p, parts, halo, &lo, &hi);
            if (hi > lo) FOTO_TRY(sp->spec->inv_local(sp->rv, sp->phi, lo, hi, kt, c->s));
        }
    }
    c->phi_halo = halo != 0;
    return 0;
}

static int sharded_sstep(foto_bb_ctx* c, int* iters, int* info) {
    const int maxiter = c->o.cg_maxiter;
    const double rtol = c->o.cg_rtol;
    const int M = SpectralPlan::moments();
    KTimer* kt = &c->kt;
    for (auto& sp : c->sh) FOTO_TRY(sp->spec->cg_begin(rtol, maxiter, kt, c->s));
    FOTO_TRY(allgather(c, [](Shard& s) { return s.spec->gath(); }, M));
    for (auto& sp : c->sh) FOTO_TRY(sp->spec->cg_plan(1, rtol, maxiter, c->s));
    auto pass = [&]() -> int {
        for (auto& sp : c->sh) FOTO_TRY(sp->spec->cg_pass(rtol, maxiter, kt, c->s));
        FOTO_TRY(allgather(c, [](Shard& s) { return s.spec->gath(); }, M));
        for (auto& sp : c->sh) FOTO_TRY(sp->spec->cg_plan(0, rtol, maxiter, c->s));
        return 0;
    };
    // every shard's state is the same (same gathered moments): the first local shard's plan polls
    return c->sh[0]->spec->sstep_passes(pass, (int)c->sh.size(), maxiter, iters, info, kt, c->s);
}

// the whole sharded solve, waiting for it on the host (FOTO_CG_DEFER=0, or the s-step CG)
static int cg_solve_spectral_sharded(foto_bb_ctx* c, int* iters, int* info) {
    const int maxiter = c->o.cg_maxiter;
    FOTO_TRY(sharded_fwd(c));
    if (c->sh[0]->spec->gauss()) {
        FOTO_TRY(sharded_gauss(c));
        int ok = 1;
        for (auto& sp : c->sh) {
            int k_ok = 0;
            FOTO_TRY(sp->spec->gauss_wait(maxiter, &k_ok, iters, info, c->s));
            ok = ok && k_ok;   // identical on every shard and rank (same gathered histograms)
        }
        if (ok) {
            FOTO_TRY(sharded_inv(c));
            for (auto& sp : c->sh) sp->spec->gauss_end();
            c->last_cg = *iters;
            return 0;
        }
        c->st.cg_redo += 1;   // the s-step CG from b^ (cg_begin takes its INIT moments)
    }
    FOTO_TRY(sharded_sstep(c, iters, info));
    FOTO_TRY(sharded_inv(c));
    c->last_cg = *iters;
    return 0;
}

// Solve A x = F (F already in rv, F.F gathered in gath_rr) to scipy's stopping rule.
// The loop runs on the device; the host only polls the done flag between chunks.  Every
// rank takes the same decisions (the flag is a function of gathered scalars), so the
// collective call sequence stays identical across ranks.
static int cg_solve(foto_bb_ctx* c, int* iters, int* info) {
    const int maxiter = c->o.cg_maxiter;
    if (c->o.cg_mode != 0) {
        if (c->W > 1) return cg_solve_spectral_sharded(c, iters, info);
        Shard& s = *c->sh[0];
        FOTO_TRY(s.spec->solve(s.rv, s.phi, c->o.cg_rtol, maxiter, c->last_cg, iters, info, &c->kt, c->s));
        c->last_cg = *iters;
        return 0;
    }
    for (auto& sp : c->sh) FOTO_HIP_CHECK(hipMemsetAsync(sp->S, 0, sizeof(CGScal), c->s));
    bool done = false;
    FOTO_TRY(cg_poll_chunks(c->last_cg > 4 ? c->last_cg - 3 : 6, maxiter, [&](int k) { return cg_iteration(c, k); },
                            c->sh[0]->S, c->hS, c->s, &done, iters, info));
    if (done && *iters == 0)
        for (auto& sp : c->sh)
            FOTO_HIP_CHECK(hipMemsetAsync(sp->phi, 0, sizeof(double) * sp->g.nloc * sp->g.nxy, c->s));
    c->last_cg = *iters;
    return 0;
}

// ----------------------------------------------------------------------------- outer iteration

// One outer iteration in two halves.  outer_head + outer_tail put the iteration's work on the
// stream (a non-deferred CG solve waits for itself inside) and push an Enq record;
// outer_complete waits for the oldest record's crit readback, finishes its deferred solve and
// computes crit.  outer_head (halos, RHS) only writes F.  With one iteration in flight, a single
// spectral shard gets the next iteration's head on the stream before the host waits for this
// iteration's crit (the stop rules can still end the run there: F is scratch; a CG redo re-runs
// the head).  With two in flight (c->pipe) the whole next iteration is enqueued first.  The
// host callback runs after the next iteration is enqueued.
static bool phase_on(const foto_bb_ctx* c) { return c->phase_force || c->kt.on; }

static int outer_head(foto_bb_ctx* c) {
    c->hpar ^= 1;
    if (phase_on(c)) FOTO_HIP_CHECK(hipEventRecord(c->ph[c->hpar][0], c->s));
    // the previous iteration's k_prox_rhs wrote F (and F.F).  (Enqueuing the next solve's x-DCT
    // here, ahead of the crit wait, measured no faster: 457 vs 457 it/s same box.)
    if (c->fuse && c->f_ready) return 0;
    FOTO_TRY(wt_drop(c));   // (F recomputed whole: no edge planes left to finish)
    FOTO_TRY(halo(c, [](Shard& s) { return s.mu[0]; }));
    FOTO_TRY(halo(c, [](Shard& s) { return s.q[0]; }));
    for (auto& sp : c->sh) {
        Shard& s = *sp;
        const double nv = (double)s.g.nloc * (double)s.g.nxy;
        hipEvent_t e = c->kt.start(c->s);
        FOTO_HIP_CHECK(launch_rhs(s.g, s.mu[0], s.mu[1], s.mu[2], s.q[0], s.q[1], s.q[2], s.rho0, s.rhoT, c->r,
                                  s.rv, s.rb, c->o.cg_mode == 0 ? s.gath_rr() : nullptr, s.rank, c->s));
        c->kt.stop(e, c->s, FOTO_K_RHS, 56.0 * nv);
    }
    if (c->o.cg_mode == 0) FOTO_TRY(allgather(c, [](Shard& s) { return s.gath_rr(); }, 1));
    return 0;
}

// the fused k_prox_rhs of every local shard on the pair recorded in its fz_src -> fz_dst;
// sharded: the two-plane phi halo and the one-plane halo of the mu it reads go first.
// guarded: each shard's launch returns at once unless its CG's done flag is set.
static int prox_rhs(foto_bb_ctx* c, bool guarded, int par) {
    const int W = c->W;
    double* hcrit = c->hcrit ? c->dgath[par] + 2 * W : nullptr;
    // sharded: defer the slab-edge F (default: two planes per neighbour on the wire, phi and w_t)
    // or recompute the neighbours' boundary stepB (FOTO_PR_EDGE=0: five planes, 2 phi + 3 mu)
    const bool defer = W > 1 && c->tn.pr_edge;
    FOTO_TRY(wt_drop(c));   // (a redo's prox supersedes a pending exchange)
    const bool pre = defer && wt_pre_on(c);
    if (W > 1) {
        if (defer) {
            if (!c->phi_halo) FOTO_TRY(halo(c, [](Shard& s) { return s.phi; }));
        } else {
            FOTO_TRY(exchange(c, halo_depth_xfers(c->Nt, (int64_t)c->Nx * c->Ny, W, 2), [](Shard& s) { return s.phi; },
                              [](Shard& s) { return s.phi; }));
            for (int f = 0; f < 3; ++f) FOTO_TRY(halo(c, [f](Shard& s) { return s.fz_src[f]; }));
        }
    }
    if (pre) {   // the edge planes' w_t first, then on the wire while k_prox_rhs runs
        for (auto& sp : c->sh) {
            Shard& s = *sp;
            const int dlo = s.g.t0 > 0, dhi = s.g.t0 + s.g.nloc < c->Nt;
            hipEvent_t e = c->kt.start(c->s);
            FOTO_HIP_CHECK(launch_wt_pre(s.g, s.phi, s.fz_src[0], s.fz_src[1], s.fz_src[2], c->r, s.wt, dlo, dhi, c->s,
                                         guarded ? s.spec->done_flag() : nullptr));
            c->kt.stop(e, c->s, FOTO_K_PROX, 56.0 * (double)((dlo ? 1 : 0) + (dhi ? 1 : 0)) * (double)s.g.nxy);
        }
        if (c->rccl) {
            FOTO_TRY(comm_fork(c));
            FOTO_TRY(exchange_raw(c, halo_xfers(c->Nt, (int64_t)c->Nx * c->Ny, W), [](Shard& s) { return s.wt; },
                                  [](Shard& s) { return s.wt; }));
            c->wt_pending = true;
            c->wt_guarded = guarded;
        } else {
            FOTO_TRY(halo(c, [](Shard& s) { return s.wt; }));
        }
    }
    for (auto& sp : c->sh) {
        Shard& s = *sp;
        const double nv = (double)s.g.nloc * (double)s.g.nxy;
        const int dlo = defer && s.g.t0 > 0, dhi = defer && s.g.t0 + s.g.nloc < c->Nt;
        hipEvent_t e = c->kt.start(c->s);
        FOTO_HIP_CHECK(launch_prox_rhs(s.g, s.phi, s.fz_src[0], s.fz_src[1], s.fz_src[2], s.fz_dst[0], s.fz_dst[1],
                                       s.fz_dst[2], s.rho0, s.rhoT, c->r, s.rv, s.rb, s.gath_crit(W) + 2 * s.rank,
                                       c->o.cg_mode == 0 ? s.gath_rr() + s.rank : nullptr, c->tn.pr_tch, c->s,
                                       guarded ? s.spec->done_flag() : nullptr, dlo, dhi, s.wt, s.edge, hcrit,
                                       pre ? 1 : 0));
        c->kt.stop(e, c->s, FOTO_K_PROX, 64.0 * nv);
    }
    if (defer && !c->wt_pending) {   // (RCCL with pre: the next forward finishes the edges)
        if (!pre) FOTO_TRY(halo(c, [](Shard& s) { return s.wt; }));
        FOTO_TRY(wt_edges(c, guarded));
    }
    c->phi_halo = false;   // (consumed: the next prox's phi comes from the next solve)
    // the stencil CG's F.F (its stopping rule) from every rank
    if (c->o.cg_mode == 0) FOTO_TRY(allgather(c, [](Shard& s) { return s.gath_rr(); }, 1));
    return 0;
}

// The prox of every local shard on its current phi and the crit readback into slot `par`: the
// fused prox_rhs (on the pair in fz_src -> fz_dst), or phi's halo and k_prox; the crit all-gather;
// its copy to the slot's host mirror unless the kernel stored it there; the iteration's `done`
// event.  outer_tail enqueues it behind a deferred solve (guarded); a redo runs it unguarded on
// the final phi and waits for the event.
static int prox_crit(foto_bb_ctx* c, bool guarded, int par, hipEvent_t done) {
    const int W = c->W;
    if (c->fuse) {
        FOTO_TRY(prox_rhs(c, guarded, par));
    } else {
        if (!c->phi_halo) FOTO_TRY(halo(c, [](Shard& s) { return s.phi; }));
        c->phi_halo = false;
        for (auto& sp : c->sh) {
            Shard& s = *sp;
            const double nv = (double)s.g.nloc * (double)s.g.nxy;
            hipEvent_t t = c->kt.start(c->s);
            FOTO_HIP_CHECK(launch_prox(s.g, s.phi, s.mu[0], s.mu[1], s.mu[2], s.q[0], s.q[1], s.q[2], c->r, s.rb,
                                       s.gath_crit(W), s.rank, c->s, guarded ? s.spec->done_flag() : nullptr));
            c->kt.stop(t, c->s, FOTO_K_PROX, 80.0 * nv);
        }
    }
    FOTO_TRY(allgather(c, [W](Shard& s) { return s.gath_crit(W); }, 2));
    if (!c->hcrit)
        FOTO_HIP_CHECK(hipMemcpyAsync(c->hgath[par], c->sh[0]->gath, sizeof(double) * 4 * W, hipMemcpyDeviceToHost,
                                      c->s));
    FOTO_HIP_CHECK(hipEventRecord(done, c->s));
    return 0;
}

// kmark: the KTimer mark taken before this iteration's head
static int outer_tail(foto_bb_ctx* c, size_t kmark) {
    const int W = c->W;
    Shard& s0 = *c->sh[0];
    foto_bb_ctx::Enq e;
    e.par = c->hpar;
    e.kmark = kmark;
    e.before = s0.rot();
    e.f_ready = c->f_ready;
    e.hpar = c->hpar ^ 1;   // (before this iteration's head)
    hipEvent_t* ph = c->ph[e.par];
    e.pev = phase_on(c);
    // phase boundaries are recorded, not waited on: the one host wait per outer iteration
    // is the crit readback below (a wait here idled the GPU for the host's wake-up)
    if (e.pev) FOTO_HIP_CHECK(hipEventRecord(ph[1], c->s));
    // Single shard, spectral: the solve is enqueued without a host wait and prox follows behind
    // it, guarded by the CG's done flag; the one sync (crit) then also delivers the CG result.
    // A solve that needs more work (s-step: more passes than predicted; Gauss: K beyond the
    // table) is finished after that sync, and prox re-runs (FOTO_CG_DEFER=0: always wait).
    const bool defer_on = c->tn.cg_defer;
    SpectralPlan* dsp = (defer_on && W == 1 && c->o.cg_mode != 0 && s0.spec && s0.spec->deferrable())
                            ? s0.spec.get()
                            : nullptr;
    if (c->pipe && !dsp) {
        set_error("outer iteration: the pipelined loop needs a deferrable Gauss solve");
        return FOTO_ERR_STATE;
    }
    // Sharded Gauss CG: likewise enqueued whole -- x^ from the table, the all-to-all back, the
    // inverse DCTs and prox (guarded by each shard's done flag) -- and checked at the crit sync;
    // a failed solve (every rank sees the same status: the same gathered histograms) is redone
    // there with the s-step CG from b^ by every rank, so the collective sequence stays identical
    const bool sdefer = defer_on && W > 1 && s0.spec && s0.spec->gauss();
    if (c->pipe) std::swap(s0.phi, s0.phi_alt);   // this iteration's phi; the last one's stays intact
    if (dsp) {
        FOTO_TRY(dsp->solve_deferred(s0.rv, s0.phi, c->o.cg_rtol, c->o.cg_maxiter, &c->kt, c->s));
    } else if (sdefer) {
        FOTO_TRY(sharded_fwd(c));
        FOTO_TRY(sharded_gauss(c));
        FOTO_TRY(sharded_inv(c));
    } else {
        FOTO_TRY(cg_solve(c, &e.its, &e.info));
    }
    const bool guarded = dsp != nullptr || sdefer;
    if (e.pev) FOTO_HIP_CHECK(hipEventRecord(ph[2], c->s));
    c->have_phi = 1;

    // fused: prox + the next iteration's RHS: mu -> nu, F -> rv; then nu is the current mu
    // (pipelined: mu -> nu -> xi -> mu rotate, so the mu before this iteration survives it)
    if (c->fuse)
        for (auto& sp : c->sh)
            for (int f = 0; f < 3; ++f) { sp->fz_src[f] = sp->mu[f]; sp->fz_dst[f] = sp->nu[f]; }
    FOTO_TRY(prox_crit(c, guarded, e.par, e.pev ? ph[3] : c->fin[e.par]));
    if (c->fuse) {
        for (auto& sp : c->sh)
            for (int f = 0; f < 3; ++f) {
                if (c->pipe) {
                    double* m = sp->mu[f];
                    sp->mu[f] = sp->nu[f];
                    sp->nu[f] = sp->xi[f];
                    sp->xi[f] = m;
                } else {
                    std::swap(sp->mu[f], sp->nu[f]);
                }
            }
        c->f_ready = true;
    }
    e.dsp = dsp;
    e.sdefer = sdefer;
    c->inflight.push_back(e);
    return 0;
}

// Drop the newest enqueued outer iteration (pipelined loop only): wait for the stream, forget
// its solve and its timings, and put the host state back as it was before it.  F of the last
// kept iteration was overwritten by the dropped one's prox, so the next head recomputes it from
// q, itself recomputed from that iteration's phi and the mu before it (both intact).
static int rollback(foto_bb_ctx* c) {
    if (c->inflight.empty()) return 0;
    const foto_bb_ctx::Enq e = c->inflight.back();
    c->inflight.pop_back();
    FOTO_HIP_CHECK(hipStreamSynchronize(c->s));
    FOTO_TRY(wt_drop(c));   // (the dropped prox's w_t: the next head recomputes F whole)
    Shard& s0 = *c->sh[0];
    if (e.dsp) FOTO_TRY(e.dsp->drop_newest(c->s));
    c->kt.discard_from(e.kmark);
    s0.rot() = e.before;
    c->hpar = e.hpar;
    if (e.f_ready && s0.fz_src[0]) {
        // q of the kept iteration (stepB of its phi and the mu before it), for the next head's RHS
        FOTO_HIP_CHECK(launch_q_from_phi(s0.g, s0.phi, s0.fz_src[0], s0.fz_src[1], s0.fz_src[2], s0.q[0], s0.q[1],
                                         s0.q[2], c->r, c->s));
    }
    c->f_ready = false;   // (a dropped first iteration leaves mu, q as they were: the head recomputes F)
    return 0;
}

// After an error with outer iterations on the stream: wait for the stream (errors ignored: the
// one being reported is the first), forget their deferred solves and timings, and leave no
// record behind, so foto_bb_reset can start over.
static void drain_inflight(foto_bb_ctx* c) {
    if (c->sc && c->wt_pending) {   // (a pending w_t exchange: let it land, nothing consumes it)
        (void)hipStreamSynchronize(c->sc);
        c->wt_pending = false;
    }
    if (c->inflight.empty()) return;
    (void)hipStreamSynchronize(c->s);
    for (auto it = c->inflight.rbegin(); it != c->inflight.rend(); ++it)
        if (it->dsp) (void)it->dsp->drop_newest(c->s);
    c->kt.discard_from(c->inflight.front().kmark);
    c->inflight.clear();
    c->broken = true;
}

// The host pointers of the last COMPLETED outer iteration.  Inside the iteration callback the
// next iteration is already on the stream and the shard's pointers are its own; the pipelined
// loop keeps the completed iteration's phi and mu intact (the record of the one in flight holds
// them), the one-in-flight loop does not (its next solve overwrites phi), so there a call from
// the callback is refused.  Only shard 0 has such a record (the pipelined loop is single-shard):
// of() gives every reader the pointers to use for a shard.
struct Completed {
    const Shard* s0 = nullptr;
    const Rot* k0 = nullptr;   // shard 0's own pointers, or the record of the iteration in flight
    const Rot& of(const Shard& s) const { return &s == s0 ? *k0 : s; }
};
static int completed_state(foto_bb_ctx* c, const char* who, Completed* out) {
    out->s0 = c->sh[0].get();
    out->k0 = out->s0;
    if (c->inflight.empty()) return 0;
    if (!c->pipe) {
        set_error("%s: called while the next outer iteration is on the stream (from the iteration callback of "
                  "the one-in-flight loop, whose next solve overwrites phi); call it after foto_bb_iterate returns",
                  who);
        return FOTO_ERR_STATE;
    }
    out->k0 = &c->inflight.front().before;   // (stays put: an export enqueues and drops no iteration)
    return 0;
}

static int outer_complete(foto_bb_ctx* c, double* crit, int* cg_iters, int* cg_info) {
    const int W = c->W;
    if (c->inflight.empty()) {
        set_error("outer iteration: nothing in flight");
        return FOTO_ERR_STATE;
    }
    const foto_bb_ctx::Enq e = c->inflight.front();
    c->inflight.erase(c->inflight.begin());
    SpectralPlan* dsp = e.dsp;
    *cg_iters = e.its;
    *cg_info = e.info;
    hipEvent_t* ph = c->ph[e.par];
    const hipEvent_t done = e.pev ? ph[3] : c->fin[e.par];   // the crit readback
    FOTO_HIP_CHECK(hipEventSynchronize(done));
    if (dsp) {
        // a failed solve is redone once the iteration behind it (whose prox its done-flag chain
        // skipped) is dropped; the loop enqueues that iteration again
        if (!c->inflight.empty() && dsp->oldest_needs_redo()) FOTO_TRY(rollback(c));
        int redo = 0;
        FOTO_TRY(dsp->finish(cg_iters, cg_info, &redo, &c->kt, c->s));
        c->last_cg = *cg_iters;
        if (redo) {   // the guarded prox returned at once: drop its timing, run it on the final phi
            c->kt.discard_last(FOTO_K_PROX, 1);
            FOTO_TRY(prox_crit(c, false, e.par, done));
            if (c->fuse) c->f_ready = true;   // (a rollback before the redo had cleared it)
            FOTO_HIP_CHECK(hipEventSynchronize(done));
            c->st.cg_redo += 1;
        }
    }
    if (e.sdefer) {
        int ok = 1;
        for (auto& sp : c->sh) {
            int k_ok = 0;
            FOTO_TRY(sp->spec->gauss_result(c->o.cg_maxiter, &k_ok, cg_iters, cg_info, c->s));
            ok = ok && k_ok;   // identical on every shard and rank
        }
        if (!ok) {
            // every rank: the s-step CG from b^ (still intact: x^ went to the box scratch), the
            // inverse again, then the prox that the done flags held back, and a new crit readback
            c->kt.discard_last(FOTO_K_PROX, (int)c->sh.size());
            FOTO_TRY(sharded_sstep(c, cg_iters, cg_info));
            FOTO_TRY(sharded_inv(c));
            FOTO_TRY(prox_crit(c, false, e.par, done));
            FOTO_HIP_CHECK(hipEventSynchronize(done));
            c->st.cg_redo += 1;
        }
        c->last_cg = *cg_iters;
    }
    float t_rhs = 0.f, t_cg = 0.f, t_prox = 0.f;
    if (e.pev) {
        FOTO_HIP_CHECK(hipEventElapsedTime(&t_rhs, ph[0], ph[1]));
        FOTO_HIP_CHECK(hipEventElapsedTime(&t_cg, ph[1], ph[2]));
        FOTO_HIP_CHECK(hipEventElapsedTime(&t_prox, ph[2], ph[3]));
    }
    c->st.ms_rhs += t_rhs;
    c->st.ms_cg += t_cg;
    c->st.ms_prox += t_prox;

    const double* hg = c->hgath[e.par];
    double num = 0.0, den = 0.0;
    for (int g = 0; g < W; ++g) { num += hg[2 * W + 2 * g]; den += hg[2 * W + 2 * g + 1]; }
    *crit = std::sqrt(num / (den + 1e-10));
    c->st.outer_iters += 1;
    c->st.cg_iters_total += *cg_iters;
    c->st.last_crit = *crit;
    return 0;
}

// foto_bb_flow_dev's target: (u, v, m) leave through one export kernel instead of three downloads
struct FlowDev {
    void* out;
    int dtype, layout;
    hipStream_t user;
};

// a shard's flow record (fu, fv, fm: one plane of float64 each) into three host arrays
static int download_flow(foto_bb_ctx* c, const Shard& s, double* u, double* v, double* m) {
    const size_t bytes = (size_t)c->Nx * c->Ny * sizeof(double);
    FOTO_HIP_CHECK(hipMemcpyAsync(u, s.fu, bytes, hipMemcpyDeviceToHost, c->s));
    FOTO_HIP_CHECK(hipMemcpyAsync(v, s.fv, bytes, hipMemcpyDeviceToHost, c->s));
    FOTO_HIP_CHECK(hipMemcpyAsync(m, s.fm, bytes, hipMemcpyDeviceToHost, c->s));
    return 0;
}

// (shard 0 reads the completed iteration's phi, k.of(): an export writes no solver state)
static int flow(foto_bb_ctx* c, const Completed& k, double* u, double* v, double* m, const FlowDev* dv = nullptr) {
    if (!c->have_phi) {
        set_error("foto_bb_flow: no outer iteration has run yet (reference: UnboundLocalError for max_it=0)");
        return FOTO_ERR_STATE;
    }
    const int W = c->W;
    FOTO_HIP_CHECK(hipEventRecord(c->fl[0], c->s));
    // Trajectories relay rank to rank: rank j runs the steps of its planes, then its
    // positions travel to rank j + 1; the last rank finishes (u, v, m) and delivers them to
    // rank 0.  The same transfer lists for both transports (exchange()).
    const int64_t nxy = (int64_t)c->Nx * c->Ny;
    auto local = [&](int rank) -> Shard* {
        for (auto& sp : c->sh)
            if (sp->rank == rank) return sp.get();
        return nullptr;
    };
    for (int j = 0; j < W; ++j) {
        if (Shard* s = local(j)) {
            const int n_lo = s->g.t0, n_hi = std::min(s->g.t0 + s->g.nloc, c->Nt - 1);
            FOTO_HIP_CHECK(launch_traj(s->g, k.of(*s).phi, n_lo, std::max(n_lo, n_hi), s->px, s->py, j == 0, c->s));
            if (j == W - 1)
                FOTO_HIP_CHECK(launch_flow_record(c->Nx, c->Ny, s->px, s->py, s->fu, s->fv, s->fm, FOTO_F64, 0, c->s));
        }
        if (j + 1 < W) {
            const std::vector<Xfer> xs = relay_xfers(nxy, j);
            FOTO_TRY(exchange(c, xs, [](Shard& s) { return s.px; }, [](Shard& s) { return s.px; }));
            FOTO_TRY(exchange(c, xs, [](Shard& s) { return s.py; }, [](Shard& s) { return s.py; }));
        }
    }
    if (W > 1) {
        const std::vector<Xfer> xs = deliver_xfers(nxy, W);
        FOTO_TRY(exchange(c, xs, [](Shard& s) { return s.fu; }, [](Shard& s) { return s.fu; }));
        FOTO_TRY(exchange(c, xs, [](Shard& s) { return s.fv; }, [](Shard& s) { return s.fv; }));
        FOTO_TRY(exchange(c, xs, [](Shard& s) { return s.fm; }, [](Shard& s) { return s.fm; }));
    }
    if (Shard* s0 = local(0)) {
        if (u && v && m) FOTO_TRY(download_flow(c, *s0, u, v, m));
        if (dv) {   // (the caller's earlier work on `out` first; the trajectories above did not touch it)
            FOTO_TRY(c->link.enter(dv->user, c->s));
            FOTO_HIP_CHECK(launch_export(nxy, s0->fu, s0->fv, s0->fm, dv->out, dv->dtype, dv->layout, c->s));
        }
    }
    FOTO_HIP_CHECK(hipEventRecord(c->fl[1], c->s));
    FOTO_HIP_CHECK(hipEventSynchronize(c->fl[1]));
    float t = 0.f;
    FOTO_HIP_CHECK(hipEventElapsedTime(&t, c->fl[0], c->fl[1]));
    c->st.ms_flow += t;
    return 0;
}

// ------------------------------------------------------------------ transport path exports
// The in-process shard that owns global plane n (one device: world == 1, virtual ranks included).
static Shard* plane_owner(foto_bb_ctx* c, int n) {
    for (auto& sp : c->sh)
        if (n >= sp->g.t0 && n < sp->g.t0 + sp->g.nloc) return sp.get();
    return nullptr;
}

// foto_bb_flow_path / _dev: launch_traj one step at a time from the running positions (shard
// 0's px, py; step n reads phi plane n of whichever shard owns it), and after each step the
// record (u_n, v_n, m_n) straight from them -- two launches per step.  Host: the record goes to
// shard 0's fu, fv, fm and from there into the caller's arrays.  Touches neither the statistics
// nor anything the outer loop reads.
static int flow_path(foto_bb_ctx* c, const Completed& k, double* hu, double* hv, double* hm, const FlowDev* dv) {
    Shard& s0 = *c->sh[0];
    const int64_t nxy = (int64_t)c->Nx * c->Ny;
    if (dv) FOTO_TRY(c->link.enter(dv->user, c->s));   // (before the first write of `out`)
    for (int n = 0; n + 1 < c->Nt; ++n) {
        Shard* sp = plane_owner(c, n);
        if (!sp) { set_error("flow path: no local shard owns plane %d", n); return FOTO_ERR_STATE; }
        FOTO_HIP_CHECK(launch_traj(sp->g, k.of(*sp).phi, n, n + 1, s0.px, s0.py, n == 0, c->s));
        if (dv) {
            const size_t rec = (size_t)nxy * (dv->layout == 0 ? 3 : 2) * dtype_bytes(dv->dtype);
            char* o = (char*)dv->out + (size_t)n * rec;
            const size_t pl = (size_t)nxy * dtype_bytes(dv->dtype);
            FOTO_HIP_CHECK(launch_flow_record(c->Nx, c->Ny, s0.px, s0.py, o, o + pl, o + 2 * pl, dv->dtype,
                                              dv->layout, c->s));
        } else {
            FOTO_HIP_CHECK(launch_flow_record(c->Nx, c->Ny, s0.px, s0.py, s0.fu, s0.fv, s0.fm, FOTO_F64, 0, c->s));
            FOTO_TRY(download_flow(c, s0, hu + n * nxy, hv + n * nxy, hm + n * nxy));
        }
    }
    if (dv) return c->link.leave(c->s, dv->user);
    FOTO_HIP_CHECK(hipStreamSynchronize(c->s));
    return 0;
}

// The state rules of the one-device exports, before any argument is looked at ...
static int export_state_check(foto_bb_ctx* c, const char* who) {
    if (!c) { set_error("%s: null ctx", who); return FOTO_ERR_ARG; }
    if (c->rccl) { set_error("%s: not supported on RCCL-sharded contexts", who); return FOTO_ERR_STATE; }
    if (c->broken) {
        set_error("%s: a failed foto_bb_iterate left the context inconsistent; foto_bb_reset it", who);
        return FOTO_ERR_STATE;
    }
    return 0;
}

// ... and of those that read phi (the device flow, the flow path, point tracking; the frames read
// mu, which a context has from the start)
static int path_state_check(foto_bb_ctx* c, const char* who) {
    FOTO_TRY(export_state_check(c, who));
    if (!c->have_phi) {   // (before the output is looked at: the reference's UnboundLocalError)
        set_error("%s: no outer iteration has run yet", who);
        return FOTO_ERR_STATE;
    }
    return 0;
}

// The argument rules of foto_bb_frames / _dev (before anything is enqueued or written).
static int frames_check(foto_bb_ctx* c, const double* s, int count, double scale, const void* out, int dtype,
                        const char* who) {
    FOTO_TRY(export_state_check(c, who));
    if (!s || !out) { set_error("%s: null pointer", who); return FOTO_ERR_ARG; }
    if (count <= 0) { set_error("%s: count = %d must be > 0", who, count); return FOTO_ERR_ARG; }
    if (!std::isfinite(scale) || !(scale > 0.0)) {
        set_error("%s: scale %g must be finite and > 0", who, scale);
        return FOTO_ERR_ARG;
    }
    if (dtype < FOTO_U8 || dtype > FOTO_F64) {
        set_error("%s: dtype %d is not FOTO_U8 / FOTO_F32 / FOTO_F64", who, dtype);
        return FOTO_ERR_ARG;
    }
    for (int k = 0; k < count; ++k) {
        if (!std::isfinite(s[k]) || s[k] < 0.0 || s[k] > (double)(c->Nt - 1)) {
            set_error("%s: s[%d] = %.17g is outside [0, Nt - 1 = %d]", who, k, s[k], c->Nt - 1);
            return FOTO_ERR_ARG;
        }
    }
    return 0;
}

// Frames [k0, k0 + cnt) of s into `out` (device memory of `dtype`), one launch: the density
// planes are mu's t-part of the completed iteration, in whichever shard owns them.
static int frames_launch(foto_bb_ctx* c, const Completed& k, const double* s, int cnt, double scale, void* out,
                         int dtype) {
    const int64_t nxy = (int64_t)c->Nx * c->Ny;
    FrameArgs fa;
    for (int i = 0; i < cnt; ++i) {
        const int n = std::min((int)s[i], c->Nt - 2);
        const double w = s[i] - (double)n;
        Shard* pa = plane_owner(c, n);
        Shard* pb = plane_owner(c, n + 1);
        if (!pa || !pb) { set_error("frames: no local shard owns plane %d / %d", n, n + 1); return FOTO_ERR_STATE; }
        fa.a[i] = k.of(*pa).mu[0] + (int64_t)(n - pa->g.t0) * nxy;
        fa.b[i] = k.of(*pb).mu[0] + (int64_t)(n + 1 - pb->g.t0) * nxy;
        fa.w[i] = w;
    }
    FOTO_HIP_CHECK(launch_frames(fa, cnt, nxy, scale, out, dtype, c->s));
    return 0;
}

// ------------------------------------------------------------------ transport report
// foto_bb_report / _dev: k_report once per in-process shard on the completed iteration's mu and phi
// (k.of()), the t-neighbour planes of a shard's edges taken from the shards that own them.  The
// table goes to `out` (device memory), or to the scratch's staging table when out is null
// (*staged).  Touches neither the statistics nor anything the outer loop reads.
static int report_run(foto_bb_ctx* c, const Completed& k, double* out, double** staged) {
    const int64_t nxy = (int64_t)c->Nx * c->Ny;
    const size_t ntab = (size_t)c->Nt * FOTO_REPORT_COLS, npart = ntab * (size_t)report_pieces(nxy);
    const size_t bytes = (ntab + npart) * sizeof(double) + (size_t)c->Nt * sizeof(unsigned);
    if (c->rep.cap < bytes) {
        FOTO_TRY(c->rep.reserve(bytes, c->s));
        FOTO_HIP_CHECK(hipMemsetAsync((double*)c->rep.p + ntab + npart, 0, (size_t)c->Nt * sizeof(unsigned), c->s));
    }
    double* const table = (double*)c->rep.p;
    double* const part = table + ntab;
    unsigned* const ticket = (unsigned*)(part + npart);
    if (!out) out = table;
    if (staged) *staged = table;
    for (auto& sp : c->sh) {
        const Shard& s = *sp;
        const Rot& ks = k.of(s);
        ReportIn in{};
        in.rho = ks.mu[0]; in.m1 = ks.mu[1]; in.m2 = ks.mu[2]; in.phi = ks.phi;
        in.rho0 = s.rho0; in.rhoT = s.rhoT;
        if (s.g.t0 > 0) {
            const Shard* lo = plane_owner(c, s.g.t0 - 1);
            if (!lo) { set_error("report: no local shard owns plane %d", s.g.t0 - 1); return FOTO_ERR_STATE; }
            const int64_t o = (int64_t)(s.g.t0 - 1 - lo->g.t0) * nxy;
            in.rho_lo = k.of(*lo).mu[0] + o;
            in.phi_lo = k.of(*lo).phi + o;
        }
        if (s.g.t0 + s.g.nloc < c->Nt) {
            const Shard* hi = plane_owner(c, s.g.t0 + s.g.nloc);
            if (!hi) { set_error("report: no local shard owns plane %d", s.g.t0 + s.g.nloc); return FOTO_ERR_STATE; }
            in.rho_hi = k.of(*hi).mu[0];
            in.phi_hi = k.of(*hi).phi;
        }
        FOTO_HIP_CHECK(launch_report(s.g, in, part, ticket, out, c->s));
    }
    return 0;
}

}  // namespace foto

// ============================================================================ C ABI (BB)

extern "C" {

int foto_version(void) { return 1; }

int foto_device_count(int* n) {
    FOTO_HIP_CHECK(hipGetDeviceCount(n));
    return 0;
}

int foto_bb_opts_default(foto_bb_opts* o) {
    if (!o) return FOTO_ERR_ARG;
    memset(o, 0, sizeof(*o));
    o->device = -1;
    o->cg_maxiter = 1000;
    o->cg_rtol = 1e-6;
    o->cg_mode = -1;  // auto (foto_bb_create): the stencil CG on small grids, the Gauss-compressed spectral CG above
    o->rank = 0;
    o->world = 1;
    o->nccl_id = nullptr;
    o->virtual_ranks = 1;
    o->timing = 0;
    return 0;
}

int foto_xfer_calls(int kind, int Nt, int Ny, int Nx, int world, int rank, int arg, int64_t* out, int cap,
                    int* count) {
    if (!out || !count || world < 1 || rank < 0 || rank >= world || Nt < world || Ny < world || Nx < 1) {
        set_error("foto_xfer_calls: bad arguments");
        return FOTO_ERR_ARG;
    }
    const int64_t nxy = (int64_t)Nx * Ny;
    std::vector<Xfer> xs;
    switch (kind) {
        case FOTO_XFER_HALO: xs = halo_xfers(Nt, nxy, world); break;
        case FOTO_XFER_SLAB_TO_BOX: xs = alltoall_xfers(Nt, Ny, Nx, world, true); break;
        case FOTO_XFER_BOX_TO_SLAB: xs = alltoall_xfers(Nt, Ny, Nx, world, false); break;
        case FOTO_XFER_RELAY:
            if (arg < 0 || arg + 1 >= world) { set_error("foto_xfer_calls: relay step out of range"); return FOTO_ERR_ARG; }
            xs = relay_xfers(nxy, arg);
            break;
        case FOTO_XFER_DELIVER: xs = deliver_xfers(nxy, world); break;
        case FOTO_XFER_HALO2: xs = halo_depth_xfers(Nt, nxy, world, 2); break;
        case FOTO_XFER_SLAB_TO_BOX_PART:
        case FOTO_XFER_BOX_TO_SLAB_PART: {
            const int part = arg & 0xff, parts = (arg >> 8) & 0xff, halo = (arg >> 16) & 0xff;
            if (parts < 1 || part >= parts || halo > 1) { set_error("foto_xfer_calls: bad part / parts / halo"); return FOTO_ERR_ARG; }
            xs = alltoall_part_xfers(Nt, Ny, Nx, world, kind == FOTO_XFER_SLAB_TO_BOX_PART, part, parts, halo);
            break;
        }
        default: set_error("foto_xfer_calls: unknown kind %d", kind); return FOTO_ERR_ARG;
    }
    const std::vector<Call> cs = rccl_calls(xs, rank);
    *count = (int)cs.size();
    if ((int)cs.size() > cap) { set_error("foto_xfer_calls: %d calls, capacity %d", (int)cs.size(), cap); return FOTO_ERR_ARG; }
    for (size_t i = 0; i < cs.size(); ++i) {
        int64_t* o = out + 5 * i;
        o[0] = cs[i].op; o[1] = cs[i].peer; o[2] = cs[i].off; o[3] = cs[i].n; o[4] = cs[i].doff;
    }
    return 0;
}

int foto_nccl_unique_id(void* out128) {
    ncclUniqueId id;
    FOTO_NCCL_CHECK(ncclGetUniqueId(&id));
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    memcpy(out128, &id, sizeof(id));
    return 0;
}

// foto_bb_create and foto_bb_create_dev: the same context from either source of the densities
static int bb_create(const RhoSrc& src, int Nt, int Nx, int Ny, double r, double reg_epsilon, const foto_bb_opts* opts,
                     foto_bb_ctx** out) {
    FOTO_TRY(grid_size_check(Nt, Nx, Ny, src.i0 ? "foto_bb_create_dev" : "foto_bb_create"));
    foto_bb_opts o;
    if (opts) o = *opts; else foto_bb_opts_default(&o);
    if (src.i0) {
        if (o.world > 1) {
            set_error("foto_bb_create_dev: device buffers are not supported on RCCL-sharded contexts (world = %d)", o.world);
            return FOTO_ERR_STATE;
        }
        // the images must be device memory of the context's device -- before anything is enqueued
        int dev = o.device;
        if (dev < 0) FOTO_HIP_CHECK(hipGetDevice(&dev));
        FOTO_TRY(image_dev_check(src.i0, Nx, Ny, dev, "foto_bb_create_dev (f0)"));
        FOTO_TRY(image_dev_check(src.iT, Nx, Ny, dev, "foto_bb_create_dev (f1)"));
    }
    if (o.world < 1 || o.rank < 0 || o.rank >= o.world) { set_error("bad rank/world"); return FOTO_ERR_ARG; }
    if (o.world > 1 && o.virtual_ranks > 1) { set_error("virtual_ranks requires world == 1"); return FOTO_ERR_ARG; }
    if (o.world > 1 && !o.nccl_id) { set_error("world > 1 needs nccl_id"); return FOTO_ERR_ARG; }
    if (o.cg_maxiter < 0) { set_error("cg_maxiter < 0"); return FOTO_ERR_ARG; }
    if (o.cg_mode > 3) { set_error("cg_mode %d: 0..3, or < 0 for auto", o.cg_mode); return FOTO_ERR_ARG; }
    // auto (cg_mode < 0, the default): the literal 7-point stencil CG on grids of at most
    // FOTO_CG_AUTO_MAX voxels (2^18: the reference's config 1 and its golden grids, where it
    // costs milliseconds and rounds like scipy's matvec -- crit within 1e-8 of the reference, where
    // the DCT-basis CGs sit at the reference's own last-bit sensitivity, 2.6e-6 on config 1), the
    // Gauss-compressed spectral CG above (the metric grid, configs 2-5)
    const Tuning tn = tuning_from_env();   // read here, once: part of the context's identity
    if (o.cg_mode < 0) o.cg_mode = ((long long)Nt * Nx * Ny <= tn.cg_auto_max) ? 0 : 3;
    // the spectral CGs recover x = C^T((b^ - r^) / lam) and need lam > 0, i.e. eps > 0; with
    // eps <= 0 (A singular, as the reference then runs it) only the stencil CG applies
    if (o.cg_mode != 0 && !(reg_epsilon > 0.0)) o.cg_mode = 0;
    auto c = std::make_unique<foto_bb_ctx>();
    c->Nt = Nt; c->Nx = Nx; c->Ny = Ny; c->r = r; c->eps = reg_epsilon; c->o = o; c->tn = tn;
    c->rccl = o.world > 1;
    c->W = c->rccl ? o.world : std::max(1, o.virtual_ranks);
    c->kt.on = o.timing != 0;
    int rc = ctx_init(c.get(), src);
    if (rc < 0) return rc;
    *out = c.release();
    return 0;
}

int foto_bb_create(const double* rho0, const double* rhoT, int Nt, int Nx, int Ny, double r, double reg_epsilon,
                   const foto_bb_opts* opts, foto_bb_ctx** out) {
    if (!rho0 || !rhoT || !out) { set_error("null argument"); return FOTO_ERR_ARG; }
    RhoSrc src;
    src.h0 = rho0;
    src.hT = rhoT;
    return bb_create(src, Nt, Nx, Ny, r, reg_epsilon, opts, out);
}

int foto_bb_create_dev(const foto_image* f0, const foto_image* f1, int normalize, void* stream, int Nt, int Nx, int Ny,
                       double r, double reg_epsilon, const foto_bb_opts* opts, double* sums2_or_null,
                       foto_bb_ctx** out) {
    if (!f0 || !f1 || !out) { set_error("foto_bb_create_dev: null argument"); return FOTO_ERR_ARG; }
    const RhoSrc src = dev_src(f0, f1, normalize, stream);
    foto_bb_ctx* c = nullptr;
    FOTO_TRY(bb_create(src, Nt, Nx, Ny, r, reg_epsilon, opts, &c));
    std::unique_ptr<foto_bb_ctx> guard(c);
    FOTO_TRY(dev_src_done(c, src, sums2_or_null));
    *out = guard.release();
    return 0;
}

static int iterate_loop(foto_bb_ctx* c, int max_iters, double tol, int use_stop_rules, foto_bb_iter_cb cb,
                        void* user, int* iters_done);

int foto_bb_iterate(foto_bb_ctx* c, int max_iters, double tol, int use_stop_rules, foto_bb_iter_cb cb, void* user,
                    int* iters_done) {
    if (!c) { set_error("null ctx"); return FOTO_ERR_ARG; }
    if (iters_done) *iters_done = 0;
    if (c->broken) {
        set_error("foto_bb_iterate: a previous call failed with outer iterations in flight; foto_bb_reset the context");
        return FOTO_ERR_STATE;
    }
    if (c->in_iterate) { set_error("foto_bb_iterate: called from its own iteration callback"); return FOTO_ERR_STATE; }
    if (!c->inflight.empty()) { set_error("foto_bb_iterate: an outer iteration is still in flight"); return FOTO_ERR_STATE; }
    c->in_iterate = true;
    const int rc = iterate_loop(c, max_iters, tol, use_stop_rules, cb, user, iters_done);
    c->in_iterate = false;
    if (rc < 0) drain_inflight(c);   // (an error leaves no record behind; only a reset continues)
    return rc;
}

}  // extern "C"

static int iterate_loop(foto_bb_ctx* c, int max_iters, double tol, int use_stop_rules, foto_bb_iter_cb cb,
                        void* user, int* iters_done) {
    int done = 0;
    int stopped = 0;
    auto stop_test = [&](double crit) {
        const double prev = c->prev_crit;
        c->prev_crit = crit;
        if (!use_stop_rules) return 0;
        if (crit <= tol) return 1;
        return (prev >= 0 && std::fabs(prev - crit) < 1e-5) ? 1 : 0;
    };
    if (c->pipe) {
        // two outer iterations in flight: iteration i + 1 is on the stream before the host
        // waits for iteration i (dropped again if the stop rules end the run at i)
        int enq = 0;
        for (int i = 0; i < max_iters; ++i) {
            while ((int)c->inflight.size() < 2 && enq < max_iters) {
                const size_t km = c->kt.mark();
                FOTO_TRY(outer_head(c));
                FOTO_TRY(outer_tail(c, km));
                ++enq;
            }
            double crit;
            int its, info;
            const size_t n_before = c->inflight.size();
            FOTO_TRY(outer_complete(c, &crit, &its, &info));
            if (c->inflight.size() + 1 < n_before) --enq;   // a redo dropped the iteration behind
            ++done;
            stopped = stop_test(crit);
            if (stopped && !c->inflight.empty()) {
                FOTO_TRY(rollback(c));
                --enq;
            }
            c->kt.resolve_upto(c->inflight.empty() ? c->kt.mark() : c->inflight.front().kmark);
            if (cb) cb(user, c->st.outer_iters - 1, crit, its, info);
            if (stopped) break;
        }
        if (iters_done) *iters_done = done;
        return stopped;
    }
    // one outer iteration in flight; the next RHS goes on the stream early for a single
    // spectral shard (see outer_head)
    const bool early = c->W == 1 && c->o.cg_mode != 0;
    if (max_iters > 0) {
        const size_t km = c->kt.mark();
        FOTO_TRY(outer_head(c));
        FOTO_TRY(outer_tail(c, km));
    }
    for (int i = 0; i < max_iters; ++i) {
        double crit;
        int its, info;
        const size_t mark = c->kt.mark();
        const bool head_early = early && i + 1 < max_iters;
        if (head_early) FOTO_TRY(outer_head(c));
        const int redo0 = c->st.cg_redo;
        FOTO_TRY(outer_complete(c, &crit, &its, &info));
        // (a redo waited for the stream after its re-run: its timing records are complete as well,
        // and count now, as in the pipelined loop, not in the next call)
        const size_t complete = c->st.cg_redo != redo0 ? c->kt.mark() : mark;
        ++done;
        stopped = stop_test(crit);
        // the next iteration goes on the stream before the host's bookkeeping for this one
        if (!stopped && i + 1 < max_iters) {
            // a redo re-ran this iteration's prox after the early head read mu, q: head again
            if (!head_early || c->st.cg_redo != redo0) FOTO_TRY(outer_head(c));
            FOTO_TRY(outer_tail(c, mark));
        }
        c->kt.resolve_upto(complete);
        if (cb) cb(user, c->st.outer_iters - 1, crit, its, info);
        if (stopped) break;
    }
    if (iters_done) *iters_done = done;
    return stopped;
}

extern "C" {

// foto_bb_reset and foto_bb_reset_dev: the same reset from either source of the densities
static int bb_reset(foto_bb_ctx* c, const RhoSrc& src) {
    if (c->in_iterate) {   // (from the iteration callback: the loop still owns the in-flight state)
        set_error("foto_bb_reset: called from foto_bb_iterate's callback");
        return FOTO_ERR_STATE;
    }
    drain_inflight(c);   // (outside foto_bb_iterate nothing is in flight: a no-op unless a call failed)
    c->broken = false;
    FOTO_HIP_CHECK(hipStreamSynchronize(c->s));
    for (auto& sp : c->sh) {
        Shard& s = *sp;
        FOTO_TRY(s.rezero(c->s));   // as ctx_init leaves them: zero, halo planes included
        FOTO_TRY(init_fields(c, s, src));
        if (s.spec) FOTO_TRY(s.spec->reset(c->s));
    }
    // the host side of the loop state, as a new context has it
    c->last_cg = 0;
    c->have_phi = 0;
    c->f_ready = false;
    for (auto& sp : c->sh)
        for (int f = 0; f < 3; ++f) sp->fz_src[f] = sp->fz_dst[f] = nullptr;
    c->prev_crit = -1;
    c->st = foto_bb_stats{};
    c->kt.resolve();
    c->kt.reset();
    c->hpar = 0;
    FOTO_HIP_CHECK(hipStreamSynchronize(c->s));
    return 0;
}

int foto_bb_reset(foto_bb_ctx* c, const double* rho0, const double* rhoT) {
    if (!c || !rho0 || !rhoT) { set_error("null argument"); return FOTO_ERR_ARG; }
    RhoSrc src;
    src.h0 = rho0;
    src.hT = rhoT;
    return bb_reset(c, src);
}

int foto_bb_reset_dev(foto_bb_ctx* c, const foto_image* f0, const foto_image* f1, int normalize, void* stream,
                      double* sums2_or_null) {
    if (!c || !f0 || !f1) { set_error("foto_bb_reset_dev: null argument"); return FOTO_ERR_ARG; }
    if (c->rccl) {
        set_error("foto_bb_reset_dev: device buffers are not supported on RCCL-sharded contexts");
        return FOTO_ERR_STATE;
    }
    // (argument errors leave the context as it was: nothing is drained, reset or enqueued yet)
    const int dev = stream_device(c->s);
    FOTO_TRY(image_dev_check(f0, c->Nx, c->Ny, dev, "foto_bb_reset_dev (f0)"));
    FOTO_TRY(image_dev_check(f1, c->Nx, c->Ny, dev, "foto_bb_reset_dev (f1)"));
    const RhoSrc src = dev_src(f0, f1, normalize, stream);
    FOTO_TRY(bb_reset(c, src));
    return dev_src_done(c, src, sums2_or_null);
}

int foto_bb_flow_dev(foto_bb_ctx* c, void* out, int dtype, int layout, void* stream) {
    if (!c) { set_error("null ctx"); return FOTO_ERR_ARG; }
    if (c->rccl) {
        set_error("foto_bb_flow_dev: device buffers are not supported on RCCL-sharded contexts");
        return FOTO_ERR_STATE;
    }
    FOTO_TRY(path_state_check(c, "foto_bb_flow_dev"));   // (the two above: this entry's own wording)
    FOTO_TRY(export_check(out, dtype, layout, (int64_t)c->Nx * c->Ny, stream_device(c->s), "foto_bb_flow_dev"));
    Completed k;
    FOTO_TRY(completed_state(c, "foto_bb_flow_dev", &k));
    const FlowDev dv{out, dtype, layout, (hipStream_t)stream};
    FOTO_TRY(flow(c, k, nullptr, nullptr, nullptr, &dv));
    return c->link.leave(c->s, dv.user);
}

int foto_bb_flow(foto_bb_ctx* c, double* u, double* v, double* m) {
    if (!c) { set_error("null ctx"); return FOTO_ERR_ARG; }
    if (c->broken) { set_error("foto_bb_flow: a failed foto_bb_iterate left the context inconsistent; foto_bb_reset it"); return FOTO_ERR_STATE; }
    Completed k;   // (pipelined loop, from the callback: the completed iteration's phi)
    FOTO_TRY(completed_state(c, "foto_bb_flow", &k));
    return flow(c, k, u, v, m);
}

static int flow_path_entry(foto_bb_ctx* c, double* u, double* v, double* m, const FlowDev* dv, const char* who) {
    FOTO_TRY(path_state_check(c, who));
    if (dv) {
        FOTO_TRY(export_check(dv->out, dv->dtype, dv->layout, (int64_t)c->Nx * c->Ny * (c->Nt - 1),
                              stream_device(c->s), who));
    } else if (!u || !v || !m) {
        set_error("%s: null pointer", who);
        return FOTO_ERR_ARG;
    }
    Completed k;
    FOTO_TRY(completed_state(c, who, &k));
    return flow_path(c, k, u, v, m, dv);
}

int foto_bb_flow_path(foto_bb_ctx* c, double* u, double* v, double* m) {
    return flow_path_entry(c, u, v, m, nullptr, "foto_bb_flow_path");
}

int foto_bb_flow_path_dev(foto_bb_ctx* c, void* out, int dtype, int layout, void* stream) {
    const FlowDev dv{out, dtype, layout, (hipStream_t)stream};
    return flow_path_entry(c, nullptr, nullptr, nullptr, &dv, "foto_bb_flow_path_dev");
}

// ------------------------------------------------------------------ point tracking
// Plane n's trajectory step reads phi plane n of the shard that owns it (shard 0: the completed
// iteration's phi, as flow_path): one launch per run of planes in one buffer, so one launch on a
// one-shard context.  Between launches the float64 positions travel through the TRK_POS scratch
// -- positions rebuilt from stored displacements ((x - x0) + x0) would not have the same bits.
static bool track_needs_pos(foto_bb_ctx* c) {
    Shard* sp = plane_owner(c, 0);
    return sp && sp->g.t0 + sp->g.nloc < c->Nt - 1;
}

static int track_run(foto_bb_ctx* c, const Completed& k, const void* pts, int pts_dtype, int64_t M, int all_steps,
                     void* out, int dtype) {
    const int last = c->Nt - 1;
    double* const pos = (double*)c->trk[foto_bb_ctx::TRK_POS].p;
    for (int n = 0; n < last;) {
        Shard* sp = plane_owner(c, n);
        if (!sp) { set_error("point tracking: no local shard owns plane %d", n); return FOTO_ERR_STATE; }
        const int n_hi = std::min(sp->g.t0 + sp->g.nloc, last);
        FOTO_HIP_CHECK(launch_track(sp->g, k.of(*sp).phi, n, n_hi, pts, pts_dtype, n == 0 ? nullptr : pos,
                                    n_hi == last ? nullptr : pos, out, dtype, M, all_steps, c->s));
        n = n_hi;
    }
    return 0;
}

int foto_bb_track(foto_bb_ctx* c, const double* pts, int64_t M, int all_steps, double* out) {
    const char* who = "foto_bb_track";
    FOTO_TRY(path_state_check(c, who));
    FOTO_TRY(track_arg_check(pts, out, M, all_steps, who));
    Completed k;
    FOTO_TRY(completed_state(c, who, &k));
    const size_t np = 2 * (size_t)M, nr = np * (size_t)(all_steps ? c->Nt - 1 : 1);
    FOTO_TRY(c->trk[foto_bb_ctx::TRK_PTS].reserve(np * sizeof(double), c->s));
    FOTO_TRY(c->trk[foto_bb_ctx::TRK_OUT].reserve(nr * sizeof(double), c->s));
    if (track_needs_pos(c)) FOTO_TRY(c->trk[foto_bb_ctx::TRK_POS].reserve(np * sizeof(double), c->s));
    double* dp = (double*)c->trk[foto_bb_ctx::TRK_PTS].p;
    double* dout = (double*)c->trk[foto_bb_ctx::TRK_OUT].p;
    FOTO_HIP_CHECK(hipMemcpyAsync(dp, pts, np * sizeof(double), hipMemcpyHostToDevice, c->s));
    FOTO_TRY(track_run(c, k, dp, FOTO_F64, M, all_steps, dout, FOTO_F64));
    FOTO_HIP_CHECK(hipMemcpyAsync(out, dout, nr * sizeof(double), hipMemcpyDeviceToHost, c->s));
    FOTO_HIP_CHECK(hipStreamSynchronize(c->s));
    return 0;
}

int foto_bb_track_dev(foto_bb_ctx* c, const void* pts, int pts_dtype, int64_t M, int all_steps, void* out, int dtype,
                      void* stream) {
    const char* who = "foto_bb_track_dev";
    FOTO_TRY(path_state_check(c, who));
    FOTO_TRY(track_arg_check(pts, out, M, all_steps, who));
    FOTO_TRY(track_dtype_check(pts, pts_dtype, who, "pts"));
    FOTO_TRY(track_dtype_check(out, dtype, who, "out"));
    const size_t np = 2 * (size_t)M, nr = np * (size_t)(all_steps ? c->Nt - 1 : 1);
    const int dev = stream_device(c->s);
    FOTO_TRY(dev_ptr_check(pts, np * dtype_bytes(pts_dtype), dev, who, "pts"));
    FOTO_TRY(dev_ptr_check(out, nr * dtype_bytes(dtype), dev, who, "out"));
    Completed k;
    FOTO_TRY(completed_state(c, who, &k));
    if (track_needs_pos(c))   // (virtual ranks only)
        FOTO_TRY(c->trk[foto_bb_ctx::TRK_POS].reserve(np * sizeof(double), c->s));
    FOTO_TRY(c->link.enter((hipStream_t)stream, c->s));   // (before the first read of `pts` / write of `out`)
    FOTO_TRY(track_run(c, k, pts, pts_dtype, M, all_steps, out, dtype));
    return c->link.leave(c->s, (hipStream_t)stream);
}

// ------------------------------------------------------------------ maps and in-betweens
// The table of phi's Nt plane pointers for this call: plane m lives in the shard that owns it, in
// whichever of its two phi buffers holds the completed iteration (k.of(): shard 0's record of the
// iteration in flight, when the default loop's callback calls).  Filled on the stream, ahead of the
// launches that read it; an earlier call's launches are ahead of the refill on the same stream.
static int plane_table(foto_bb_ctx* c, const Completed& k, const double* const** table) {
    DevScratch& tab = c->itp[foto_bb_ctx::ITP_TAB];
    FOTO_TRY(tab.reserve((size_t)c->Nt * sizeof(double*), c->s));
    int covered = 0;
    PlaneSegs sg;
    sg.n = 0;
    for (auto& sp : c->sh) {
        sg.base[sg.n] = k.of(*sp).phi;
        sg.t0[sg.n] = sp->g.t0;
        sg.nloc[sg.n] = sp->g.nloc;
        covered += sp->g.nloc;
        if (++sg.n == PLANE_SEGS || sp == c->sh.back()) {
            FOTO_HIP_CHECK(launch_plane_table(sg, (int64_t)c->Nx * c->Ny, (const double**)tab.p, c->s));
            sg.n = 0;
        }
    }
    if (covered != c->Nt) { set_error("maps: the local shards own %d of %d planes", covered, c->Nt); return FOTO_ERR_STATE; }
    *table = (const double* const*)tab.p;
    return 0;
}

// records [k0, k0 + cnt) of every launch: MAPS_MAX times each
static int maps_run(foto_bb_ctx* c, const double* const* table, const double* s, int count, int inv_iters, void* out,
                    int dtype) {
    const size_t rec = 4 * (size_t)c->Nx * c->Ny * dtype_bytes(dtype);
    for (int k0 = 0; k0 < count; k0 += MAPS_MAX)
        FOTO_HIP_CHECK(launch_maps(table, c->Nt, c->Nx, c->Ny, s + k0, std::min(MAPS_MAX, count - k0), inv_iters,
                                   (char*)out + (size_t)k0 * rec, dtype, c->s));
    return 0;
}

int foto_bb_maps(foto_bb_ctx* c, const double* s, int count, int inv_iters, double* out) {
    const char* who = "foto_bb_maps";
    FOTO_TRY(path_state_check(c, who));
    FOTO_TRY(maps_arg_check(s, out, count, inv_iters, c->Nt, who));
    Completed k;
    FOTO_TRY(completed_state(c, who, &k));
    const size_t bytes = (size_t)count * 4 * (size_t)c->Nx * c->Ny * sizeof(double);
    FOTO_TRY(c->itp[foto_bb_ctx::ITP_OUT].reserve(bytes, c->s));
    const double* const* table = nullptr;
    FOTO_TRY(plane_table(c, k, &table));
    void* dout = c->itp[foto_bb_ctx::ITP_OUT].p;
    FOTO_TRY(maps_run(c, table, s, count, inv_iters, dout, FOTO_F64));
    FOTO_HIP_CHECK(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, c->s));
    FOTO_HIP_CHECK(hipStreamSynchronize(c->s));
    return 0;
}

int foto_bb_maps_dev(foto_bb_ctx* c, const double* s, int count, int inv_iters, void* out, int dtype, void* stream) {
    const char* who = "foto_bb_maps_dev";
    FOTO_TRY(path_state_check(c, who));
    FOTO_TRY(maps_arg_check(s, out, count, inv_iters, c->Nt, who));
    if (dtype != FOTO_F32 && dtype != FOTO_F64) {
        set_error("%s: dtype %d is not FOTO_F32 / FOTO_F64", who, dtype);
        return FOTO_ERR_ARG;
    }
    if ((uintptr_t)out % dtype_bytes(dtype) != 0) {
        set_error("%s: out %p is not aligned to its %zu-byte element", who, out, dtype_bytes(dtype));
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(dev_ptr_check(out, (size_t)count * 4 * (size_t)c->Nx * c->Ny * dtype_bytes(dtype), stream_device(c->s),
                           who, "out"));
    Completed k;
    FOTO_TRY(completed_state(c, who, &k));
    const double* const* table = nullptr;
    FOTO_TRY(plane_table(c, k, &table));
    FOTO_TRY(c->link.enter((hipStream_t)stream, c->s));   // (before the first write of `out`)
    FOTO_TRY(maps_run(c, table, s, count, inv_iters, out, dtype));
    return c->link.leave(c->s, (hipStream_t)stream);
}

int foto_bb_interp_dev(foto_bb_ctx* c, const foto_image* f0, const foto_image* f1, int channels, int64_t stride_c0,
                       int64_t stride_c1, const double* s, int count, int inv_iters, void* out, int out_dtype,
                       void* stream) {
    const char* who = "foto_bb_interp_dev";
    FOTO_TRY(path_state_check(c, who));
    // ---- host-only checks
    if (!f0 || !f1) { set_error("%s: null pointer", who); return FOTO_ERR_ARG; }
    FOTO_TRY(maps_arg_check(s, out, count, inv_iters, c->Nt, who));
    FOTO_TRY(interp_frame_check(f0, channels, stride_c0, c->Nx, c->Ny, who));
    FOTO_TRY(interp_frame_check(f1, channels, stride_c1, c->Nx, c->Ny, who));
    if (out_dtype < FOTO_U8 || out_dtype > FOTO_F64) {
        set_error("%s: out_dtype %d is not FOTO_U8 / FOTO_F32 / FOTO_F64", who, out_dtype);
        return FOTO_ERR_ARG;
    }
    if ((uintptr_t)out % dtype_bytes(out_dtype) != 0) {
        set_error("%s: out %p is not aligned to its %zu-byte element", who, out, dtype_bytes(out_dtype));
        return FOTO_ERR_ARG;
    }
    // ---- the pointer queries, before anything is enqueued
    const int dev = stream_device(c->s);
    const size_t b0 = interp_frame_bytes(f0, channels, stride_c0, c->Nx, c->Ny);
    const size_t b1 = interp_frame_bytes(f1, channels, stride_c1, c->Nx, c->Ny);
    const size_t img = (size_t)c->Nx * c->Ny * (size_t)channels * dtype_bytes(out_dtype);
    FOTO_TRY(dev_ptr_check(f0->data, b0, dev, who, "frame 0 (all channels)"));
    FOTO_TRY(dev_ptr_check(f1->data, b1, dev, who, "frame 1 (all channels)"));
    FOTO_TRY(dev_ptr_check(out, (size_t)count * img, dev, who, "out"));
    if (overlaps(out, (size_t)count * img, f0->data, b0) || overlaps(out, (size_t)count * img, f1->data, b1)) {
        set_error("%s: out may not overlap a frame (the in-between gathers)", who);
        return FOTO_ERR_ARG;
    }
    Completed k;
    FOTO_TRY(completed_state(c, who, &k));
    const double* const* table = nullptr;
    FOTO_TRY(plane_table(c, k, &table));
    FOTO_TRY(c->link.enter((hipStream_t)stream, c->s));   // (before the first read of a frame / write of `out`)
    for (int k0 = 0; k0 < count; k0 += MAPS_MAX)
        FOTO_HIP_CHECK(launch_interp(table, c->Nt, c->Nx, c->Ny, *f0, stride_c0, *f1, stride_c1, channels, s + k0,
                                     std::min(MAPS_MAX, count - k0), inv_iters, (char*)out + (size_t)k0 * img, out_dtype,
                                     c->s));
    return c->link.leave(c->s, (hipStream_t)stream);
}

int foto_bb_report(foto_bb_ctx* c, double* out) {
    const char* who = "foto_bb_report";
    FOTO_TRY(path_state_check(c, who));
    if (!out) { set_error("%s: null pointer", who); return FOTO_ERR_ARG; }
    Completed k;
    FOTO_TRY(completed_state(c, who, &k));
    double* table = nullptr;
    FOTO_TRY(report_run(c, k, nullptr, &table));
    FOTO_HIP_CHECK(hipMemcpyAsync(out, table, (size_t)c->Nt * FOTO_REPORT_COLS * sizeof(double),
                                  hipMemcpyDeviceToHost, c->s));
    FOTO_HIP_CHECK(hipStreamSynchronize(c->s));
    return 0;
}

int foto_bb_report_dev(foto_bb_ctx* c, double* out, void* stream) {
    const char* who = "foto_bb_report_dev";
    FOTO_TRY(path_state_check(c, who));
    if (!out) { set_error("%s: null pointer", who); return FOTO_ERR_ARG; }
    if ((uintptr_t)out % sizeof(double) != 0) {
        set_error("%s: out %p is not aligned to its 8-byte element", who, (void*)out);
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(dev_ptr_check(out, (size_t)c->Nt * FOTO_REPORT_COLS * sizeof(double), stream_device(c->s), who, "out"));
    Completed k;
    FOTO_TRY(completed_state(c, who, &k));
    FOTO_TRY(c->link.enter((hipStream_t)stream, c->s));   // (before the first write of `out`)
    FOTO_TRY(report_run(c, k, out, nullptr));
    return c->link.leave(c->s, (hipStream_t)stream);
}

int foto_bb_frames(foto_bb_ctx* c, const double* s, int count, double scale, double* out) {
    FOTO_TRY(frames_check(c, s, count, scale, out, FOTO_F64, "foto_bb_frames"));
    Completed k;
    FOTO_TRY(completed_state(c, "foto_bb_frames", &k));
    // one frame at a time through shard 0's fu (a plane of float64 the flow extraction rewrites)
    Shard& s0 = *c->sh[0];
    const int64_t nxy = (int64_t)c->Nx * c->Ny;
    for (int i = 0; i < count; ++i) {
        FOTO_TRY(frames_launch(c, k, s + i, 1, scale, s0.fu, FOTO_F64));
        FOTO_HIP_CHECK(hipMemcpyAsync(out + (int64_t)i * nxy, s0.fu, nxy * sizeof(double), hipMemcpyDeviceToHost,
                                      c->s));
    }
    FOTO_HIP_CHECK(hipStreamSynchronize(c->s));
    return 0;
}

int foto_bb_frames_dev(foto_bb_ctx* c, const double* s, int count, double scale, void* out, int dtype,
                       void* stream) {
    const char* who = "foto_bb_frames_dev";
    FOTO_TRY(frames_check(c, s, count, scale, out, dtype, who));
    const int64_t nxy = (int64_t)c->Nx * c->Ny;
    const size_t fb = (size_t)nxy * dtype_bytes(dtype);
    if ((uintptr_t)out % dtype_bytes(dtype) != 0) {
        set_error("%s: out %p is not aligned to its %zu-byte element", who, out, dtype_bytes(dtype));
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(dev_ptr_check(out, (size_t)count * fb, stream_device(c->s), who, "out"));
    Completed k;
    FOTO_TRY(completed_state(c, who, &k));
    FOTO_TRY(c->link.enter((hipStream_t)stream, c->s));   // (before the first write of `out`)
    for (int k0 = 0; k0 < count; k0 += FRAMES_MAX) {      // (one launch for count <= FRAMES_MAX)
        const int cnt = std::min(FRAMES_MAX, count - k0);
        FOTO_TRY(frames_launch(c, k, s + k0, cnt, scale, (char*)out + (size_t)k0 * fb, dtype));
    }
    return c->link.leave(c->s, (hipStream_t)stream);
}

int foto_bb_shard(const foto_bb_ctx* c, int* t0, int* nloc) {
    if (!c) return FOTO_ERR_ARG;
    if (c->rccl) { *t0 = c->sh[0]->g.t0; *nloc = c->sh[0]->g.nloc; }
    else { *t0 = 0; *nloc = c->Nt; }
    return 0;
}

int foto_bb_comm_size(const foto_bb_ctx* c, int* nranks) {
    if (!c || !nranks) return FOTO_ERR_ARG;
    *nranks = 0;
    if (c->rccl && c->nc) FOTO_NCCL_CHECK(ncclCommCount(c->nc, nranks));
    return 0;
}

int foto_bb_get_phi(foto_bb_ctx* c, double* phi) {
    if (!c || !phi) return FOTO_ERR_ARG;
    Completed k;
    FOTO_TRY(completed_state(c, "foto_bb_get_phi", &k));
    size_t off = 0;
    for (auto& sp : c->sh) {
        const size_t n = (size_t)sp->g.nloc * sp->g.nxy;
        FOTO_HIP_CHECK(hipMemcpyAsync(phi + off, k.of(*sp).phi, n * sizeof(double), hipMemcpyDeviceToHost, c->s));
        off += n;
    }
    FOTO_HIP_CHECK(hipStreamSynchronize(c->s));
    return 0;
}

int foto_bb_get_state(foto_bb_ctx* c, double* mu3, double* q3) {
    if (!c) return FOTO_ERR_ARG;
    Completed k;
    FOTO_TRY(completed_state(c, "foto_bb_get_state", &k));
    if (q3 && c->fuse && c->have_phi) {   // the fused kernel never stores q: recompute it (bit-identical)
        for (auto& sp : c->sh) {   // (phi's halo planes are the ones the last prox read)
            Shard& s = *sp;
            const Rot& ks = k.of(s);
            double* const* src = ks.fz_src;
            if (!src[0]) continue;
            FOTO_HIP_CHECK(launch_q_from_phi(s.g, ks.phi, src[0], src[1], src[2], s.q[0], s.q[1],
                                             s.q[2], c->r, c->s));
        }
    }
    size_t tot = 0;
    for (auto& sp : c->sh) tot += (size_t)sp->g.nloc * sp->g.nxy;
    for (int f = 0; f < 3; ++f) {
        size_t off = 0;
        for (auto& sp : c->sh) {
            const size_t n = (size_t)sp->g.nloc * sp->g.nxy;
            if (mu3)
                FOTO_HIP_CHECK(hipMemcpyAsync(mu3 + f * tot + off, k.of(*sp).mu[f], n * 8, hipMemcpyDeviceToHost, c->s));
            if (q3) FOTO_HIP_CHECK(hipMemcpyAsync(q3 + f * tot + off, sp->q[f], n * 8, hipMemcpyDeviceToHost, c->s));
            off += n;
        }
    }
    FOTO_HIP_CHECK(hipStreamSynchronize(c->s));
    return 0;
}

int foto_bb_stats_get(const foto_bb_ctx* c, foto_bb_stats* st) {
    if (!c || !st) return FOTO_ERR_ARG;
    *st = c->st;
    for (int k = 0; k < 8; ++k) { st->n_k[k] = c->kt.n[k]; st->ms_k[k] = c->kt.ms[k]; st->bytes_k[k] = c->kt.bytes[k]; }
    return 0;
}

int foto_bb_stats_reset(foto_bb_ctx* c) {
    if (!c) return FOTO_ERR_ARG;
    const int oi = c->st.outer_iters;
    memset(&c->st, 0, sizeof(c->st));
    c->st.outer_iters = oi;
    c->kt.reset();
    return 0;
}

int foto_bb_set_timing(foto_bb_ctx* c, int on) {
    if (!c) return FOTO_ERR_ARG;
    c->kt.on = on != 0;
    return 0;
}

int foto_bb_sync(foto_bb_ctx* c) {
    if (!c) return FOTO_ERR_ARG;
    FOTO_HIP_CHECK(hipStreamSynchronize(c->s));
    return 0;
}

void foto_bb_destroy(foto_bb_ctx* c) { delete c; }

int foto_bb_solve(const double* rho0, const double* rhoT, int Nt, int Nx, int Ny, double r, double tol, double eps,
                  int max_it, foto_bb_iter_cb cb, void* user, double* u, double* v, double* m) {
    foto_bb_ctx* c = nullptr;
    FOTO_TRY(foto_bb_create(rho0, rhoT, Nt, Nx, Ny, r, eps, nullptr, &c));
    int done = 0;
    int rc = foto_bb_iterate(c, max_it, tol, 1, cb, user, &done);
    if (rc >= 0) rc = foto_bb_flow(c, u, v, m);
    if (rc >= 0) rc = foto_bb_sync(c);
    foto_bb_destroy(c);
    return rc < 0 ? rc : 0;
}

namespace {
struct SolveLog {
    foto_bb_solve_stats* st;
    int n = 0;
    int64_t cg = 0;
};
void solve_log_cb(void* user, int, double crit, int its, int info) {
    SolveLog* L = (SolveLog*)user;
    foto_bb_solve_stats* st = L->st;
    if (st && L->n < st->cap) {
        if (st->crit) st->crit[L->n] = crit;
        if (st->cg_its) st->cg_its[L->n] = its;
        if (st->cg_info) st->cg_info[L->n] = info;
    }
    L->n += 1;
    L->cg += its;
}
double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
}  // namespace

int foto_bb_solve_ex(const double* rho0, const double* rhoT, int Nt, int Nx, int Ny, double r, double tol, double eps,
                     int max_it, const foto_bb_opts* opts, double* u, double* v, double* m, double* phi_or_null,
                     foto_bb_solve_stats* st) {
    if (max_it <= 0) {
        set_error("max_it = %d: the reference's loop never runs and phi is unbound (benamou_brenier.py:271, "
                  "UnboundLocalError)", max_it);
        return FOTO_ERR_STATE;
    }
    if (st) {   // (the caller's arrays and cap stay; every output field starts at zero)
        const foto_bb_solve_stats keep = *st;
        memset(st, 0, sizeof(*st));
        st->cap = std::max(0, keep.cap);
        st->crit = keep.crit; st->cg_its = keep.cg_its; st->cg_info = keep.cg_info;
    }
    auto t0 = std::chrono::steady_clock::now();
    foto_bb_ctx* c = nullptr;
    FOTO_TRY(foto_bb_create(rho0, rhoT, Nt, Nx, Ny, r, eps, opts, &c));
    std::unique_ptr<foto_bb_ctx> guard(c);
    if (st) st->ms_create = ms_since(t0);
    SolveLog L{st};
    int done = 0;
    t0 = std::chrono::steady_clock::now();
    const int rc = foto_bb_iterate(c, max_it, tol, 1, solve_log_cb, &L, &done);
    if (rc < 0) return rc;
    FOTO_TRY(foto_bb_sync(c));
    const double ms_loop = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    FOTO_TRY(foto_bb_flow(c, u, v, m));
    if (phi_or_null) FOTO_TRY(foto_bb_get_phi(c, phi_or_null));
    FOTO_TRY(foto_bb_sync(c));
    if (st) {
        st->ms_flow = ms_since(t0);
        st->ms_loop = ms_loop;
        st->outer_iters = L.n;
        st->stopped = rc;
        FOTO_TRY(foto_bb_shard(c, &st->phi_t0, &st->phi_nloc));
        FOTO_TRY(foto_bb_stats_get(c, &st->bb));
        // the algorithmic bytes of one outer iteration on this rank: the default path's itemised
        // 188 B per voxel (bench.py STEP_BYTES_PER_VOXEL), the literal stencil
        // CG's (21 + 10 k) 8 B; the other modes from the kernel timers
        const double nv = (double)st->phi_nloc * (double)Nx * (double)Ny;
        if (c->o.cg_mode == 3) st->alg_bytes_per_iter = 188.0 * nv;
        else if (c->o.cg_mode == 0 && L.n > 0) st->alg_bytes_per_iter = (21.0 + 10.0 * (double)L.cg / L.n) * 8.0 * nv;
        else if (L.n > 0) {
            double b = 0;
            for (int k = 0; k < 8; ++k) b += st->bb.bytes_k[k];   // (summed over the launches)
            st->alg_bytes_per_iter = b / L.n;   // (0 without opts->timing)
        }
    }
    return 0;
}

}  // extern "C"

extern "C" int foto_cg(const double* b, int Nt, int Nx, int Ny, double r, double eps, double rtol, int maxiter, int mode,
                       double* x, int* iterations) {
    if (!b || !x) { set_error("null argument"); return FOTO_ERR_ARG; }
    FOTO_TRY(grid_size_check(Nt, Nx, Ny, "foto_cg"));
    const int64_t nxy = (int64_t)Nx * Ny, N = nxy * Nt;
    std::vector<double> z((size_t)nxy, 0.0);
    foto_bb_opts o;
    foto_bb_opts_default(&o);
    o.cg_rtol = rtol;
    o.cg_maxiter = maxiter;
    o.cg_mode = mode;
    foto_bb_ctx* c = nullptr;
    FOTO_TRY(foto_bb_create(z.data(), z.data(), Nt, Nx, Ny, r, eps, &o, &c));
    std::unique_ptr<foto_bb_ctx> guard(c);
    Shard& s = *c->sh[0];
    FOTO_HIP_CHECK(hipMemcpyAsync(s.rv, b, N * sizeof(double), hipMemcpyHostToDevice, c->s));
    FOTO_HIP_CHECK(launch_dot_self(N, s.rv, s.rb, s.gath_rr(), 0, c->s));
    int its = 0, info = 0;
    FOTO_TRY(cg_solve(c, &its, &info));
    FOTO_HIP_CHECK(hipMemcpyAsync(x, s.phi, N * sizeof(double), hipMemcpyDeviceToHost, c->s));
    FOTO_HIP_CHECK(hipStreamSynchronize(c->s));
    if (iterations) *iterations = its;
    return info;
}

// ctypes mirrors these layouts (foto/_lib.py); tests/test_cabi.py checks the Python side.
static_assert(sizeof(foto_bb_opts) == 48, "foto_bb_opts layout");
static_assert(offsetof(foto_bb_stats, n_k) == 56, "foto_bb_stats layout");
static_assert(sizeof(foto_bb_stats) == 256, "foto_bb_stats layout");
static_assert(offsetof(foto_bb_solve_stats, ms_create) == 48 && offsetof(foto_bb_solve_stats, bb) == 80 &&
                  sizeof(foto_bb_solve_stats) == 336,
              "foto_bb_solve_stats layout");
static_assert(sizeof(foto_gn_stats) == 48, "foto_gn_stats layout");
