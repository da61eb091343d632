// Device-wide sums and the wave primitives under them, each defined once: the last-block
// reductions of foto_kernels.hip, foto_spectral.hip (with foto_gauss.inc) and foto_gn.hip, the
// hand-off between blocks they all rely on (k_report's per-plane tickets included), the DPP /
// readlane wrappers with the row tree, and the Chebyshev-moment accumulation of the s-step CG.
// A file of its own, not a part of foto_devutil.h: that header serves units that never reduce
// across blocks and knows nothing of RedBuf or NT (foto_internal.h).  crit, the CG counts and
// phi are reproducible because every global sum runs the one definition here.
// What the s-step kernels do with their summed moments (slot of the all-gather or plan) needs
// the planner and stays with it in foto_spectral.hip (moments_handed_over).
//
// The kernels built from these helpers compile to the instructions they had when each unit
// carried its own copy (profiles/reduce_refactor_resources.txt).  That was not free: hipcc's
// output moved with the shape of a helper (a branch sense, a by-reference argument), so after
// changing one, compare the device assembly of the three units again.
#pragma once

#include "foto_internal.h"

namespace foto {

// ============================================================================ hand-off between blocks
// A block stores its partials write-through (relaxed agent-scope stores: sc1), drains them
// (vmcnt(0)) and adds one agent-scope ticket; the block whose add comes last reads all
// partials with sc1 loads after a barrier and puts the ticket back to 0 for the next launch
// (MI355X_MICROARCH.md "Valid forms" row 1).

__device__ __forceinline__ void partial_store(double* p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double partial_load(const double* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Drain, take a ticket, am I last: one thread of the wave that stored the block's partials; true
// in the last of the n blocks that share `ticket`.  The wait is the wave's, so where several
// lanes of one wave store the partials (grid_reduce_last_rs) that wave drains once and one lane
// adds: the two halves are there for that caller alone.
__device__ __forceinline__ void partials_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ bool ticket_add_last(unsigned* ticket, int n) {
    return __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(n - 1);
}
__device__ __forceinline__ bool ticket_take_last(unsigned* ticket, int n) {
    partials_drain();
    return ticket_add_last(ticket, n);
}
__device__ __forceinline__ void ticket_reset(unsigned* ticket) {
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ============================================================================ last-block reduction

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// Fixed-tree block sum of K values; result valid in thread 0.  `sh` holds K*NTH/64 doubles.
template <int K, int NTH = NT>
__device__ __forceinline__ void block_sum(double (&v)[K], double* sh) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        v[k] = wave_sum(v[k]);
        if (lane == 0) sh[k * (NTH / 64) + w] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double s = sh[k * (NTH / 64)];
#pragma unroll
            for (int j = 1; j < NTH / 64; ++j) s += sh[k * (NTH / 64) + j];
            v[k] = s;
        }
    }
}

// Every block contributes v[K]; the block whose ticket add comes last sums all block
// partials in block order (deterministic) and returns true with the totals in thread 0.
template <int K, int NTH = NT>
__device__ bool grid_reduce_last(double (&v)[K], RedBuf rb, double (&tot)[K]) {
    __shared__ double sh[K * (NTH / 64)];
    __shared__ int is_last;
    block_sum<K, NTH>(v, sh);
    const int nb = gridDim.x;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) partial_store(&rb.partials[(int64_t)k * nb + blockIdx.x], v[k]);
        is_last = ticket_take_last(rb.ticket, nb);
    }
    __syncthreads();
    if (!is_last) return false;
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (int i = threadIdx.x; i < nb; i += NTH) {
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += partial_load(&rb.partials[(int64_t)k * nb + i]);
    }
    block_sum<K, NTH>(acc, sh);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) tot[k] = acc[k];
        ticket_reset(rb.ticket);
    }
    return true;
}

// ============================================================================ reduce-scatter
// Wave-level sum of K per-lane values without LDS: at each xor level a lane keeps one half
// of its remaining values and adds the partner's copy of that half (the partner sends it),
// so the K values halve per level (48 -> 24 -> 12 -> 6 -> 3 over xor 32, 16, 8, 4) and the
// last levels butterfly the remainder.  Lane l ends with the wave totals of quantities
// rs_base(l) + j, j < rs_count<K>(); lanes differing only in the butterflied low bits hold
// identical values.  Every total is a pairwise tree over the 64 lanes: deterministic, and
// (measured in the s-step prototype) as accurate as compensated summation for the moments.
template <int K>
constexpr int rs_levels() {   // halving levels
    int c = K, l = 0;
    while (c % 2 == 0 && l < 6) { c /= 2; ++l; }
    return l;
}
template <int K>
constexpr int rs_count() { return K >> rs_levels<K>(); }

template <int C, int MASK>
__device__ __forceinline__ void rs_halve(double* v, int lane) {
    if constexpr (C % 2 == 0 && MASK >= 1) {
        const bool hi = (lane & MASK) != 0;
#pragma unroll
        for (int j = 0; j < C / 2; ++j) {
            if (j % 8 == 0) asm volatile("" ::: "memory");   // bound batched shuffles (registers)
            const double send = hi ? v[j] : v[C / 2 + j];
            const double keep = hi ? v[C / 2 + j] : v[j];
            v[j] = keep + __shfl_xor(send, MASK, 64);
        }
        rs_halve<C / 2, MASK / 2>(v, lane);
    } else if constexpr (MASK >= 1) {
#pragma unroll
        for (int j = 0; j < C; ++j) v[j] += __shfl_xor(v[j], MASK, 64);
        rs_halve<C, MASK / 2>(v, lane);
    }
}

template <int K>
__device__ __forceinline__ int rs_base(int lane) {
    int base = 0, c = K;
#pragma unroll
    for (int l = 0, mask = 32; l < rs_levels<K>(); ++l, mask >>= 1) {
        c /= 2;
        if (lane & mask) base += c;
    }
    return base;
}

// Block (NTH threads) sum of K values per thread into red[k] (shared, K): reduce-scatter per
// wave, then the waves' partials are added pairwise by K threads.  wred: shared, (NTH/64) * K.
template <int K, int NTH>
__device__ __forceinline__ void blk_sum_rs(double (&v)[K], double* wred, double* out /* shared K */) {
    constexpr int NW = NTH / 64, LEV = rs_levels<K>(), CNT = rs_count<K>();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    rs_halve<K, 32>(v, lane);
    const int base = rs_base<K>(lane);
    const int low = (LEV == 0) ? 63 : ((32 >> (LEV - 1)) - 1);
    if ((lane & low) == 0) {
#pragma unroll
        for (int j = 0; j < CNT; ++j) wred[w * K + base + j] = v[j];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double a[NW];
#pragma unroll
        for (int i = 0; i < NW; ++i) a[i] = wred[i * K + threadIdx.x];
#pragma unroll
        for (int st = 1; st < NW; st *= 2)
#pragma unroll
            for (int i = 0; i + st < NW; i += 2 * st) a[i] += a[i + st];
        out[threadIdx.x] = a[0];
    }
    __syncthreads();
}

// Cross-block sum of K values per thread: block sums by reduce-scatter, k-major partials,
// agent-scope ticket; the last block gathers the partials with 16 threads per quantity
// (16 loads in flight each: one round trip for up to 256 blocks), pairwise throughout.
// With 256-thread blocks and 1024 blocks the gather was 14 us of each pass; with 1024-thread
// blocks (one per CU) and this layout of the loads it is ~3 us.
template <int K, int NTH>
__device__ bool grid_reduce_last_rs(double (&v)[K], RedBuf rb, double* tot /* shared, K */) {
    constexpr int NW = NTH / 64;
    static_assert(K <= 64, "the partials are wave 0's stores: it drains them");
    __shared__ double wred[NW * K];
    __shared__ double bsum[K];
    __shared__ int is_last;
    const int tid = threadIdx.x, nb = gridDim.x;
    blk_sum_rs<K, NTH>(v, wred, bsum);
    if (tid < K) partial_store(&rb.partials[(int64_t)tid * nb + blockIdx.x], bsum[tid]);
    if (tid < 64) {
        partials_drain();   // wave 0's stores drained before its ticket add
        if (tid == 0) is_last = ticket_add_last(rb.ticket, nb);
    }
    __syncthreads();
    if (!is_last) return false;
    // Gather: thread t sums quantity t / 16 over the blocks b = t % 16 + 16 j (16 loads in
    // flight per round, pairwise), then the 16 lanes of a quantity combine by xor butterfly.
    // K * 16 threads per round of quantities (all 48 at once with 1024-thread blocks).
    constexpr int QPR = NTH / 16;   // quantities per round
#pragma unroll
    for (int c = 0; c < K; c += QPR) {
        const int k = c + (tid >> 4), sub = tid & 15;
        double x = 0.0;
        if (k < K) {
            for (int base = 0; base < nb; base += 256) {
                double y[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int b = min(base + sub + 16 * j, nb - 1);
                    y[j] = partial_load(&rb.partials[(int64_t)k * nb + b]);
                }
#pragma unroll
                for (int j = 0; j < 16; ++j) y[j] = (base + sub + 16 * j < nb) ? y[j] : 0.0;
#pragma unroll
                for (int st = 1; st < 16; st *= 2)
#pragma unroll
                    for (int j = 0; j + st < 16; j += 2 * st) y[j] += y[j + st];
                x += y[0];
            }
        }
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
        if (k < K && sub == 0) tot[k] = x;
    }
    __syncthreads();
    if (tid == 0) ticket_reset(rb.ticket);
    return true;
}

// this rank's K totals (shared) into its slot of the buffer the ranks all-gather
template <int K, int NTH>
__device__ __forceinline__ void rank_slot_store(double* gath, int rank, const double* tot) {
    for (int m = threadIdx.x; m < K; m += NTH) gath[rank * K + m] = tot[m];
}

// ============================================================================ DPP and readlane on doubles

__device__ __forceinline__ double dbl_readlane(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffLL), lane);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// Lanes without a source read 0.  On all rows that is bound_ctrl; with a ROWMASK the DPP runs
// on those rows only and the others, like lanes without a source, keep the 0 passed as `old`.
template <int CTRL, int ROWMASK = 0xf>
__device__ __forceinline__ double dbl_dpp(double v) {
    constexpr bool BOUND = ROWMASK == 0xf;
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffLL), CTRL, ROWMASK, 0xf, BOUND);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROWMASK, 0xf, BOUND);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// The row tree, row_shr 1, 2, 4, 8: lane 15 of each 16-lane row ends with its row's sum.
// (k_gq_cg / k_gq_cgtab's reduce2 keeps a written-out copy for its two interleaved chains:
// profiles/reduce_refactor_ab.txt.)
__device__ __forceinline__ void dpp_row_sums(double& v) {
    v += dbl_dpp<0x111>(v);
    v += dbl_dpp<0x112>(v);
    v += dbl_dpp<0x114>(v);
    v += dbl_dpp<0x118>(v);
}

// ============================================================================ Chebyshev moments
// acc[c * NM + m] += T_m(x) w_c, m < NM, over the C channels w = (r r, r q, q q) of the
// s-step CG (C = 3), or r r alone (C = 1): T_0 as a plain add, T_1 and the three-term recurrence
// T_m = 2 x T_{m-1} - T_{m-2} as FMAs.  The rounding of exactly this sequence is what
// DESIGN.md 3.1.1 weighs.
template <int C, int NM>
__device__ __forceinline__ void cheb_moments_acc(double (&acc)[C * NM], double x, double r, double q = 0.0) {
    static_assert(C == 1 || C == 3, "rr alone, or rr, rq, qq");
    const double x2 = x + x;
    const double rr = r * r, rq = r * q, qq = q * q;
    acc[0] += rr;
    if constexpr (C == 3) {
        acc[NM] += rq;
        acc[2 * NM] += qq;
    }
    acc[1] = fma(x, rr, acc[1]);
    if constexpr (C == 3) {
        acc[NM + 1] = fma(x, rq, acc[NM + 1]);
        acc[2 * NM + 1] = fma(x, qq, acc[2 * NM + 1]);
    }
    double tm2 = 1.0, tm1 = x;
#pragma unroll
    for (int m = 2; m < NM; ++m) {
        const double t = fma(x2, tm1, -tm2);
        acc[m] = fma(t, rr, acc[m]);
        if constexpr (C == 3) {
            acc[NM + m] = fma(t, rq, acc[NM + m]);
            acc[2 * NM + m] = fma(t, qq, acc[2 * NM + m]);
        }
        tm2 = tm1;
        tm1 = t;
    }
}

}  // namespace foto
