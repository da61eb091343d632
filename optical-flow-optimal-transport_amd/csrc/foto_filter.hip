// Flow filtering (include/foto.h, "flow filtering"): the guided weighted median of a flow buffer
// and, with unusable pixels at weight zero, hole filling -- one launch of k_median per round.
//
//   staging     a block owns a FT_W x FT_H = 32 x 8 tile (one pixel per thread) and stages it once
//               with its R-wide halo: the two 64-bit keys, the usable byte and up to GUIDE_LDS
//               guide channels as doubles, and the two weight tables.  Halo positions outside the
//               frame are staged as "not usable" (weight 0): no read leaves the frame, nothing is
//               padded.  At R = 7 that is 46 x 22 = 1012 positions, 25 KB with one guide channel
//               (DESIGN.md 3.15 has the budget and the occupancy).  Guide channels past GUIDE_LDS
//               are read from memory at in-frame positions.
//   selection   R <= 2 (<= 25 candidates): one thread per pixel, keys and weights in registers, rank
//               counting: the candidate's cumulative weight is the sum over the keys <= its own.
//               R >= 3 (49 .. 225 candidates): a wave per pixel, 64 pixels in turn; lane l holds
//               candidates l, l + 64, ...; the key is bisected from its top bit with the weight
//               below the trial key summed across the wave (dpp_row_sums of foto_reduce.h, the four
//               row sums by readlane).  Bits on which all weighted candidates agree cannot change
//               the selected sample and are skipped: of a float32 flow that is the 29 low mantissa
//               bits and, usually, the sign and the exponent.
//   sums        weights are uint32 products of two uint16, per-lane partial sums uint64; across the
//               wave they travel as doubles, exact below 2^53 (T < 2^40).
//
// The selected value is one of the samples and the weights are integers, so the result does not
// depend on the order of any sum here: tests/filter_ref.py restates the definition with sorted
// keys and the tests ask for the same bits.  Every index is int64_t.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "foto_devmem.h"
#include "foto_devutil.h"
#include "foto_internal.h"
#include "foto_reduce.h"

namespace foto {

namespace {

typedef unsigned long long u64;

constexpr int FT_W = FOTO_MEDIAN_TILE_W, FT_H = FOTO_MEDIAN_TILE_H;
static_assert(FT_W == 32 && FT_W * FT_H == NT, "one pixel per thread, two tile rows per wave");
constexpr int GUIDE_LDS = 4;                 // guide channels staged on chip
constexpr int SPAT_PAD = 15 * 15 + 1;        // entries of the staged spatial table (even)
constexpr int THREAD_SELECT_MAX_R = 2;       // above it a wave cooperates on a pixel

// Where a round reads the flow of the round before.  Round 1: the caller's buffers; later rounds:
// the state scratch, st = [K][2][n] doubles, su = [K][n] bytes (bit 0: in V_{t-1}, bit 1: in V_0).
struct Src {
    int raw;
    const void* flow;
    int f32, inter;
    int64_t rec;            // elements per record
    const void* mask;       // null: none
    int mask_dtype;
    int64_t msy, msx;
    const double* st;
    const unsigned char* su;
};
struct Guide {
    const void* data;       // channel 0
    int dtype, channels;    // channels 0: no guide
    int64_t sy, sx, sc;
    double divisor;
};
// Where a round writes.  Not the last: the other half of the state scratch.  The last: the
// caller's buffers; m_src is the m plane of a planar input (null: +0.0).
struct Dst {
    int last;
    double* st;
    unsigned char* su;
    void* out;
    int f32, inter;
    int64_t rec;
    unsigned char* valid;
    double* table;
    const void* m_src;
    int m_f32;
    int64_t m_rec;
};

__device__ __forceinline__ u64 key_of(double x) {
    const u64 b = (u64)__double_as_longlong(x);
    return b ^ ((b >> 63) ? ~0ULL : (1ULL << 63));
}
__device__ __forceinline__ double value_of(u64 k) {
    return __longlong_as_double((long long)(k ^ ((k >> 63) ? (1ULL << 63) : ~0ULL)));
}

__device__ __forceinline__ double elem_raw(const void* data, int dtype, int64_t off) {
    if (dtype == FOTO_U8) return (double)((const unsigned char*)data)[off];
    if (dtype == FOTO_F32) return (double)((const float*)data)[off];
    return ((const double*)data)[off];
}
// (double)pixel / divisor of channel c at the in-frame pixel (x, y); x / 1.0 is x, bit for bit
__device__ __forceinline__ double guide_val(const Guide& g, int c, int x, int y) {
    const double v = elem_raw(g.data, g.dtype, (int64_t)c * g.sc + (int64_t)y * g.sy + (int64_t)x * g.sx);
    return g.divisor == 1.0 ? v : v / g.divisor;
}

// The staged tile: LN = (FT_W + 2R)(FT_H + 2R) positions, row pitch LW.
struct Lds {
    u64* kU;
    u64* kV;
    double* gd;               // [cs][LN]
    unsigned short* spat;     // [SPAT_PAD]
    unsigned short* rng;      // [FOTO_MEDIAN_MAX_RANGE]
    unsigned char* us;        // [LN]
    int cs;                   // guide channels staged
};

// G(p, q) of the definition: positions q, p of the staged tile, pixels (qx, qy), (px, py)
template <int LN>
__device__ __forceinline__ unsigned guide_weight(const Lds& L, const Guide& g, int n_range, double scale, int q, int p,
                                                 int qx, int qy, int px, int py) {
    if (g.channels == 0) return 1u;
    double d = 0.0;
    bool bad = false;
    for (int c = 0; c < L.cs; ++c) {
        const double dd = fabs(L.gd[c * LN + q] - L.gd[c * LN + p]);
        bad = bad || dd != dd;
        d = dd > d ? dd : d;
    }
    for (int c = L.cs; c < g.channels; ++c) {
        const double dd = fabs(guide_val(g, c, qx, qy) - guide_val(g, c, px, py));
        bad = bad || dd != dd;
        d = dd > d ? dd : d;
    }
    const double t = floor(d * scale + 0.5);
    const int idx = (bad || !(t < (double)(n_range - 1))) ? n_range - 1 : (int)t;
    return (unsigned)L.rng[idx];
}

// the wave's total of v, in every lane (and scalar): row sums by DPP, the four rows by readlane
__device__ __forceinline__ double wave_total(double v) {
    dpp_row_sums(v);
    return (dbl_readlane(v, 15) + dbl_readlane(v, 31)) + (dbl_readlane(v, 47) + dbl_readlane(v, 63));
}
__device__ __forceinline__ u64 uniform64(u64 v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v & 0xffffffffULL));
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 wave_and(u64 v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v &= __shfl_xor(v, m, 64);
    return uniform64(v);
}
__device__ __forceinline__ u64 wave_or(u64 v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v |= __shfl_xor(v, m, 64);
    return uniform64(v);
}

// The lower weighted median of the wave's candidates (lane slot s: key K[cp + off[s]], weight
// wt[s]), T > 0 their total: the smallest x with 2 cum(x) >= T, cum(x) = the weight of the keys <=
// x.  cum steps only at the key of a weighted candidate, so x is one.  Bits that all weighted keys
// share are x's too; the others are decided from the top: with the higher bits fixed, x has the
// bit clear iff the largest key with it clear already reaches T.
template <int NC>
__device__ __forceinline__ u64 wave_select(const u64* __restrict__ K, int cp, const int (&off)[NC],
                                           const unsigned (&wt)[NC], double T) {
    u64 k[NC], all = ~0ULL, any = 0ULL;
#pragma unroll
    for (int s = 0; s < NC; ++s) {
        k[s] = K[cp + off[s]];
        if (wt[s]) {
            all &= k[s];
            any |= k[s];
        }
    }
    all = wave_and(all);
    any = wave_or(any);
    u64 diff = all ^ any, ans = all;
    while (diff) {
        const u64 bit = 1ULL << (63 - __builtin_clzll(diff));
        diff &= ~bit;
        const u64 trial = ans | (bit - 1);
        u64 part = 0;
#pragma unroll
        for (int s = 0; s < NC; ++s) part += k[s] <= trial ? (u64)wt[s] : 0ULL;
        const double c = wave_total((double)part);
        if (c + c < T) ans |= bit;
    }
    return ans;
}

// One thread, N = (2R + 1)^2 <= 25 candidates around position cp: T, then per component the
// smallest key whose cumulative weight reaches T / 2.  A candidate of weight 0 never wins against
// the weighted candidate below it (which has the same cumulative weight), so none is excluded.
template <int R, int LN>
__device__ __forceinline__ bool thread_select(const Lds& L, const Guide& g, int n_range, double scale, int cp, int px,
                                              int py, u64& rU, u64& rV) {
    constexpr int D = 2 * R + 1, N = D * D, LW = FT_W + 2 * R;
    unsigned wt[N];
    u64 T = 0;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const int dy = c / D - R, dx = c % D - R, q = cp + dy * LW + dx;
        wt[c] = (L.us[q] & 1) ? (unsigned)L.spat[c] * guide_weight<LN>(L, g, n_range, scale, q, cp, px + dx, py + dy, px, py) : 0u;
        T += wt[c];
    }
    if (T == 0) return false;
#pragma unroll 1
    for (int comp = 0; comp < 2; ++comp) {
        const u64* K = comp ? L.kV : L.kU;
        u64 k[N];
#pragma unroll
        for (int c = 0; c < N; ++c) k[c] = K[cp + (c / D - R) * LW + (c % D - R)];
        u64 best = ~0ULL;
#pragma unroll 1
        for (int a = 0; a < N; ++a) {
            const u64 ka = K[cp + (a / D - R) * LW + (a % D - R)];
            u64 cum = 0;
#pragma unroll
            for (int c = 0; c < N; ++c) cum += k[c] <= ka ? (u64)wt[c] : 0ULL;
            if (2 * cum >= T && ka < best) best = ka;
        }
        if (comp) rV = best;
        else rU = best;
    }
    return true;
}

template <class T>
__device__ __forceinline__ void store_uvm(const Dst& d, int64_t r, int64_t n, int64_t p, double u, double v, double m) {
    T* base = (T*)d.out + r * d.rec;
    if (!d.inter) {
        base[p] = (T)u;
        base[n + p] = (T)v;
        base[2 * n + p] = (T)m;
    } else {
        base[2 * p] = (T)u;
        base[2 * p + 1] = (T)v;
    }
}

// One round for the records r0 + blockIdx.y; the tiles of a record are shared out over blockIdx.x.
template <int R>
__global__ __launch_bounds__(NT) void k_median(Src src, Guide g, Dst dst, foto_median_opts o, int64_t r0, int w,
                                               int h, int64_t tiles, int tiles_x, double* partials,
                                               unsigned* tickets) {
    constexpr int D = 2 * R + 1, N = D * D, LW = FT_W + 2 * R, LH = FT_H + 2 * R, LN = LW * LH;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int64_t n = (int64_t)w * h, r = r0 + blockIdx.y;
    Lds L;
    L.cs = g.channels < GUIDE_LDS ? g.channels : GUIDE_LDS;
    L.kU = (u64*)smem;
    L.kV = L.kU + LN;
    L.gd = (double*)(L.kV + LN);
    L.spat = (unsigned short*)(L.gd + (int64_t)L.cs * LN);
    L.rng = L.spat + SPAT_PAD;
    L.us = (unsigned char*)(L.rng + FOTO_MEDIAN_MAX_RANGE);
    for (int i = tid; i < N; i += NT) L.spat[i] = o.spatial[i];
    for (int i = tid; i < FOTO_MEDIAN_MAX_RANGE; i += NT) L.rng[i] = o.range[i];

    const int lx = tid & (FT_W - 1), ly = tid / FT_W;
    const int cmine = (ly + R) * LW + lx + R;   // this thread's pixel in the staged tile
    double acc[4] = {0.0, 0.0, 0.0, 0.0};

    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t tyi = t / tiles_x;
        const int txi = (int)(t - tyi * tiles_x);
        const int x0 = txi * FT_W, y0 = (int)(tyi * FT_H);
        __syncthreads();   // the tables are staged; the tile before is read out
        for (int idx = tid; idx < LN; idx += NT) {
            const int sy = idx / LW, sx = idx - sy * LW;
            const int gx = x0 - R + sx, gy = y0 - R + sy;
            u64 ku = 0, kv = 0;
            unsigned char ub = 0;
            if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
                const int64_t p = (int64_t)gy * w + gx;
                double u, v;
                if (src.raw) {
                    const int64_t iu = r * src.rec + (src.inter ? 2 * p : p), iv = src.inter ? iu + 1 : iu + n;
                    if (src.f32) {
                        u = (double)((const float*)src.flow)[iu];
                        v = (double)((const float*)src.flow)[iv];
                    } else {
                        u = ((const double*)src.flow)[iu];
                        v = ((const double*)src.flow)[iv];
                    }
                    bool ok = isfinite(u) && isfinite(v);
                    if (src.mask) ok = ok && elem_raw(src.mask, src.mask_dtype, gy * src.msy + gx * src.msx) != 0.0;
                    ub = ok ? 3 : 0;
                } else {
                    u = src.st[(r * 2) * n + p];
                    v = src.st[(r * 2 + 1) * n + p];
                    ub = src.su[r * n + p];
                }
                ku = key_of(u);
                kv = key_of(v);
                for (int c = 0; c < L.cs; ++c) L.gd[c * LN + idx] = guide_val(g, c, gx, gy);
            } else {
                for (int c = 0; c < L.cs; ++c) L.gd[c * LN + idx] = 0.0;
            }
            L.kU[idx] = ku;
            L.kV[idx] = kv;
            L.us[idx] = ub;
        }
        __syncthreads();

        // this thread's pixel: what it keeps unless a median replaces it
        u64 myU = L.kU[cmine], myV = L.kV[cmine];
        const int mine = L.us[cmine];
        int in_v = mine & 1;
        const int px = x0 + lx, py = y0 + ly;
        const bool inside = px < w && py < h;

        if constexpr (R <= THREAD_SELECT_MAX_R) {
            if (inside && !(o.fill_only && in_v)) {
                u64 ru = 0, rv = 0;
                if (thread_select<R, LN>(L, g, o.n_range, o.range_scale, cmine, px, py, ru, rv)) {
                    myU = ru;
                    myV = rv;
                    in_v = 1;
                }
            }
        } else {
            // (the slots depend on the lane and R alone, yet stay inside the tile loop: hoisted, they cost
            // the R = 7 instance its fifth wave per SIMD -- 96 -> 100 VGPRs -- for a few divisions per tile)
            constexpr int NC = (N + 63) / 64;
            const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
            int off[NC], ddx[NC], ddy[NC];
            unsigned sp[NC];
#pragma unroll
            for (int s = 0; s < NC; ++s) {
                const int c = lane + 64 * s;
                const bool has = c < N;
                ddy[s] = has ? c / D - R : 0;
                ddx[s] = has ? c % D - R : 0;
                off[s] = ddy[s] * LW + ddx[s];
                sp[s] = has ? (unsigned)L.spat[c] : 0u;
            }
            for (int pi = 0; pi < 64; ++pi) {
                const int qlx = pi & (FT_W - 1), qly = 2 * wv + pi / FT_W;
                const int qx = x0 + qlx, qy = y0 + qly;
                if (qx >= w || qy >= h) continue;   // (the same for the whole wave)
                const int cp = (qly + R) * LW + qlx + R;
                const int cus = __builtin_amdgcn_readfirstlane((int)L.us[cp]);
                if (o.fill_only && (cus & 1)) continue;
                unsigned wt[NC];
                u64 part = 0;
#pragma unroll
                for (int s = 0; s < NC; ++s) {
                    const int q = cp + off[s];
                    wt[s] = (sp[s] && (L.us[q] & 1))
                                ? sp[s] * guide_weight<LN>(L, g, o.n_range, o.range_scale, q, cp, qx + ddx[s], qy + ddy[s], qx, qy)
                                : 0u;
                    part += wt[s];
                }
                const double T = wave_total((double)part);
                if (!(T > 0.0)) continue;
                const u64 ru = wave_select<NC>(L.kU, cp, off, wt, T);
                const u64 rv = wave_select<NC>(L.kV, cp, off, wt, T);
                if (lane == pi) {
                    myU = ru;
                    myV = rv;
                    in_v = 1;
                }
            }
        }

        if (inside) {
            const int64_t p = (int64_t)py * w + px;
            const double u = value_of(myU), v = value_of(myV);
            const int in_v0 = (mine >> 1) & 1;
            if (!dst.last) {
                dst.st[(r * 2) * n + p] = u;
                dst.st[(r * 2 + 1) * n + p] = v;
                dst.su[r * n + p] = (unsigned char)(in_v | (in_v0 << 1));
            } else {
                double m = 0.0;
                if (!dst.inter && dst.m_src) {
                    const int64_t im = r * dst.m_rec + 2 * n + p;
                    m = dst.m_f32 ? (double)((const float*)dst.m_src)[im] : ((const double*)dst.m_src)[im];
                }
                if (dst.f32) store_uvm<float>(dst, r, n, p, u, v, m);
                else store_uvm<double>(dst, r, n, p, u, v, m);
                if (dst.valid) dst.valid[r * n + p] = (unsigned char)in_v;
                acc[0] += in_v0 ? 1.0 : 0.0;
                acc[1] += (!in_v0 && in_v) ? 1.0 : 0.0;
                acc[2] += in_v ? 0.0 : 1.0;
            }
        }
    }
    if (dst.last && dst.table) {
        const RedBuf rb{partials + (int64_t)blockIdx.y * 4 * gridDim.x, tickets + blockIdx.y, 0};
        double tot[4];
        if (grid_reduce_last<4>(acc, rb, tot) && threadIdx.x == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) dst.table[r * 4 + q] = tot[q];
        }
    }
}

// ----------------------------------------------------------------------------- host side

constexpr int MAX_GRID_Y = 65535;   // records per launch

size_t lds_bytes(int R, int channels) {
    const size_t ln = (size_t)(FT_W + 2 * R) * (FT_H + 2 * R);
    const size_t cs = (size_t)std::min(channels, GUIDE_LDS);
    return ln * 16 + cs * ln * 8 + (size_t)(SPAT_PAD + FOTO_MEDIAN_MAX_RANGE) * 2 + ln;
}

void opts_default(foto_median_opts* o) {
    memset(o, 0, sizeof(*o));
    o->radius = 2;
    o->rounds = 1;
    o->fill_only = 0;
    o->n_range = 1;
    o->range_scale = 255.0;
    for (int i = 0; i < 15 * 15; ++i) o->spatial[i] = 1;
    for (int i = 0; i < FOTO_MEDIAN_MAX_RANGE; ++i) o->range[i] = 1;
}

int filter_check(const foto_flow* fl, const foto_image* guide, int channels, int64_t stride_c, const foto_image* mask,
                 int w, int h, const foto_median_opts* o, const char* who) {
    FOTO_TRY(flow_check(fl, w, h, who));
    FOTO_TRY(image_size_check(w, h, 1, who));
    if (guide) FOTO_TRY(interp_frame_check(guide, channels, stride_c, w, h, who));
    if (mask) FOTO_TRY(image_check(mask, w, h, who));
    if (!o) { set_error("%s: opts is null", who); return FOTO_ERR_ARG; }
    if (o->radius < 1 || o->radius > FOTO_MEDIAN_MAX_RADIUS) {
        set_error("%s: radius = %d is outside [1, %d]", who, o->radius, FOTO_MEDIAN_MAX_RADIUS);
        return FOTO_ERR_ARG;
    }
    if (o->rounds < 1 || o->rounds > FOTO_MEDIAN_MAX_ROUNDS) {
        set_error("%s: rounds = %d is outside [1, %d]", who, o->rounds, FOTO_MEDIAN_MAX_ROUNDS);
        return FOTO_ERR_ARG;
    }
    if (o->fill_only != 0 && o->fill_only != 1) {
        set_error("%s: fill_only = %d is not 0 / 1", who, o->fill_only);
        return FOTO_ERR_ARG;
    }
    if (o->n_range < 1 || o->n_range > FOTO_MEDIAN_MAX_RANGE) {
        set_error("%s: n_range = %d is outside [1, %d]", who, o->n_range, FOTO_MEDIAN_MAX_RANGE);
        return FOTO_ERR_ARG;
    }
    if (!std::isfinite(o->range_scale) || !(o->range_scale > 0.0)) {
        set_error("%s: range_scale = %g must be finite and > 0", who, o->range_scale);
        return FOTO_ERR_ARG;
    }
    const int D = 2 * o->radius + 1;
    if (o->spatial[o->radius * D + o->radius] == 0 || o->range[0] == 0) {
        set_error("%s: the centre weight spatial[R][R] and range[0] must be > 0 (a usable pixel keeps a candidate)", who);
        return FOTO_ERR_ARG;
    }
    return 0;
}

// a flow output: dtype F32 | F64, layout 0 | 1, non-null, aligned to its element (foto_chain.hip's rule)
int out_check(const void* out, int dtype, int layout, const double* table, const char* who) {
    if (!out) { set_error("%s: out is null", who); return FOTO_ERR_ARG; }
    if (dtype != FOTO_F32 && dtype != FOTO_F64) {
        set_error("%s: out_dtype %d is not FOTO_F32 / FOTO_F64", who, dtype);
        return FOTO_ERR_ARG;
    }
    if (layout != 0 && layout != 1) {
        set_error("%s: out_layout %d is not 0 (planar u, v, m) / 1 (interleaved (u, v))", who, layout);
        return FOTO_ERR_ARG;
    }
    if ((uintptr_t)out % dtype_bytes(dtype) != 0) {
        set_error("%s: out %p is not aligned to its %zu-byte element", who, out, dtype_bytes(dtype));
        return FOTO_ERR_ARG;
    }
    if (table && (uintptr_t)table % sizeof(double) != 0) {
        set_error("%s: table %p is not aligned to 8 bytes", who, (const void*)table);
        return FOTO_ERR_ARG;
    }
    return 0;
}

size_t mask_span_bytes(const foto_image* im, int w, int h) {
    const size_t last = (size_t)(h - 1) * (size_t)im->stride_y + (size_t)(w - 1) * (size_t)im->stride_x;
    return (last + 1) * dtype_bytes(im->dtype);
}

// One stream, link and scratch set per device, kept for the process (ChainDev's scheme): the call
// only enqueues, nothing waits on the host but a scratch that has to grow.
struct FilterDev {
    hipStream_t s = nullptr;
    StreamLink link;
    DevScratch ctl;     // the tickets of the last round: zeroed per call
    DevScratch work;    // its partials
    DevScratch state;   // the flow between the rounds: two halves of [K][2][n] doubles, then two of [K][n] bytes
};
std::mutex fd_mu;
std::vector<FilterDev*> fd_dev;

int filter_dev(int* device, FilterDev** out) {
    int dev = 0;
    FOTO_HIP_CHECK(hipGetDevice(&dev));
    if ((int)fd_dev.size() <= dev) fd_dev.resize(dev + 1, nullptr);
    if (!fd_dev[dev]) {
        hipStream_t s = nullptr;
        FOTO_TRY(stream_acquire(&s));
        fd_dev[dev] = new FilterDev();
        fd_dev[dev]->s = s;
    }
    *device = dev;
    *out = fd_dev[dev];
    return 0;
}

template <int R>
void launch_round(dim3 grid, size_t lds, hipStream_t s, const Src& src, const Guide& g, const Dst& dst,
                  const foto_median_opts& o, int64_t r0, int w, int h, int64_t tiles, int tiles_x, double* partials,
                  unsigned* tickets) {
    k_median<R><<<grid, NT, lds, s>>>(src, g, dst, o, r0, w, h, tiles, tiles_x, partials, tickets);
}

}  // namespace
}  // namespace foto

using namespace foto;

static_assert(sizeof(foto_median_opts) == 992, "foto_median_opts layout");

extern "C" {

int foto_median_opts_default(foto_median_opts* o) {
    if (!o) { set_error("foto_median_opts_default: null pointer"); return FOTO_ERR_ARG; }
    opts_default(o);
    return 0;
}

int foto_filter_check(const foto_flow* fl, const foto_image* guide_or_null, int channels, int64_t stride_c,
                      const foto_image* mask_or_null, int w, int h, const foto_median_opts* opts) {
    return filter_check(fl, guide_or_null, channels, stride_c, mask_or_null, w, h, opts, "foto_filter_check");
}

int foto_flow_median_dev(const foto_flow* fl, const foto_image* guide, int channels, int64_t stride_c,
                         const foto_image* mask, int w, int h, const foto_median_opts* opts, void* out, int out_dtype,
                         int out_layout, void* valid_out, double* table, void* stream) {
    static const char* const who = "foto_flow_median_dev";
    FOTO_TRY(filter_check(fl, guide, channels, stride_c, mask, w, h, opts, who));
    FOTO_TRY(out_check(out, out_dtype, out_layout, table, who));
    const foto_median_opts o = *opts;
    std::lock_guard<std::mutex> lk(fd_mu);
    int device = 0;
    FilterDev* fd = nullptr;
    FOTO_TRY(filter_dev(&device, &fd));
    const int64_t n = (int64_t)w * h, K = fl->records;
    const size_t in_b = flow_bytes(fl, w, h);
    const size_t g_b = guide ? interp_frame_bytes(guide, channels, stride_c, w, h) : 0;
    const size_t mk_b = mask ? mask_span_bytes(mask, w, h) : 0;
    const size_t out_b = (size_t)K * (out_layout == 0 ? 3 : 2) * (size_t)n * dtype_bytes(out_dtype);
    const size_t v_b = valid_out ? (size_t)K * (size_t)n : 0, t_b = table ? (size_t)K * 4 * sizeof(double) : 0;
    FOTO_TRY(dev_ptr_check(fl->data, in_b, device, who, "flow data"));
    if (guide) FOTO_TRY(dev_ptr_check(guide->data, g_b, device, who, "guide"));
    if (mask) FOTO_TRY(image_dev_check(mask, w, h, device, who));
    FOTO_TRY(dev_ptr_check(out, out_b, device, who, "out"));
    if (valid_out) FOTO_TRY(dev_ptr_check(valid_out, v_b, device, who, "valid_out"));
    if (table) FOTO_TRY(dev_ptr_check(table, t_b, device, who, "table"));
    const void* in[3] = {fl->data, guide ? guide->data : nullptr, mask ? mask->data : nullptr};
    const size_t in_bytes[3] = {in_b, g_b, mk_b};
    const void* outs[3] = {out, valid_out, table};
    const size_t outs_b[3] = {out_b, v_b, t_b};
    for (int k = 0; k < 3; ++k) {
        if (!outs[k]) continue;
        for (int q = 0; q < 3; ++q)
            if (in[q] && overlaps(outs[k], outs_b[k], in[q], in_bytes[q])) {
                set_error("%s: out, valid_out and table may not overlap the flow, the guide or the mask (the filter gathers)", who);
                return FOTO_ERR_ARG;
            }
        for (int q = 0; q < k; ++q)
            if (outs[q] && overlaps(outs[k], outs_b[k], outs[q], outs_b[q])) {
                set_error("%s: out, valid_out and table may not overlap each other", who);
                return FOTO_ERR_ARG;
            }
    }

    hipStream_t s = fd->s;
    const int tiles_x = (w + FT_W - 1) / FT_W;
    const int64_t tiles = (int64_t)tiles_x * ((h + FT_H - 1) / FT_H);
    const int64_t ry_max = std::min<int64_t>(K, MAX_GRID_Y);
    // blocks per record: every block of the last round ends with one returning atomic on its record's ticket
    const unsigned bx = (unsigned)std::min<int64_t>(tiles, std::max<int64_t>(64, 4096 / ry_max));
    const size_t ctl_bytes = (size_t)ry_max * sizeof(unsigned);
    FOTO_TRY(fd->ctl.reserve(ctl_bytes, s));
    FOTO_TRY(fd->work.reserve((size_t)ry_max * 4 * bx * sizeof(double), s));
    const size_t half_d = (size_t)K * 2 * (size_t)n * sizeof(double), half_u = (size_t)K * (size_t)n;
    if (o.rounds > 1) FOTO_TRY(fd->state.reserve(2 * half_d + 2 * half_u, s));
    double* st[2] = {(double*)fd->state.p, (double*)((char*)fd->state.p + half_d)};
    unsigned char* su[2] = {(unsigned char*)fd->state.p + 2 * half_d, (unsigned char*)fd->state.p + 2 * half_d + half_u};

    Guide g{};
    if (guide) g = Guide{guide->data, guide->dtype, channels, guide->stride_y, guide->stride_x, stride_c, guide->divisor};
    const size_t lds = lds_bytes(o.radius, g.channels);
    const int64_t rec_in = (fl->layout == 1 ? 2 : 3) * n;

    FOTO_TRY(fd->link.enter((hipStream_t)stream, s));
    if (table) FOTO_HIP_CHECK(hipMemsetAsync(fd->ctl.p, 0, ctl_bytes, s));
    for (int t = 1; t <= o.rounds; ++t) {
        Src src{};
        src.raw = t == 1;
        if (src.raw) {
            src.flow = fl->data;
            src.f32 = fl->dtype == FOTO_F32;
            src.inter = fl->layout == 1;
            src.rec = rec_in;
            if (mask) {
                src.mask = mask->data;
                src.mask_dtype = mask->dtype;
                src.msy = mask->stride_y;
                src.msx = mask->stride_x;
            }
        } else {
            src.st = st[t & 1];
            src.su = su[t & 1];
        }
        Dst dst{};
        dst.last = t == o.rounds;
        if (!dst.last) {
            dst.st = st[(t + 1) & 1];
            dst.su = su[(t + 1) & 1];
        } else {
            dst.out = out;
            dst.f32 = out_dtype == FOTO_F32;
            dst.inter = out_layout == 1;
            dst.rec = (out_layout == 1 ? 2 : 3) * n;
            dst.valid = (unsigned char*)valid_out;
            dst.table = table;
            if (fl->layout == 0) {
                dst.m_src = fl->data;
                dst.m_f32 = fl->dtype == FOTO_F32;
                dst.m_rec = rec_in;
            }
        }
        for (int64_t r0 = 0; r0 < K; r0 += MAX_GRID_Y) {
            const dim3 grid(bx, (unsigned)std::min<int64_t>(K - r0, MAX_GRID_Y));
#define FOTO_MEDIAN_R(RR)                                                                                          \
    case RR:                                                                                                       \
        launch_round<RR>(grid, lds, s, src, g, dst, o, r0, w, h, tiles, tiles_x, (double*)fd->work.p,            \
                         (unsigned*)fd->ctl.p);                                                                    \
        break
            switch (o.radius) {
                FOTO_MEDIAN_R(1);
                FOTO_MEDIAN_R(2);
                FOTO_MEDIAN_R(3);
                FOTO_MEDIAN_R(4);
                FOTO_MEDIAN_R(5);
                FOTO_MEDIAN_R(6);
                FOTO_MEDIAN_R(7);
            }
#undef FOTO_MEDIAN_R
        }
    }
    FOTO_HIP_CHECK(hipGetLastError());
    return fd->link.leave(s, (hipStream_t)stream);
}

}  // extern "C"
