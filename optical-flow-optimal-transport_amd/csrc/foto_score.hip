// Scoring (include/foto.h, "scoring"): utils.EE / AE / IE (utils.py:294-354) with the robustness
// measures R(t), the accuracy percentiles A(p) and the normalised interpolation error NE of the
// Middlebury evaluation, on the flow and frame buffers the *_dev entries leave in HBM -- float32
// or float64, planar or .flo-interleaved, all records per launch (records ride on gridDim.y).
//
//   k_score_moments  one read of flow, ground truth and mask: counts, sums, threshold counts
//                    (grid_reduce_last of foto_reduce.h: fixed order, last-block hand-off), the
//                    maxima (one vector atomic max per block on the bit pattern, as k_flow_maxrad),
//                    the maps, and the kept errors as keys into the scratch (not kept: all ones).
//                    The last block of a record also sets up its select: k of every percentile.
//   k_score_dev2     the squared deviations around the means, which it reads from device memory.
//   k_score_hist / k_score_scan, once per digit from the top: an exact radix select on the keys.
//                    A non-negative double orders like its bit pattern; a pass counts one digit
//                    of the keys that share the prefix found so far (integer LDS atomics per
//                    block, then integer vector atomics to the global histogram), the scan picks
//                    the bin that holds rank k and extends the prefix.  Integer work throughout:
//                    the result does not depend on the order of execution.
//   k_score_finish   the only writer of the table.
//   k_frames_moments / k_frames_finish  IE, NE and max |d| of grey frames against one truth frame.
//
// The per-pixel arithmetic is k_err_partial's (foto_eval.hip), operation for operation, on values
// widened exactly to double; built with -ffp-contract=off like every other unit.  The keys cost 16
// bytes per pixel and record of grow-only scratch and save the deviations pass and every digit pass
// the three square roots, the division and the acos per pixel.  Every index is int64_t and
// every loop bounded by the sizes the host checked; the select walks at most `bins` bins.
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

constexpr unsigned long long KEY_NONE = ~0ULL;   // not kept (a NaN pattern no kept error has)
constexpr int SC_K = 13;      // sums of k_score_moments
constexpr int SC_REC = 16;    // doubles per record between the launches: SC_K sums, then 2 of k_score_dev2
constexpr int SC_PCT = 4;     // percentile slots per quantity
constexpr int SC_T = 2 * SC_PCT;
// SC_K sums: 0 n_valid, 1 n_EE, 2 sum EE, 3 n_AE, 4 sum AE, 5-8 #(EE > t), 9-12 #(AE > t)

struct FlowView {
    const void* data;
    int f32, inter;
    int64_t rec;   // elements per record (0: one record, read for every record)
};
struct ImgView {
    const void* data;
    int dtype;
    int64_t sy, sx;
    double divisor;
};
struct SelState {
    unsigned long long prefix;   // the digits found so far (key >> the bits not yet looked at)
    unsigned long long k;        // rank wanted among the keys that share the prefix, 1-based; 0: none
};

__device__ __forceinline__ void load_uv(const FlowView& f, int64_t r, int64_t n, int64_t p, double& u, double& v) {
    const int64_t iu = r * f.rec + (f.inter ? 2 * p : p), iv = f.inter ? iu + 1 : iu + n;
    if (f.f32) {
        u = (double)((const float*)f.data)[iu];
        v = (double)((const float*)f.data)[iv];
    } else {
        u = ((const double*)f.data)[iu];
        v = ((const double*)f.data)[iv];
    }
}

__device__ __forceinline__ double img_raw(const ImgView& im, int64_t off) {
    if (im.dtype == FOTO_U8) return (double)((const unsigned char*)im.data)[off];
    if (im.dtype == FOTO_F32) return (double)((const float*)im.data)[off];
    return ((const double*)im.data)[off];
}
// (double)pixel / divisor; x / 1.0 is x, bit for bit
__device__ __forceinline__ double img_val(const ImgView& im, int64_t off) {
    const double x = img_raw(im, off);
    return im.divisor == 1.0 ? x : x / im.divisor;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double y = __shfl_down(v, o, 64);
        if (y > v) v = y;
    }
    return v;
}

// the block's maxima of M non-negative values into mx[0..M): a tree, then one atomic max per value
template <int M>
__device__ __forceinline__ void block_atomic_max(double (&best)[M], unsigned long long* mx) {
    __shared__ double shm[M * (NT / 64)];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        best[m] = wave_max(best[m]);
        if (lane == 0) shm[m * (NT / 64) + wv] = best[m];
    }
    __syncthreads();
    if (threadIdx.x < M) {
        double b = shm[threadIdx.x * (NT / 64)];
#pragma unroll
        for (int j = 1; j < NT / 64; ++j) {
            const double y = shm[threadIdx.x * (NT / 64) + j];
            if (y > b) b = y;
        }
        if (b > 0.0) atomicMax(mx + threadIdx.x, (unsigned long long)__double_as_longlong(b));
    }
}

template <class To>
__device__ __forceinline__ void map_store(void* maps, int64_t i, double x) { ((To*)maps)[i] = (To)x; }

__global__ __launch_bounds__(NT) void k_score_moments(FlowView fl, FlowView gt, ImgView mask, int has_mask, int w,
                                                      int64_t n, foto_score_opts o, unsigned long long* keys,
                                                      void* maps, int maps_f32, double* partials, unsigned* tickets,
                                                      unsigned long long* mx, double* rec, SelState* st) {
    const int64_t r = blockIdx.y;
    double acc[SC_K];
#pragma unroll
    for (int k = 0; k < SC_K; ++k) acc[k] = 0.0;
    double best[2] = {0.0, 0.0};
    unsigned long long* kE = keys + (r * 2) * n;
    unsigned long long* kA = kE + n;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < n; p += (int64_t)gridDim.x * NT) {
        double u, v, uG, vG;
        load_uv(fl, r, n, p, u, v);
        load_uv(gt, r, n, p, uG, vG);
        bool valid = !flow_unknown(uG, vG);
        if (has_mask) {
            const int64_t row = p / w, col = p - row * w;
            valid = valid && img_raw(mask, row * mask.sy + col * mask.sx) != 0.0;
        }
        // k_err_partial's operations
        const double du = u - uG, dv = v - vG;
        const double e = sqrt(du * du + dv * dv);
        const double a = acos((1.0 + u * uG + v * vG) / (sqrt(1.0 + u * u + v * v) * sqrt(1.0 + uG * uG + vG * vG)));
        const bool keepE = valid && e <= o.ee_cap, keepA = valid && !(a != a);
        kE[p] = keepE ? (unsigned long long)__double_as_longlong(e) : KEY_NONE;
        kA[p] = keepA ? (unsigned long long)__double_as_longlong(a) : KEY_NONE;
        if (maps) {
            const int64_t i = (r * 2) * n + p;
            if (maps_f32) {
                map_store<float>(maps, i, valid ? e : qnan);
                map_store<float>(maps, i + n, valid ? a : qnan);
            } else {
                map_store<double>(maps, i, valid ? e : qnan);
                map_store<double>(maps, i + n, valid ? a : qnan);
            }
        }
        if (valid) acc[0] += 1.0;
        if (keepE) {
            acc[1] += 1.0;
            acc[2] += e;
            if (e > best[0]) best[0] = e;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < o.n_ee_thr && e > o.ee_thr[i]) acc[5 + i] += 1.0;
        }
        if (keepA) {
            acc[3] += 1.0;
            acc[4] += a;
            if (a > best[1]) best[1] = a;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < o.n_ae_thr && a > o.ae_thr[i]) acc[9 + i] += 1.0;
        }
    }
    block_atomic_max<2>(best, mx + r * 2);
    const RedBuf rb{partials + r * SC_K * gridDim.x, tickets + r, 0};
    double tot[SC_K];
    if (grid_reduce_last<SC_K>(acc, rb, tot) && threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < SC_K; ++k) rec[r * SC_REC + k] = tot[k];
        // the ranks of the select: k = max(1, ceil(p n / 100)) in float64, never above n
        for (int q = 0; q < 2; ++q) {
            const double nq = q == 0 ? tot[1] : tot[3];
            for (int j = 0; j < SC_PCT; ++j) {
                SelState s{0ULL, 0ULL};
                if (j < o.n_pct && nq > 0.0) {
                    double kk = ceil(o.pct[j] * nq / 100.0);
                    if (!(kk >= 1.0)) kk = 1.0;
                    if (kk > nq) kk = nq;
                    s.k = (unsigned long long)kk;
                }
                st[r * SC_T + q * SC_PCT + j] = s;
            }
        }
    }
}

// rec[13], rec[14] = sum (EE - mean)^2, sum (AE - mean)^2 over the kept errors
__global__ __launch_bounds__(NT) void k_score_dev2(int64_t n, const unsigned long long* __restrict__ keys,
                                                   double* partials, unsigned* tickets, double* rec) {
    const int64_t r = blockIdx.y;
    const double mee = rec[r * SC_REC + 2] / rec[r * SC_REC + 1], mae = rec[r * SC_REC + 4] / rec[r * SC_REC + 3];
    const unsigned long long* kE = keys + (r * 2) * n;
    const unsigned long long* kA = kE + n;
    double acc[2] = {0.0, 0.0};
    for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < n; p += (int64_t)gridDim.x * NT) {
        const unsigned long long be = kE[p], ba = kA[p];
        if (be != KEY_NONE) {
            const double e = __longlong_as_double((long long)be);
            acc[0] += (e - mee) * (e - mee);
        }
        if (ba != KEY_NONE) {
            const double a = __longlong_as_double((long long)ba);
            acc[1] += (a - mae) * (a - mae);
        }
    }
    const RedBuf rb{partials + r * 2 * gridDim.x, tickets + r, 0};
    double tot[2];
    if (grid_reduce_last<2>(acc, rb, tot) && threadIdx.x == 0) {
        rec[r * SC_REC + 13] = tot[0];
        rec[r * SC_REC + 14] = tot[1];
    }
}

// hist[r][t][digit] += the keys of target t's quantity whose bits above the digit equal its prefix.
// lh: 2 * npct * bins counters of dynamic LDS (the percentiles in use, both quantities).  Targets of
// one quantity that still share their prefix (all of them on the first pass) have the same
// histogram: the first of them counts, and the flush adds its counters to each one's global bins.
__global__ __launch_bounds__(NT) void k_score_hist(int64_t n, const unsigned long long* __restrict__ keys,
                                                   const SelState* __restrict__ st, unsigned* hist, int shift,
                                                   int bits, int npct) {
    extern __shared__ __attribute__((aligned(16))) unsigned lh[];
    __shared__ unsigned long long pre[SC_T];
    __shared__ int act[SC_T];
    __shared__ int rep[SC_T];   // the target that counts for this one (itself, or an earlier twin); -1: none
    const int64_t r = blockIdx.y;
    const int bins = 1 << bits;
    for (int i = threadIdx.x; i < 2 * npct * bins; i += NT) lh[i] = 0u;
    if (threadIdx.x < SC_T) {
        const SelState s = st[r * SC_T + threadIdx.x];
        pre[threadIdx.x] = s.prefix;
        act[threadIdx.x] = s.k != 0ULL;
    }
    __syncthreads();
    if (threadIdx.x < SC_T) {
        const int t = threadIdx.x, q0 = (t / SC_PCT) * SC_PCT;
        int rp = -1;
        if (act[t]) {
            rp = t;
            for (int j = t - 1; j >= q0; --j)
                if (act[j] && pre[j] == pre[t]) rp = j;
        }
        rep[t] = rp;
    }
    __syncthreads();
    const int hi = shift + bits;   // >= 64 on the first pass: no prefix yet
    const unsigned long long dmask = (unsigned long long)(bins - 1);
    for (int q = 0; q < 2; ++q) {
        bool any = false;
#pragma unroll
        for (int j = 0; j < SC_PCT; ++j) any = any || act[q * SC_PCT + j];
        if (!any) continue;
        const unsigned long long* kq = keys + (r * 2 + q) * n;
        for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < n; p += (int64_t)gridDim.x * NT) {
            const unsigned long long key = kq[p];
            if (key == KEY_NONE) continue;
            const int dig = (int)((key >> shift) & dmask);
            const unsigned long long top = hi >= 64 ? 0ULL : key >> hi;
#pragma unroll
            for (int j = 0; j < SC_PCT; ++j) {
                const int t = q * SC_PCT + j;
                if (j < npct && rep[t] == t && top == pre[t]) atomicAdd(&lh[(q * npct + j) * bins + dig], 1u);
            }
        }
    }
    __syncthreads();
    unsigned* gh = hist + r * SC_T * bins;
    for (int i = threadIdx.x; i < 2 * npct * bins; i += NT) {
        const int tl = i / bins, q = tl / npct, t = q * SC_PCT + (tl - q * npct), b = i - tl * bins;
        if (rep[t] < 0) continue;
        const unsigned c = lh[(q * npct + (rep[t] - q * SC_PCT)) * bins + b];
        if (c) atomicAdd(&gh[t * bins + b], c);
    }
}

// One block per (target, record): the bin that holds rank k, the prefix extended by it, k made
// relative to that bin; the target's bins go back to zero for the next pass.  Thread i owns `per`
// consecutive bins; an inclusive scan of the threads' sums finds the one thread whose bins hold
// rank k, and it walks them.
__global__ __launch_bounds__(NT) void k_score_scan(SelState* st, unsigned* hist, int bits) {
    __shared__ unsigned long long scan[2][NT];
    const int t = blockIdx.x;
    const int64_t r = blockIdx.y;
    const int bins = 1 << bits;
    const SelState s = st[r * SC_T + t];
    if (s.k == 0ULL) return;   // (block-uniform; its bins were never counted into)
    unsigned* gh = hist + (r * SC_T + t) * bins;
    constexpr int PER_MAX = (1 << 11) / NT;   // digit_bits() <= 11
    const int per = (bins + NT - 1) / NT;
    unsigned mine[PER_MAX];
    unsigned long long sum = 0ULL;
#pragma unroll
    for (int j = 0; j < PER_MAX; ++j) {
        const int b = threadIdx.x * per + j;
        mine[j] = 0u;
        if (j < per && b < bins) {
            mine[j] = gh[b];
            gh[b] = 0u;
        }
        sum += mine[j];
    }
    int cur = 0;
    scan[0][threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {   // Hillis-Steele, inclusive
        unsigned long long x = scan[cur][threadIdx.x];
        if ((int)threadIdx.x >= d) x += scan[cur][threadIdx.x - d];
        scan[cur ^ 1][threadIdx.x] = x;
        cur ^= 1;
        __syncthreads();
    }
    const unsigned long long incl = scan[cur][threadIdx.x];
    unsigned long long cum = incl - sum;   // the keys in the bins before this thread's
    if (cum < s.k && s.k <= incl) {
        int b = threadIdx.x * per;
#pragma unroll
        for (int j = 0; j < PER_MAX - 1; ++j)
            if (j < per - 1 && cum + mine[j] < s.k) {
                cum += mine[j];
                ++b;
            } else {
                break;
            }
        if (b > bins - 1) b = bins - 1;
        SelState o = s;
        o.k = s.k - cum;
        o.prefix = (s.prefix << bits) | (unsigned long long)b;
        st[r * SC_T + t] = o;
    }
}

__device__ __forceinline__ void finish_quantity(double* row, double n, double sum, double ss, unsigned long long mx,
                                                const double* cnt, int n_thr, const SelState* st, int n_pct) {
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const bool any = n > 0.0;
    row[0] = n;
    row[1] = any ? sum / n : qnan;
    row[2] = any ? sqrt(ss / n) : qnan;
    row[3] = any ? __longlong_as_double((long long)mx) : qnan;
    for (int i = 0; i < 4; ++i) row[4 + i] = any && i < n_thr ? cnt[i] / n : qnan;
    for (int j = 0; j < SC_PCT; ++j)
        row[8 + j] = any && j < n_pct ? __longlong_as_double((long long)st[j].prefix) : qnan;
}

__global__ __launch_bounds__(NT) void k_score_finish(int64_t R, foto_score_opts o, const double* __restrict__ rec,
                                                     const unsigned long long* __restrict__ mx,
                                                     const SelState* __restrict__ st, double* __restrict__ table) {
    const int64_t r = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (r >= R) return;
    const double* c = rec + r * SC_REC;
    double* row = table + r * FOTO_SCORE_COLS;
    row[0] = c[0];
    finish_quantity(row + 1, c[1], c[2], c[13], mx[r * 2], c + 5, o.n_ee_thr, st + r * SC_T, o.n_pct);
    finish_quantity(row + 13, c[3], c[4], c[14], mx[r * 2 + 1], c + 9, o.n_ae_thr, st + r * SC_T + SC_PCT, o.n_pct);
    for (int k = 25; k < FOTO_SCORE_COLS; ++k) row[k] = 0.0;
}

// ----------------------------------------------------------------------------- frames
// rec[r][0..2] = n, sum d^2, sum d^2 / (gx^2 + gy^2 + eps); mx[r] = max |d|; d = 255 I - 255 T
__global__ __launch_bounds__(NT) void k_frames_moments(ImgView fr, int64_t stride_rec, ImgView tr, ImgView mask,
                                                       int has_mask, int w, int h, double eps, double* partials,
                                                       unsigned* tickets, unsigned long long* mx, double* rec) {
    const int64_t r = blockIdx.y, n = (int64_t)w * h;
    double acc[3] = {0.0, 0.0, 0.0};
    double best[1] = {0.0};
    for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < n; p += (int64_t)gridDim.x * NT) {
        const int64_t row = p / w, col = p - row * w;
        if (has_mask && !(img_raw(mask, row * mask.sy + col * mask.sx) != 0.0)) continue;
        auto T = [&](int64_t y, int64_t x) { return 255 * img_val(tr, y * tr.sy + x * tr.sx); };
        const double d = 255 * img_val(fr, r * stride_rec + row * fr.sy + col * fr.sx) - T(row, col);
        // np.gradient: central in the interior (/ 2), one-sided at the border
        double gx = 0.0, gy = 0.0;
        if (w > 1) gx = col == 0 ? T(row, 1) - T(row, 0) : col == w - 1 ? T(row, col) - T(row, col - 1)
                                                                        : (T(row, col + 1) - T(row, col - 1)) / 2.0;
        if (h > 1) gy = row == 0 ? T(1, col) - T(0, col) : row == h - 1 ? T(row, col) - T(row - 1, col)
                                                                        : (T(row + 1, col) - T(row - 1, col)) / 2.0;
        const double d2 = d * d;
        acc[0] += 1.0;
        acc[1] += d2;
        acc[2] += d2 / (gx * gx + gy * gy + eps);
        if (fabs(d) > best[0]) best[0] = fabs(d);
    }
    block_atomic_max<1>(best, mx + r);
    const RedBuf rb{partials + r * 3 * gridDim.x, tickets + r, 0};
    double tot[3];
    if (grid_reduce_last<3>(acc, rb, tot) && threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) rec[r * 4 + k] = tot[k];
    }
}

__global__ __launch_bounds__(NT) void k_frames_finish(int64_t R, const double* __restrict__ rec,
                                                      const unsigned long long* __restrict__ mx,
                                                      double* __restrict__ table4) {
    const int64_t r = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (r >= R) return;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const double n = rec[r * 4];
    const bool any = n > 0.0;
    table4[r * 4] = n;
    table4[r * 4 + 1] = any ? sqrt(rec[r * 4 + 1] / n) : qnan;
    table4[r * 4 + 2] = any ? sqrt(rec[r * 4 + 2] / n) : qnan;
    table4[r * 4 + 3] = any ? __longlong_as_double((long long)mx[r]) : qnan;
}

// ----------------------------------------------------------------------------- host side

constexpr size_t HIST_LDS_MAX = 48 * 1024;   // of k_score_hist per block: three percentiles of 11-bit digits

// Blocks per record of the pixel passes: one per NT pixels up to about 2048 blocks per launch, the
// grid-stride loop takes the rest.  Every block ends with one returning atomic on its record's
// ticket, and one word takes about 88 of those per microsecond: with 1024 blocks per record the
// 31 x 1024 tickets of a 640 x 480 flow path cost 360 us per launch, whatever the kernel did
// (DESIGN.md 3.13).
int score_blocks(int64_t n, int64_t R) { return capped_blocks(n, (int)std::max<int64_t>(8, 2048 / R)); }

void opts_default(foto_score_opts* o) {
    memset(o, 0, sizeof(*o));
    o->ee_cap = 50.0;
    o->n_ee_thr = o->n_ae_thr = o->n_pct = 3;
    const double et[3] = {0.5, 1.0, 2.0}, ad[3] = {2.5, 5.0, 10.0}, pc[3] = {50.0, 75.0, 95.0};
    for (int i = 0; i < 3; ++i) {
        o->ee_thr[i] = et[i];
        o->ae_thr[i] = ad[i] * (M_PI / 180.0);   // np.deg2rad
        o->pct[i] = pc[i];
    }
}

int opts_check(const foto_score_opts* o, const char* who) {
    if (!o) return 0;
    if (!(o->ee_cap > 0.0)) { set_error("%s: ee_cap %g must be > 0 (or +inf)", who, o->ee_cap); return FOTO_ERR_ARG; }
    const int cnt[3] = {o->n_ee_thr, o->n_ae_thr, o->n_pct};
    static const char* const names[3] = {"n_ee_thr", "n_ae_thr", "n_pct"};
    for (int k = 0; k < 3; ++k)
        if (cnt[k] < 0 || cnt[k] > 4) { set_error("%s: %s = %d is outside 0..4", who, names[k], cnt[k]); return FOTO_ERR_ARG; }
    for (int i = 0; i < o->n_ee_thr; ++i)
        if (!std::isfinite(o->ee_thr[i]) || o->ee_thr[i] < 0.0) {
            set_error("%s: ee_thr[%d] = %g must be finite and >= 0", who, i, o->ee_thr[i]);
            return FOTO_ERR_ARG;
        }
    for (int i = 0; i < o->n_ae_thr; ++i)
        if (!std::isfinite(o->ae_thr[i]) || o->ae_thr[i] < 0.0) {
            set_error("%s: ae_thr[%d] = %g must be finite and >= 0", who, i, o->ae_thr[i]);
            return FOTO_ERR_ARG;
        }
    for (int j = 0; j < o->n_pct; ++j)
        if (!(o->pct[j] > 0.0) || !(o->pct[j] <= 100.0)) {
            set_error("%s: pct[%d] = %g is outside (0, 100]", who, j, o->pct[j]);
            return FOTO_ERR_ARG;
        }
    return 0;
}

int score_check(const foto_flow* fl, const foto_flow* gt, const foto_image* mask, int w, int h,
                const foto_score_opts* o, const char* who) {
    if (!fl || !gt) { set_error("%s: null flow descriptor", who); return FOTO_ERR_ARG; }
    FOTO_TRY(flow_check(fl, w, h, who));
    FOTO_TRY(flow_check(gt, w, h, who));
    FOTO_TRY(image_size_check(w, h, 1, who));
    if (fl->records > FOTO_SCORE_MAX_RECORDS) {
        set_error("%s: %d records; one call takes up to %d", who, fl->records, FOTO_SCORE_MAX_RECORDS);
        return FOTO_ERR_ARG;
    }
    if (gt->records != 1 && gt->records != fl->records) {
        set_error("%s: the ground truth has %d records: 1 (for every record) or the flow's %d", who, gt->records,
                  fl->records);
        return FOTO_ERR_ARG;
    }
    if (mask) FOTO_TRY(image_check(mask, w, h, who));
    return opts_check(o, who);
}

// table / maps of a flow score: non-null table, alignment, maps_dtype
int outputs_check(const double* table, const void* maps, int maps_dtype, const char* who) {
    if (!table) { set_error("%s: table is null", who); return FOTO_ERR_ARG; }
    if ((uintptr_t)table % sizeof(double) != 0) {
        set_error("%s: table %p is not aligned to 8 bytes", who, (const void*)table);
        return FOTO_ERR_ARG;
    }
    if (maps) {
        if (maps_dtype != FOTO_F32 && maps_dtype != FOTO_F64) {
            set_error("%s: maps_dtype %d is not FOTO_F32 / FOTO_F64", who, maps_dtype);
            return FOTO_ERR_ARG;
        }
        if ((uintptr_t)maps % dtype_bytes(maps_dtype) != 0) {
            set_error("%s: maps %p is not aligned to its %zu-byte element", who, maps, dtype_bytes(maps_dtype));
            return FOTO_ERR_ARG;
        }
    }
    return 0;
}

size_t image_span_bytes(const foto_image* im, int w, int h) {
    const size_t last = (size_t)(h - 1) * (size_t)im->stride_y + (size_t)(w - 1) * (size_t)im->stride_x;
    return (last + 1) * dtype_bytes(im->dtype);
}

// One stream, link and scratch set per device, kept for the process (RenderDev's scheme): the calls
// only enqueue, nothing waits on the host but a scratch that has to grow.
struct ScoreDev {
    hipStream_t s = nullptr;
    StreamLink link;
    DevScratch ctl;     // tickets, maxima, select states, histograms: zeroed per call
    DevScratch work;    // partials, per-record sums, keys
    DevScratch io[5];   // the host entry: flow, ground truth, mask, table, maps
};
std::mutex sd_mu;
std::vector<ScoreDev*> sd_dev;

int score_dev(int* device, ScoreDev** out) {
    int dev = 0;
    FOTO_HIP_CHECK(hipGetDevice(&dev));
    if ((int)sd_dev.size() <= dev) sd_dev.resize(dev + 1, nullptr);
    if (!sd_dev[dev]) {
        hipStream_t s = nullptr;
        FOTO_TRY(stream_acquire(&s));
        sd_dev[dev] = new ScoreDev();
        sd_dev[dev]->s = s;
    }
    *device = dev;
    *out = sd_dev[dev];
    return 0;
}

size_t up16(size_t b) { return (b + 15) / 16 * 16; }

// the digit width of the select: FOTO_SCORE_BITS (4..11), read at the entry of a call
int digit_bits() {
    const long long b = env_int("FOTO_SCORE_BITS", 8);
    return b < 4 ? 4 : b > 11 ? 11 : (int)b;
}

FlowView flow_view(const foto_flow* f, const void* data, int64_t n, bool broadcast) {
    return FlowView{data, f->dtype == FOTO_F32, f->layout == 1, broadcast ? 0 : (f->layout == 0 ? 3 : 2) * n};
}
ImgView img_view(const foto_image* im, const void* data) {
    if (!im) return ImgView{nullptr, FOTO_U8, 0, 0, 1.0};
    return ImgView{data, im->dtype, im->stride_y, im->stride_x, im->divisor};
}

// every launch of a flow score on sd->s; all pointers are device memory
int score_enqueue(ScoreDev* sd, const foto_flow* fl, const void* fl_data, const foto_flow* gt, const void* gt_data,
                  const foto_image* mask, const void* mask_data, int w, int h, const foto_score_opts& o, double* table,
                  void* maps, int maps_dtype, int bits) {
    hipStream_t s = sd->s;
    while (bits > 4 && ((size_t)2 * o.n_pct << bits) * sizeof(unsigned) > HIST_LDS_MAX) --bits;
    const int64_t n = (int64_t)w * h, R = fl->records;
    const int bins = 1 << bits;
    const unsigned bx = (unsigned)score_blocks(n, R);
    // ctl: tickets | maxima | states | histograms
    const size_t o_mx = up16((size_t)R * sizeof(unsigned)), o_st = o_mx + up16((size_t)R * 2 * 8);
    const size_t o_hist = o_st + (size_t)R * SC_T * sizeof(SelState);
    const size_t ctl_bytes = o_hist + up16((size_t)R * SC_T * bins * sizeof(unsigned));
    // work: partials | per-record sums | keys
    const size_t o_rec = (size_t)R * SC_K * bx * 8, o_keys = o_rec + (size_t)R * SC_REC * 8;
    const size_t work_bytes = o_keys + (size_t)R * 2 * (size_t)n * 8;
    FOTO_TRY(sd->ctl.reserve(ctl_bytes, s));
    FOTO_TRY(sd->work.reserve(work_bytes, s));
    char* ctl = (char*)sd->ctl.p;
    char* work = (char*)sd->work.p;
    unsigned* tickets = (unsigned*)ctl;
    unsigned long long* mx = (unsigned long long*)(ctl + o_mx);
    SelState* st = (SelState*)(ctl + o_st);
    unsigned* hist = (unsigned*)(ctl + o_hist);
    double* partials = (double*)work;
    double* rec = (double*)(work + o_rec);
    unsigned long long* keys = (unsigned long long*)(work + o_keys);

    FOTO_HIP_CHECK(hipMemsetAsync(ctl, 0, ctl_bytes, s));
    const FlowView fv = flow_view(fl, fl_data, n, false), gv = flow_view(gt, gt_data, n, gt->records == 1 && R > 1);
    k_score_moments<<<dim3(bx, (unsigned)R), NT, 0, s>>>(fv, gv, img_view(mask, mask_data), mask ? 1 : 0, w, n, o, keys,
                                                         maps, maps_dtype == FOTO_F32, partials, tickets, mx, rec, st);
    k_score_dev2<<<dim3(bx, (unsigned)R), NT, 0, s>>>(n, keys, partials, tickets, rec);
    if (o.n_pct > 0) {
        const int passes = (64 + bits - 1) / bits;
        for (int p = passes - 1; p >= 0; --p) {
            k_score_hist<<<dim3(bx, (unsigned)R), NT, (size_t)2 * o.n_pct * bins * sizeof(unsigned), s>>>(
                n, keys, st, hist, p * bits, bits, o.n_pct);
            k_score_scan<<<dim3(SC_T, (unsigned)R), NT, 0, s>>>(st, hist, bits);
        }
    }
    k_score_finish<<<(unsigned)((R + NT - 1) / NT), NT, 0, s>>>(R, o, rec, mx, st, table);
    FOTO_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace
}  // namespace foto

using namespace foto;

extern "C" {

int foto_score_opts_default(foto_score_opts* o) {
    if (!o) { set_error("foto_score_opts_default: null pointer"); return FOTO_ERR_ARG; }
    opts_default(o);
    return 0;
}

int foto_score_check(const foto_flow* fl, const foto_flow* gt, const foto_image* mask_or_null, int w, int h,
                     const foto_score_opts* opts_or_null) {
    return score_check(fl, gt, mask_or_null, w, h, opts_or_null, "foto_score_check");
}

int foto_score_flow_dev(const foto_flow* fl, const foto_flow* gt, const foto_image* mask, int w, int h,
                        const foto_score_opts* opts_or_null, double* table, void* maps, int maps_dtype, void* stream) {
    static const char* const who = "foto_score_flow_dev";
    // ---- host-only checks, before any device call
    FOTO_TRY(score_check(fl, gt, mask, w, h, opts_or_null, who));
    FOTO_TRY(outputs_check(table, maps, maps_dtype, who));
    foto_score_opts o;
    if (opts_or_null) o = *opts_or_null;
    else opts_default(&o);
    const int bits = digit_bits();
    // ---- the pointer queries, before anything is enqueued
    std::lock_guard<std::mutex> lk(sd_mu);
    int device = 0;
    ScoreDev* sd = nullptr;
    FOTO_TRY(score_dev(&device, &sd));
    const size_t fl_b = flow_bytes(fl, w, h), gt_b = flow_bytes(gt, w, h);
    const size_t tb_b = (size_t)fl->records * FOTO_SCORE_COLS * sizeof(double);
    const size_t mp_b = maps ? (size_t)fl->records * 2 * (size_t)w * (size_t)h * dtype_bytes(maps_dtype) : 0;
    const size_t mk_b = mask ? image_span_bytes(mask, w, h) : 0;
    FOTO_TRY(dev_ptr_check(fl->data, fl_b, device, who, "flow data"));
    FOTO_TRY(dev_ptr_check(gt->data, gt_b, device, who, "ground-truth data"));
    if (mask) FOTO_TRY(image_dev_check(mask, w, h, device, who));
    FOTO_TRY(dev_ptr_check(table, tb_b, device, who, "table"));
    if (maps) FOTO_TRY(dev_ptr_check(maps, mp_b, device, who, "maps"));
    const void* in[3] = {fl->data, gt->data, mask ? mask->data : nullptr};
    const size_t in_b[3] = {fl_b, gt_b, mk_b};
    for (int k = 0; k < 3; ++k)
        if (in[k] && (overlaps(table, tb_b, in[k], in_b[k]) || (maps && overlaps(maps, mp_b, in[k], in_b[k])))) {
            set_error("%s: table and maps may not overlap the flow, the ground truth or the mask", who);
            return FOTO_ERR_ARG;
        }
    if (maps && overlaps(table, tb_b, maps, mp_b)) {
        set_error("%s: table and maps may not overlap each other", who);
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(sd->link.enter((hipStream_t)stream, sd->s));
    FOTO_TRY(score_enqueue(sd, fl, fl->data, gt, gt->data, mask, mask ? mask->data : nullptr, w, h, o, table, maps,
                           maps_dtype, bits));
    return sd->link.leave(sd->s, (hipStream_t)stream);
}

int foto_score_flow(const foto_flow* fl, const foto_flow* gt, const foto_image* mask, int w, int h,
                    const foto_score_opts* opts_or_null, double* table, void* maps, int maps_dtype) {
    static const char* const who = "foto_score_flow";
    FOTO_TRY(score_check(fl, gt, mask, w, h, opts_or_null, who));
    FOTO_TRY(outputs_check(table, maps, maps_dtype, who));
    foto_score_opts o;
    if (opts_or_null) o = *opts_or_null;
    else opts_default(&o);
    const int bits = digit_bits();
    std::lock_guard<std::mutex> lk(sd_mu);
    int device = 0;
    ScoreDev* sd = nullptr;
    FOTO_TRY(score_dev(&device, &sd));
    hipStream_t s = sd->s;
    const size_t fl_b = flow_bytes(fl, w, h), gt_b = flow_bytes(gt, w, h);
    const size_t tb_b = (size_t)fl->records * FOTO_SCORE_COLS * sizeof(double);
    const size_t mp_b = maps ? (size_t)fl->records * 2 * (size_t)w * (size_t)h * dtype_bytes(maps_dtype) : 0;
    const size_t mk_b = mask ? image_span_bytes(mask, w, h) : 0;
    const void* src[3] = {fl->data, gt->data, mask ? mask->data : nullptr};
    const size_t by[5] = {fl_b, gt_b, mk_b, tb_b, mp_b};
    for (int k = 0; k < 5; ++k)
        if (by[k]) FOTO_TRY(sd->io[k].reserve(by[k], s));
    for (int k = 0; k < 3; ++k)
        if (by[k]) FOTO_HIP_CHECK(hipMemcpyAsync(sd->io[k].p, src[k], by[k], hipMemcpyHostToDevice, s));
    FOTO_TRY(score_enqueue(sd, fl, sd->io[0].p, gt, sd->io[1].p, mask, mask ? sd->io[2].p : nullptr, w, h, o,
                           (double*)sd->io[3].p, maps ? sd->io[4].p : nullptr, maps_dtype, bits));
    FOTO_HIP_CHECK(hipMemcpyAsync(table, sd->io[3].p, tb_b, hipMemcpyDeviceToHost, s));
    if (maps) FOTO_HIP_CHECK(hipMemcpyAsync(maps, sd->io[4].p, mp_b, hipMemcpyDeviceToHost, s));
    FOTO_HIP_CHECK(hipStreamSynchronize(s));   // the one wait
    return 0;
}

int foto_score_frames_dev(const foto_image* frames, int count, int64_t stride_rec, const foto_image* truth,
                          const foto_image* mask, int w, int h, double ne_eps, double* table4, void* stream) {
    static const char* const who = "foto_score_frames_dev";
    if (!frames || !truth || !table4) { set_error("%s: null pointer", who); return FOTO_ERR_ARG; }
    if (count < 1 || count > FOTO_SCORE_MAX_RECORDS) {
        set_error("%s: count = %d is outside 1..%d", who, count, FOTO_SCORE_MAX_RECORDS);
        return FOTO_ERR_ARG;
    }
    if (stride_rec <= 0) {
        set_error("%s: stride_rec = %lld must be > 0 (in elements)", who, (long long)stride_rec);
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(image_size_check(w, h, 1, who));
    FOTO_TRY(image_check(frames, w, h, who));
    FOTO_TRY(image_check(truth, w, h, who));
    if (mask) FOTO_TRY(image_check(mask, w, h, who));
    if (!std::isfinite(ne_eps) || ne_eps < 0.0) {
        set_error("%s: ne_eps %g must be finite and >= 0", who, ne_eps);
        return FOTO_ERR_ARG;
    }
    if ((uintptr_t)table4 % sizeof(double) != 0) {
        set_error("%s: table %p is not aligned to 8 bytes", who, (const void*)table4);
        return FOTO_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(sd_mu);
    int device = 0;
    ScoreDev* sd = nullptr;
    FOTO_TRY(score_dev(&device, &sd));
    const size_t fr_b = image_span_bytes(frames, w, h) +
                        (size_t)(count - 1) * (size_t)stride_rec * dtype_bytes(frames->dtype);
    const size_t tr_b = image_span_bytes(truth, w, h), mk_b = mask ? image_span_bytes(mask, w, h) : 0;
    const size_t tb_b = (size_t)count * 4 * sizeof(double);
    FOTO_TRY(dev_ptr_check(frames->data, fr_b, device, who, "frames (all records)"));
    FOTO_TRY(image_dev_check(truth, w, h, device, who));
    if (mask) FOTO_TRY(image_dev_check(mask, w, h, device, who));
    FOTO_TRY(dev_ptr_check(table4, tb_b, device, who, "table"));
    if (overlaps(table4, tb_b, frames->data, fr_b) || overlaps(table4, tb_b, truth->data, tr_b) ||
        (mask && overlaps(table4, tb_b, mask->data, mk_b))) {
        set_error("%s: table may not overlap the frames, the truth or the mask", who);
        return FOTO_ERR_ARG;
    }
    hipStream_t s = sd->s;
    const int64_t n = (int64_t)w * h, R = count;
    const unsigned bx = (unsigned)score_blocks(n, R);
    const size_t o_mx = up16((size_t)R * sizeof(unsigned)), ctl_bytes = o_mx + up16((size_t)R * 8);
    const size_t o_rec = (size_t)R * 3 * bx * 8, work_bytes = o_rec + (size_t)R * 4 * 8;
    FOTO_TRY(sd->ctl.reserve(ctl_bytes, s));
    FOTO_TRY(sd->work.reserve(work_bytes, s));
    unsigned* tickets = (unsigned*)sd->ctl.p;
    unsigned long long* mx = (unsigned long long*)((char*)sd->ctl.p + o_mx);
    double* partials = (double*)sd->work.p;
    double* rec = (double*)((char*)sd->work.p + o_rec);
    FOTO_TRY(sd->link.enter((hipStream_t)stream, s));
    FOTO_HIP_CHECK(hipMemsetAsync(sd->ctl.p, 0, ctl_bytes, s));
    k_frames_moments<<<dim3(bx, (unsigned)R), NT, 0, s>>>(img_view(frames, frames->data), stride_rec,
                                                          img_view(truth, truth->data),
                                                          img_view(mask, mask ? mask->data : nullptr), mask ? 1 : 0, w,
                                                          h, ne_eps, partials, tickets, mx, rec);
    k_frames_finish<<<(unsigned)((R + NT - 1) / NT), NT, 0, s>>>(R, rec, mx, table4);
    FOTO_HIP_CHECK(hipGetLastError());
    return sd->link.leave(s, (hipStream_t)stream);
}

}  // extern "C"

static_assert(sizeof(foto_score_opts) == 120, "foto_score_opts layout");
