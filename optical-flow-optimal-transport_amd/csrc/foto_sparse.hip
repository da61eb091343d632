// libfoto: sparse tracking on gfx950 -- Shi-Tomasi corners (Shi & Tomasi 1994), pyramidal
// Lucas-Kanade with fixed counts (Lucas & Kanade 1981; Bouguet 2001), and a dense flow sampled at
// points.  include/foto.h has the arithmetic; tests/sparse_ref.py restates it in numpy and the
// device is held to it bit for bit (-ffp-contract=off, every sum in one fixed order).
//
// Corners, all float64:
//   launch_ingest            the frame widened to [h][w]
//   k_corner_response        one LDS tile: Gx Gx, Gx Gy, Gy Gy on the haloed tile (cdiff_x / cdiff_y,
//                            TV-L1's gradients), the horizontal then the vertical box sums, R, and the
//                            frame maximum (order-free: a tree, then one integer atomic max per block
//                            on the bit pattern of the positive double)
//   k_corner_mark            the candidate rules per pixel; a count per block of CM_PIX pixels
//   k_corner_scan            one block: the exclusive scan of the block counts
//   k_corner_gather          the candidates in raster order: index and key (R's bits)
//   k_corner_rank            rank = #{stronger, or as strong and earlier}: exact, by counting.  Two
//                            candidates are more than s pixels apart (the tie rule), so there are at
//                            most ceil(w / (s + 1)) ceil(h / (s + 1)) of them and the count is cheap
//   k_corner_emit            the survivors in raster order, NaN beyond the count, the count
// No float atomics and no host wait (but for a scratch that has to grow, or a host count).
//
// Lucas-Kanade: one wavefront per point, four per block.  A lane holds its <= 4 window elements'
// T, Gx, Gy in registers for the level; every sum is lane-serial, then wave_sum's tree
// (foto_reduce.h), broadcast with dbl_readlane, so every lane carries the same d.  The gradients
// are formed at the taps (no gradient planes: the template is sampled once per level, the
// iterations read the search frame alone).  No LDS, no atomics, no data-dependent loop count.
#include <cmath>
#include <memory>
#include <mutex>
#include <vector>

#include "foto_devmem.h"
#include "foto_devutil.h"
#include "foto_gn.h"
#include "foto_reduce.h"

namespace foto {
namespace {

// ----------------------------------------------------------------------------- corner kernels

constexpr int CT_W = 32, CT_H = 16;                  // the response tile: two pixels per thread
constexpr int CW_MAX = FOTO_CORNER_MAX_WINDOW;       // the largest box radius c
constexpr int CP_W = CT_W + 2 * CW_MAX, CP_H = CT_H + 2 * CW_MAX;   // the haloed tile
static_assert(CT_W * CT_H == 2 * NT, "two response pixels per thread");
constexpr int CM_PER = 4, CM_PIX = CM_PER * NT;      // pixels per thread / block of mark and gather

__device__ __forceinline__ double wave_max_pos(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double y = __shfl_down(v, o, 64);
        if (y > v) v = y;
    }
    return v;
}

// R of every pixel and the maximum of the finite positive R into rmax (the bits of a double, 0
// before the launch).  The products outside the frame are +0.0; both sums start from their first
// term and run in increasing offset.
__global__ __launch_bounds__(NT) void k_corner_response(int w, int h, int c, int tiles_x, const double* __restrict__ f,
                                                        double* __restrict__ resp, unsigned long long* rmax) {
    __shared__ double sP[3][CP_H * CP_W];
    __shared__ double sH[3][CP_H * CT_W];
    __shared__ double smax[NT / 64];
    const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)blockIdx.x - ty * tiles_x;
    const int ox = tx * CT_W, oy = ty * CT_H;
    const int pw = CT_W + 2 * c, ph = CT_H + 2 * c;
    for (int l = threadIdx.x; l < pw * ph; l += NT) {
        const int ly = l / pw, lx = l - ly * pw;
        const int gx = ox - c + lx, gy = oy - c + ly;
        double a = 0.0, b = 0.0, d = 0.0;
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
            const double Gx = cdiff_x(f, w, gx, (int64_t)gy * w), Gy = cdiff_y(f, w, h, gx, gy);
            a = Gx * Gx;
            b = Gx * Gy;
            d = Gy * Gy;
        }
        sP[0][ly * CP_W + lx] = a;
        sP[1][ly * CP_W + lx] = b;
        sP[2][ly * CP_W + lx] = d;
    }
    __syncthreads();
    for (int l = threadIdx.x; l < CT_W * ph; l += NT) {
        const int ly = l / CT_W, lx = l - ly * CT_W;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const double* row = &sP[p][ly * CP_W + lx];
            double s = row[0];
            for (int dx = 1; dx <= 2 * c; ++dx) s += row[dx];
            sH[p][ly * CT_W + lx] = s;
        }
    }
    __syncthreads();
    double best = 0.0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int l = threadIdx.x + q * NT;
        const int ly = l / CT_W, lx = l - ly * CT_W;
        double t[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const double* col = &sH[p][ly * CT_W + lx];
            double s = col[0];
            for (int dy = 1; dy <= 2 * c; ++dy) s += col[dy * CT_W];
            t[p] = s;
        }
        const double a = t[0], b = t[1], cc = t[2];
        const double R = 0.5 * ((a + cc) - sqrt((a - cc) * (a - cc) + 4.0 * (b * b)));
        const int gx = ox + lx, gy = oy + ly;
        if (gx < w && gy < h) {
            resp[(int64_t)gy * w + gx] = R;
            if (R > best && R < INFINITY) best = R;
        }
    }
    best = wave_max_pos(best);
    if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int j = 1; j < NT / 64; ++j)
            if (smax[j] > best) best = smax[j];
        if (best > 0.0) atomicMax(rmax, (unsigned long long)__double_as_longlong(best));
    }
}

struct CornerPar {
    int w, h, s, margin;
    double quality;
};

// the candidate rules of include/foto.h at pixel i; a NaN anywhere in the neighbourhood fails them
__device__ __forceinline__ bool corner_candidate(const CornerPar& P, const double* __restrict__ resp, double thr,
                                                 int64_t i) {
    const double R = resp[i];
    if (!(R > 0.0 && R < INFINITY) || !(R >= thr)) return false;
    const int y = (int)((unsigned)i / (unsigned)P.w), x = (int)i - y * P.w;
    if (x < P.margin || x >= P.w - P.margin || y < P.margin || y >= P.h - P.margin) return false;
    const int x0 = max(x - P.s, 0), x1 = min(x + P.s, P.w - 1), y0 = max(y - P.s, 0), y1 = min(y + P.s, P.h - 1);
    bool ok = true;
    for (int yy = y0; yy <= y1 && ok; ++yy) {
        const double* row = resp + (int64_t)yy * P.w;
        for (int xx = x0; xx <= x1; ++xx) {
            const double Q = row[xx];
            const bool earlier = yy < y || (yy == y && xx < x);
            const bool self = yy == y && xx == x;
            ok = ok && (self || (earlier ? R > Q : R >= Q));
        }
    }
    return ok;
}

// the exclusive prefix of v over the block's threads and the block's total; sh: NT / 64 ints
__device__ __forceinline__ int block_excl_scan(int v, int* sh, int& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(x, o, 64);
        if (lane >= o) x += t;
    }
    if (lane == 63) sh[wv] = x;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int j = 0; j < NT / 64; ++j) {
        if (j < wv) base += sh[j];
        total += sh[j];
    }
    __syncthreads();   // (sh may be written again by the caller's next round)
    return base + x - v;
}

__global__ __launch_bounds__(NT) void k_corner_mark(CornerPar P, const double* __restrict__ resp,
                                                    const unsigned long long* __restrict__ rmax,
                                                    unsigned char* __restrict__ flag, int* __restrict__ blockcnt) {
    __shared__ int sh[NT / 64];
    const int64_t n = (int64_t)P.w * P.h;
    const double thr = P.quality * __longlong_as_double((long long)rmax[0]);
    const int64_t base = (int64_t)blockIdx.x * CM_PIX + (int64_t)threadIdx.x * CM_PER;
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < CM_PER; ++q) {
        const int64_t i = base + q;
        if (i >= n) break;
        const bool c = corner_candidate(P, resp, thr, i);
        flag[i] = c ? 1 : 0;
        cnt += c ? 1 : 0;
    }
    int total;
    (void)block_excl_scan(cnt, sh, total);
    if (threadIdx.x == 0) blockcnt[blockIdx.x] = total;
}

// one block: off[b] = the candidates before block b; ccount[0] = all of them
__global__ __launch_bounds__(NT) void k_corner_scan(int nb, const int* __restrict__ blockcnt, int* __restrict__ off,
                                                    int* __restrict__ ccount) {
    __shared__ int sh[NT / 64];
    int running = 0;
    for (int base = 0; base < nb; base += NT) {
        const int b = base + threadIdx.x;
        const int v = b < nb ? blockcnt[b] : 0;
        int total;
        const int e = block_excl_scan(v, sh, total);
        if (b < nb) off[b] = running + e;
        running += total;
    }
    if (threadIdx.x == 0) ccount[0] = running;
}

// cap: the candidate lists' capacity (the bound of the tie rule; never exceeded, and checked)
__global__ __launch_bounds__(NT) void k_corner_gather(int64_t n, const double* __restrict__ resp,
                                                      const unsigned char* __restrict__ flag,
                                                      const int* __restrict__ off, int cap, int* __restrict__ cidx,
                                                      unsigned long long* __restrict__ ckey) {
    __shared__ int sh[NT / 64];
    const int64_t base = (int64_t)blockIdx.x * CM_PIX + (int64_t)threadIdx.x * CM_PER;
    bool c[CM_PER];
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < CM_PER; ++q) {
        c[q] = base + q < n && flag[base + q] != 0;
        cnt += c[q] ? 1 : 0;
    }
    int total;
    int pos = off[blockIdx.x] + block_excl_scan(cnt, sh, total);
#pragma unroll
    for (int q = 0; q < CM_PER; ++q) {
        if (!c[q]) continue;
        if (pos < cap) {
            cidx[pos] = (int)(base + q);
            ckey[pos] = (unsigned long long)__double_as_longlong(resp[base + q]);
        }
        ++pos;
    }
}

// keep[i] = fewer than max_count candidates are stronger, or as strong and earlier (R > 0: the
// bit patterns order as the values; the list is in raster order)
__global__ __launch_bounds__(NT) void k_corner_rank(const int* __restrict__ ccount, int cap,
                                                    const unsigned long long* __restrict__ ckey, int max_count,
                                                    unsigned char* __restrict__ keep) {
    __shared__ unsigned long long sk[NT];
    const int C = min(ccount[0], cap);
    if ((int)(blockIdx.x * NT) >= C) return;
    const int i = blockIdx.x * NT + threadIdx.x;
    const unsigned long long ki = i < C ? ckey[i] : 0ULL;
    int rank = 0;
    for (int base = 0; base < C; base += NT) {
        sk[threadIdx.x] = base + (int)threadIdx.x < C ? ckey[base + threadIdx.x] : 0ULL;
        __syncthreads();
        const int m = min(NT, C - base);
        for (int j = 0; j < m; ++j) {
            const unsigned long long kj = sk[j];
            rank += (kj > ki || (kj == ki && base + j < i)) ? 1 : 0;
        }
        __syncthreads();
    }
    if (i < C) keep[i] = rank < max_count ? 1 : 0;
}

// the kept candidates in raster order as (x, y) rows, NaN rows from the count on, the count
template <class TO>
__global__ __launch_bounds__(NT) void k_corner_emit(int w, const int* __restrict__ ccount, int cap,
                                                    const int* __restrict__ cidx,
                                                    const unsigned char* __restrict__ keep, int max_count,
                                                    TO* __restrict__ pts, int* __restrict__ count) {
    __shared__ unsigned char sk[NT];
    const int C = min(ccount[0], cap);
    const int cnt = min(C, max_count);
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i == 0) count[0] = cnt;
    if (i >= cnt && i < max_count) {
        pts[2 * (int64_t)i] = (TO)NAN;
        pts[2 * (int64_t)i + 1] = (TO)NAN;
    }
    if ((int)(blockIdx.x * NT) >= C) return;
    int pos = i;
    if (C > max_count) {   // the kept candidates before this one
        pos = 0;
        const int last = min((int)(blockIdx.x * NT) + NT, C);
        for (int base = 0; base < last; base += NT) {
            sk[threadIdx.x] = base + (int)threadIdx.x < C ? keep[base + threadIdx.x] : 0;
            __syncthreads();
            const int m = min(NT, i - base);
            for (int j = 0; j < m; ++j) pos += sk[j];
            __syncthreads();
        }
    }
    if (i < C && keep[i] && pos < max_count) {
        const int p = cidx[i];
        const int y = (int)((unsigned)p / (unsigned)w), x = p - y * w;
        pts[2 * (int64_t)pos] = (TO)x;
        pts[2 * (int64_t)pos + 1] = (TO)y;
    }
}

// ----------------------------------------------------------------------------- Lucas-Kanade kernel

struct LkLevels {
    int L;
    int w[FOTO_GN_PYR_MAX_LEVELS], h[FOTO_GN_PYR_MAX_LEVELS];
    const double* a[FOTO_GN_PYR_MAX_LEVELS];   // the template frame's levels
    const double* b[FOTO_GN_PYR_MAX_LEVELS];   // the search frame's levels
};
struct LkPar {
    int radius, iters;
    double min_eig, fb_tol;
};
constexpr int LK_PER = 4;   // window elements per lane: (2 * 7 + 1)^2 = 225 <= 4 * 64
static_assert((2 * FOTO_LK_MAX_RADIUS + 1) * (2 * FOTO_LK_MAX_RADIUS + 1) <= LK_PER * 64, "the window and the wave");

// The window sum of include/foto.h: the lane's four slots (0.0 where the element is past n) added
// in order, the 64 partials through wave_sum's tree, lane 0's total to every lane.
__device__ __forceinline__ double lk_sum(const double (&v)[LK_PER]) {
    const double s = ((v[0] + v[1]) + v[2]) + v[3];
    return dbl_readlane(wave_sum(s), 0);
}

template <class TP, class TO>
__global__ __launch_bounds__(NT) void k_lk_track(LkLevels lv, LkPar par, const TP* __restrict__ pts,
                                                 const TO* __restrict__ prior, int64_t M, TO* __restrict__ out,
                                                 unsigned char* status, double* __restrict__ err,
                                                 double* __restrict__ fb) {
    const int lane = threadIdx.x & 63;
    const int64_t pt = (int64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (pt >= M) return;   // (a whole wave)
    double x0 = (double)pts[2 * pt], y0 = (double)pts[2 * pt + 1];
    double px = 0.0, py = 0.0;
    if (prior) {
        px = (double)prior[2 * pt];
        py = (double)prior[2 * pt + 1];
        x0 = x0 + px;
        y0 = y0 + py;
    }
    const int R = par.radius, side = 2 * R + 1, n = side * side;
    bool on[LK_PER];
    double ax[LK_PER], ay[LK_PER];
#pragma unroll
    for (int q = 0; q < LK_PER; ++q) {
        const int e = lane + 64 * q;
        on[q] = e < n;
        const int ee = on[q] ? e : 0, r = ee / side;
        ay[q] = (double)(r - R);
        ax[q] = (double)(ee - r * side - R);
    }
    const bool fin = isfinite(x0) && isfinite(y0);
    double dx = 0.0, dy = 0.0, errv = NAN;
    unsigned st = 0;
    if (fin) {   // (the same in every lane of the wave, like every branch below)
        for (int l = lv.L - 1; l >= 0; --l) {
            double x = x0, y = y0;
            for (int k = 0; k < l; ++k) {
                x = (x + 0.5) * ((double)lv.w[k + 1] / (double)lv.w[k]) - 0.5;
                y = (y + 0.5) * ((double)lv.h[k + 1] / (double)lv.h[k]) - 0.5;
            }
            if (l < lv.L - 1) {
                dx = dx * ((double)lv.w[l] / (double)lv.w[l + 1]);
                dy = dy * ((double)lv.h[l] / (double)lv.h[l + 1]);
            }
            const int w = lv.w[l], h = lv.h[l];
            const double* __restrict__ fa = lv.a[l];
            const double* __restrict__ fb_ = lv.b[l];
            double T[LK_PER], Gx[LK_PER], Gy[LK_PER], v[LK_PER];
#pragma unroll
            for (int q = 0; q < LK_PER; ++q) {
                T[q] = Gx[q] = Gy[q] = 0.0;
                if (!on[q]) continue;
                const SampleTaps S = sample_taps(w, h, x + ax[q], y + ay[q]);
                const int i0 = S.i0, j0 = S.j0;
                const int64_t r0 = (int64_t)j0 * w, r1 = r0 + w;
                T[q] = sample_sum(S, fa[r0 + i0], fa[r0 + i0 + 1], fa[r1 + i0], fa[r1 + i0 + 1]);
                Gx[q] = sample_sum(S, cdiff_x(fa, w, i0, r0), cdiff_x(fa, w, i0 + 1, r0), cdiff_x(fa, w, i0, r1),
                                   cdiff_x(fa, w, i0 + 1, r1));
                Gy[q] = sample_sum(S, cdiff_y(fa, w, h, i0, j0), cdiff_y(fa, w, h, i0 + 1, j0),
                                   cdiff_y(fa, w, h, i0, j0 + 1), cdiff_y(fa, w, h, i0 + 1, j0 + 1));
            }
#pragma unroll
            for (int q = 0; q < LK_PER; ++q) v[q] = Gx[q] * Gx[q];
            const double gxx = lk_sum(v);
#pragma unroll
            for (int q = 0; q < LK_PER; ++q) v[q] = Gx[q] * Gy[q];
            const double gxy = lk_sum(v);
#pragma unroll
            for (int q = 0; q < LK_PER; ++q) v[q] = Gy[q] * Gy[q];
            const double gyy = lk_sum(v);
            const double det = gxx * gyy - gxy * gxy;
            const double mineig =
                0.5 * ((gxx + gyy) - sqrt((gxx - gyy) * (gxx - gyy) + 4.0 * (gxy * gxy))) / (double)n;
            const bool textured = mineig > par.min_eig;
            if (!textured && l == 0) st |= FOTO_LK_FLAT;
            // `iters` steps on a textured level; at level 0 one more residual pass for err
            const int passes = (textured ? par.iters : 0) + (l == 0 ? 1 : 0);
            for (int it = 0; it < passes; ++it) {
                double r[LK_PER];
#pragma unroll
                for (int q = 0; q < LK_PER; ++q)
                    r[q] = on[q] ? T[q] - pyr_sample(fb_, w, h, (x + dx) + ax[q], (y + dy) + ay[q]) : 0.0;
                if (it == passes - 1 && l == 0) {
#pragma unroll
                    for (int q = 0; q < LK_PER; ++q) v[q] = fabs(r[q]);
                    errv = lk_sum(v) / (double)n;
                    break;
                }
#pragma unroll
                for (int q = 0; q < LK_PER; ++q) v[q] = r[q] * Gx[q];
                const double bx = lk_sum(v);
#pragma unroll
                for (int q = 0; q < LK_PER; ++q) v[q] = r[q] * Gy[q];
                const double by = lk_sum(v);
                dx += (gyy * bx - gxy * by) / det;
                dy += (gxx * by - gxy * bx) / det;
            }
        }
    }
    if (!fin || !isfinite(dx) || !isfinite(dy)) {
        dx = dy = errv = NAN;
        st |= FOTO_LK_NONFINITE;
    }
    const double xe = x0 + dx, ye = y0 + dy;
    const double xm = (double)(lv.w[0] - 1), ym = (double)(lv.h[0] - 1);
    const bool inside = x0 >= 0.0 && x0 <= xm && y0 >= 0.0 && y0 <= ym && xe >= 0.0 && xe <= xm && ye >= 0.0 && ye <= ym;
    if (!inside) st |= FOTO_LK_OUT;
    if (lane != 0) return;
    out[2 * pt] = (TO)dx;
    out[2 * pt + 1] = (TO)dy;
    if (err) err[pt] = errv;
    if (prior) {   // the round trip: the caller's status keeps its bits and gains INCONSISTENT
        const double sx = px + dx, sy = py + dy;
        const double f = sqrt(sx * sx + sy * sy);
        if (fb) fb[pt] = f;
        if (!(f <= par.fb_tol)) status[pt] = (unsigned char)(status[pt] | FOTO_LK_INCONSISTENT);
    } else {
        status[pt] = (unsigned char)st;
    }
}

// ----------------------------------------------------------------------------- flow sampling

struct FlowSrc {
    const void* data;
    int inter;
    int64_t rec;   // elements per record
};

// out[r][p] = (S(u_r; x_p, y_p), S(v_r; x_p, y_p)); a NaN coordinate gives NaN from in-frame taps
template <class TF, class TP, class TO>
__global__ __launch_bounds__(NT) void k_flow_sample(FlowSrc fl, int w, int h, int64_t M, int64_t total,
                                                    const TP* __restrict__ pts, TO* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const int64_t r = i / M, p = i - r * M;
    const SampleTaps S = sample_taps(w, h, (double)pts[2 * p], (double)pts[2 * p + 1]);
    const int64_t n = (int64_t)w * h;
    const TF* f = (const TF*)fl.data + r * fl.rec;
    const int64_t p00 = (int64_t)S.j0 * w + S.i0, p01 = p00 + 1, p10 = p00 + w, p11 = p10 + 1;
    double u, v;
    if (fl.inter) {
        u = sample_sum(S, (double)f[2 * p00], (double)f[2 * p01], (double)f[2 * p10], (double)f[2 * p11]);
        v = sample_sum(S, (double)f[2 * p00 + 1], (double)f[2 * p01 + 1], (double)f[2 * p10 + 1],
                       (double)f[2 * p11 + 1]);
    } else {
        u = sample_sum(S, (double)f[p00], (double)f[p01], (double)f[p10], (double)f[p11]);
        v = sample_sum(S, (double)f[n + p00], (double)f[n + p01], (double)f[n + p10], (double)f[n + p11]);
    }
    out[2 * i] = (TO)u;
    out[2 * i + 1] = (TO)v;
}

template <class TF, class TP>
void flow_sample_launch(const FlowSrc& fl, int w, int h, int64_t M, int64_t total, const void* pts, void* out,
                        int dtype, hipStream_t s) {
    const unsigned grid = (unsigned)((total + NT - 1) / NT);
    if (dtype == FOTO_F32) k_flow_sample<TF, TP, float><<<grid, NT, 0, s>>>(fl, w, h, M, total, (const TP*)pts, (float*)out);
    else k_flow_sample<TF, TP, double><<<grid, NT, 0, s>>>(fl, w, h, M, total, (const TP*)pts, (double*)out);
}

// ----------------------------------------------------------------------------- per-device state

// One stream, link and grow-only scratch per device for the entries without a plan (corners,
// sampling), kept for the process like foto_render.hip's.  The calls only enqueue on it.
struct SparseDev {
    hipStream_t s = nullptr;
    StreamLink link;
    DevScratch tmp;
};
std::mutex sp_mu;
std::vector<SparseDev*> sp_dev;

int sparse_dev(int* device, SparseDev** out) {   // (sp_mu held by the caller)
    int dev = 0;
    FOTO_HIP_CHECK(hipGetDevice(&dev));
    if ((int)sp_dev.size() <= dev) sp_dev.resize(dev + 1, nullptr);
    if (!sp_dev[dev]) {
        hipStream_t s = nullptr;
        FOTO_TRY(stream_acquire(&s));
        sp_dev[dev] = new SparseDev();
        sp_dev[dev]->s = s;
    }
    *device = dev;
    *out = sp_dev[dev];
    return 0;
}

int corner_opts_check(const foto_corner_opts& o, const char* who) {
    if (!std::isfinite(o.quality) || o.quality < 0 || o.quality > 1) {
        set_error("%s: quality = %g must be in [0, 1]", who, o.quality);
        return FOTO_ERR_ARG;
    }
    if (o.window < 1 || o.window > FOTO_CORNER_MAX_WINDOW) {
        set_error("%s: window = %d: the box radius is 1 .. %d", who, o.window, FOTO_CORNER_MAX_WINDOW);
        return FOTO_ERR_ARG;
    }
    if (o.nms < 1 || o.nms > FOTO_CORNER_MAX_NMS) {
        set_error("%s: nms = %d: the suppression radius is 1 .. %d", who, o.nms, FOTO_CORNER_MAX_NMS);
        return FOTO_ERR_ARG;
    }
    if (o.margin < 0) { set_error("%s: margin = %d must be >= 0", who, o.margin); return FOTO_ERR_ARG; }
    return 0;
}

int lk_opts_check(const foto_lk_opts& o, const char* who) {
    if (o.radius < 1 || o.radius > FOTO_LK_MAX_RADIUS) {
        set_error("%s: radius = %d: the window radius is 1 .. %d", who, o.radius, FOTO_LK_MAX_RADIUS);
        return FOTO_ERR_ARG;
    }
    if (o.iters < 1) { set_error("%s: iters = %d: the count must be >= 1", who, o.iters); return FOTO_ERR_ARG; }
    if (!std::isfinite(o.min_eig) || o.min_eig < 0) {
        set_error("%s: min_eig = %g must be finite and >= 0", who, o.min_eig);
        return FOTO_ERR_ARG;
    }
    return 0;
}

// a device array of M (x, y) pairs: non-null, F32 | F64, aligned to a pair (host-only)
int pairs_check(const void* p, int dtype, const char* who, const char* what) {
    if (!p) { set_error("%s: %s is null", who, what); return FOTO_ERR_ARG; }
    return track_dtype_check(p, dtype, who, what);
}

int count_check(int64_t M, const char* who) {
    if (M < 1 || M > (int64_t)INT32_MAX) {
        set_error("%s: M = %lld points must be in [1, 2^31 - 1]", who, (long long)M);
        return FOTO_ERR_ARG;
    }
    return 0;
}

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace
}  // namespace foto

using namespace foto;

// ============================================================================ the LK plan (host)

struct foto_lk {
    int w = 0, h = 0, device = 0;
    foto_lk_opts o{};
    std::vector<int> wl, hl;        // level sizes, finest first
    hipStream_t s = nullptr;
    DevArena mem;
    std::vector<double*> f0, f1;    // both frames per level
    bool have_frames = false;
    StreamLink link;

    ~foto_lk() {
        if (s) (void)hipStreamSynchronize(s);
        mem.clear();
        stream_release(s);
    }
};

extern "C" {

int foto_corner_opts_default(foto_corner_opts* o) {
    if (!o) { set_error("foto_corner_opts_default: null argument"); return FOTO_ERR_ARG; }
    o->quality = 0.01;
    o->window = 3;
    o->nms = 5;
    o->margin = 8;
    o->reserved = 0;
    return 0;
}

int foto_corners_dev(const foto_image* frame, int w, int h, const foto_corner_opts* opts, int max_count, void* pts,
                     int pts_dtype, int32_t* count_dev, int* count_host_or_null, double* response_or_null,
                     void* stream) {
    static const char* const who = "foto_corners_dev";
    if (!frame) { set_error("%s: null image descriptor", who); return FOTO_ERR_ARG; }
    FOTO_TRY(image_size_check(w, h, 2, who));
    FOTO_TRY(image_check(frame, w, h, who));
    foto_corner_opts o;
    (void)foto_corner_opts_default(&o);
    if (opts) o = *opts;
    FOTO_TRY(corner_opts_check(o, who));
    if (max_count < 1) { set_error("%s: max_count = %d must be >= 1", who, max_count); return FOTO_ERR_ARG; }
    FOTO_TRY(pairs_check(pts, pts_dtype, who, "pts"));
    if (!count_dev || (uintptr_t)count_dev % sizeof(int32_t) != 0) {
        set_error("%s: count_dev %p is null or not aligned to an int32", who, (void*)count_dev);
        return FOTO_ERR_ARG;
    }
    if (response_or_null && (uintptr_t)response_or_null % sizeof(double) != 0) {
        set_error("%s: response %p is not aligned to a double", who, (void*)response_or_null);
        return FOTO_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(sp_mu);
    int device = 0;
    SparseDev* sd = nullptr;
    FOTO_TRY(sparse_dev(&device, &sd));
    const int64_t n = (int64_t)w * h;
    const size_t pts_bytes = (size_t)max_count * 2 * dtype_bytes(pts_dtype);
    FOTO_TRY(image_dev_check(frame, w, h, device, who));
    FOTO_TRY(dev_ptr_check(pts, pts_bytes, device, who, "pts"));
    FOTO_TRY(dev_ptr_check(count_dev, sizeof(int32_t), device, who, "count_dev"));
    if (response_or_null) FOTO_TRY(dev_ptr_check(response_or_null, (size_t)n * sizeof(double), device, who, "response"));
    // the scratch: the widened frame, R (when the caller takes none), flags, block counts and
    // offsets, the candidate lists, the maximum and the candidate count
    const int nb = (int)((n + CM_PIX - 1) / CM_PIX);
    const int64_t cap64 = (int64_t)((w + o.nms) / (o.nms + 1)) * ((h + o.nms) / (o.nms + 1));
    const int cap = (int)cap64;   // (<= w h / 4 < 2^31)
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t at = off; off += align_up(bytes); return at; };
    const size_t o_f = take((size_t)n * 8), o_r = take(response_or_null ? 0 : (size_t)n * 8), o_flag = take((size_t)n);
    const size_t o_cnt = take((size_t)nb * 4), o_off = take((size_t)nb * 4), o_idx = take((size_t)cap * 4);
    const size_t o_key = take((size_t)cap * 8), o_keep = take((size_t)cap), o_scal = take(16);
    FOTO_TRY(sd->tmp.reserve(off, sd->s));
    char* base = (char*)sd->tmp.p;
    double* f = (double*)(base + o_f);
    double* resp = response_or_null ? response_or_null : (double*)(base + o_r);
    unsigned char* flag = (unsigned char*)(base + o_flag);
    int *blockcnt = (int*)(base + o_cnt), *blockoff = (int*)(base + o_off), *cidx = (int*)(base + o_idx);
    unsigned long long* ckey = (unsigned long long*)(base + o_key);
    unsigned char* keep = (unsigned char*)(base + o_keep);
    unsigned long long* rmax = (unsigned long long*)(base + o_scal);
    int* ccount = (int*)(base + o_scal + 8);
    hipStream_t s = sd->s;
    FOTO_TRY(sd->link.enter((hipStream_t)stream, s));
    auto run = [&]() -> int {
        FOTO_HIP_CHECK(launch_ingest(*frame, w, h, f, s));
        FOTO_HIP_CHECK(hipMemsetAsync(rmax, 0, 16, s));
        const int tiles_x = (w + CT_W - 1) / CT_W;
        const unsigned tiles = (unsigned)tiles_x * (unsigned)((h + CT_H - 1) / CT_H);
        k_corner_response<<<tiles, NT, 0, s>>>(w, h, o.window, tiles_x, f, resp, rmax);
        FOTO_HIP_CHECK(hipGetLastError());
        const CornerPar P{w, h, o.nms, o.margin, o.quality};
        k_corner_mark<<<nb, NT, 0, s>>>(P, resp, rmax, flag, blockcnt);
        FOTO_HIP_CHECK(hipGetLastError());
        k_corner_scan<<<1, NT, 0, s>>>(nb, blockcnt, blockoff, ccount);
        FOTO_HIP_CHECK(hipGetLastError());
        k_corner_gather<<<nb, NT, 0, s>>>(n, resp, flag, blockoff, cap, cidx, ckey);
        FOTO_HIP_CHECK(hipGetLastError());
        k_corner_rank<<<(cap + NT - 1) / NT, NT, 0, s>>>(ccount, cap, ckey, max_count, keep);
        FOTO_HIP_CHECK(hipGetLastError());
        const int eg = (std::max(cap, max_count) + NT - 1) / NT;
        if (pts_dtype == FOTO_F32)
            k_corner_emit<float><<<eg, NT, 0, s>>>(w, ccount, cap, cidx, keep, max_count, (float*)pts, count_dev);
        else
            k_corner_emit<double><<<eg, NT, 0, s>>>(w, ccount, cap, cidx, keep, max_count, (double*)pts, count_dev);
        FOTO_HIP_CHECK(hipGetLastError());
        return 0;
    };
    int rc = run();
    int32_t hc = 0;
    if (rc == 0 && count_host_or_null &&
        hipMemcpyAsync(&hc, count_dev, sizeof(hc), hipMemcpyDeviceToHost, s) != hipSuccess) {
        set_error("%s: the copy of the count failed", who);
        rc = FOTO_ERR_HIP;
    }
    const int rl = sd->link.leave(s, (hipStream_t)stream);
    if (rc < 0) return rc;
    FOTO_TRY(rl);
    if (count_host_or_null) {
        FOTO_HIP_CHECK(hipStreamSynchronize(s));
        *count_host_or_null = hc;
    }
    return 0;
}

int foto_lk_opts_default(foto_lk_opts* o) {
    if (!o) { set_error("foto_lk_opts_default: null argument"); return FOTO_ERR_ARG; }
    o->radius = 7;
    o->levels = 4;
    o->min_size = 16;
    o->iters = 10;
    o->min_eig = 1e-7;
    return 0;
}

int foto_lk_create(int w, int h, const foto_lk_opts* opts, foto_lk** out) {
    if (!out) { set_error("foto_lk_create: null argument"); return FOTO_ERR_ARG; }
    auto P = std::make_unique<foto_lk>();
    (void)foto_lk_opts_default(&P->o);
    if (opts) P->o = *opts;
    int wl[FOTO_GN_PYR_MAX_LEVELS], hl[FOTO_GN_PYR_MAX_LEVELS], L = 0;
    FOTO_TRY(foto_gn_pyr_sizes(w, h, P->o.levels, P->o.min_size, wl, hl, FOTO_GN_PYR_MAX_LEVELS, &L));
    FOTO_TRY(lk_opts_check(P->o, "foto_lk_create"));
    P->w = w; P->h = h;
    P->wl.assign(wl, wl + L);
    P->hl.assign(hl, hl + L);
    FOTO_HIP_CHECK(hipGetDevice(&P->device));
    FOTO_TRY(stream_acquire(&P->s));
    size_t frames = 0;
    for (int l = 0; l < L; ++l) frames += 2 * (size_t)wl[l] * hl[l];
    double* q = nullptr;   // one block: both frames of every level
    FOTO_TRY(P->mem.alloc_n(frames, &q));
    for (int l = 0; l < L; ++l) {
        const size_t n = (size_t)wl[l] * hl[l];
        P->f0.push_back(q); q += n;
        P->f1.push_back(q); q += n;
    }
    *out = P.release();
    return 0;
}

void foto_lk_destroy(foto_lk* p) { delete p; }

int foto_lk_device(const foto_lk* p) { return p ? p->device : -1; }

int foto_lk_set_frames_dev(foto_lk* p, const foto_image* f0, const foto_image* f1, void* stream) {
    static const char* const who = "foto_lk_set_frames_dev";
    if (!p || !f0 || !f1) { set_error("%s: null argument", who); return FOTO_ERR_ARG; }
    FOTO_TRY(image_dev_check(f0, p->w, p->h, p->device, "foto_lk_set_frames_dev (f0)"));
    FOTO_TRY(image_dev_check(f1, p->w, p->h, p->device, "foto_lk_set_frames_dev (f1)"));
    hipStream_t s = p->s;
    FOTO_TRY(p->link.enter((hipStream_t)stream, s));
    auto run = [&]() -> int {
        FOTO_HIP_CHECK(launch_ingest(*f0, p->w, p->h, p->f0[0], s));
        FOTO_HIP_CHECK(launch_ingest(*f1, p->w, p->h, p->f1[0], s));
        for (size_t l = 0; l + 1 < p->wl.size(); ++l)
            FOTO_HIP_CHECK(launch_pyr_down(p->wl[l], p->hl[l], p->f0[l], p->f1[l], p->f0[l + 1], p->f1[l + 1], s));
        return 0;
    };
    const int rc = run();
    const int rl = p->link.leave(s, (hipStream_t)stream);
    p->have_frames = rc == 0;
    return rc < 0 ? rc : rl;
}

int foto_lk_track_dev(foto_lk* p, const void* pts, int pts_dtype, int64_t M, int direction, const void* prior_or_null,
                      double fb_tol, void* out, int dtype, unsigned char* status, double* err_or_null,
                      double* fb_or_null, void* stream) {
    static const char* const who = "foto_lk_track_dev";
    if (!p) { set_error("%s: null plan", who); return FOTO_ERR_ARG; }
    FOTO_TRY(count_check(M, who));
    FOTO_TRY(pairs_check(pts, pts_dtype, who, "pts"));
    FOTO_TRY(pairs_check(out, dtype, who, "out"));
    if (prior_or_null) FOTO_TRY(pairs_check(prior_or_null, dtype, who, "prior"));
    if (!status) { set_error("%s: status is null", who); return FOTO_ERR_ARG; }
    if (direction != 0 && direction != 1) {
        set_error("%s: direction = %d is not 0 (f0 -> f1) / 1 (f1 -> f0)", who, direction);
        return FOTO_ERR_ARG;
    }
    if (fb_or_null && !prior_or_null) {
        set_error("%s: fb is the round trip's length and needs a prior", who);
        return FOTO_ERR_ARG;
    }
    if (prior_or_null && std::isnan(fb_tol)) { set_error("%s: fb_tol is NaN", who); return FOTO_ERR_ARG; }
    if (((uintptr_t)err_or_null | (uintptr_t)fb_or_null) % sizeof(double) != 0) {
        set_error("%s: err / fb is not aligned to a double", who);
        return FOTO_ERR_ARG;
    }
    if (!p->have_frames) { set_error("%s: no frames yet (foto_lk_set_frames_dev)", who); return FOTO_ERR_STATE; }
    const size_t pair_in = 2 * dtype_bytes(pts_dtype), pair_out = 2 * dtype_bytes(dtype);
    FOTO_TRY(dev_ptr_check(pts, (size_t)M * pair_in, p->device, who, "pts"));
    FOTO_TRY(dev_ptr_check(out, (size_t)M * pair_out, p->device, who, "out"));
    if (prior_or_null) FOTO_TRY(dev_ptr_check(prior_or_null, (size_t)M * pair_out, p->device, who, "prior"));
    FOTO_TRY(dev_ptr_check(status, (size_t)M, p->device, who, "status"));
    if (err_or_null) FOTO_TRY(dev_ptr_check(err_or_null, (size_t)M * sizeof(double), p->device, who, "err"));
    if (fb_or_null) FOTO_TRY(dev_ptr_check(fb_or_null, (size_t)M * sizeof(double), p->device, who, "fb"));
    if (overlaps(out, (size_t)M * pair_out, pts, (size_t)M * pair_in) ||
        (prior_or_null && overlaps(out, (size_t)M * pair_out, prior_or_null, (size_t)M * pair_out))) {
        set_error("%s: out may not overlap pts or prior", who);
        return FOTO_ERR_ARG;
    }
    LkLevels lv;
    lv.L = (int)p->wl.size();
    for (int l = 0; l < FOTO_GN_PYR_MAX_LEVELS; ++l) {
        const bool in = l < lv.L;
        lv.w[l] = in ? p->wl[l] : 0;
        lv.h[l] = in ? p->hl[l] : 0;
        lv.a[l] = in ? (direction == 0 ? p->f0[l] : p->f1[l]) : nullptr;
        lv.b[l] = in ? (direction == 0 ? p->f1[l] : p->f0[l]) : nullptr;
    }
    const LkPar par{p->o.radius, p->o.iters, p->o.min_eig, fb_tol};
    const unsigned grid = (unsigned)((M + NT / 64 - 1) / (NT / 64));
    hipStream_t s = p->s;
    FOTO_TRY(p->link.enter((hipStream_t)stream, s));
    if (pts_dtype == FOTO_F32 && dtype == FOTO_F32)
        k_lk_track<float, float><<<grid, NT, 0, s>>>(lv, par, (const float*)pts, (const float*)prior_or_null, M,
                                                     (float*)out, status, err_or_null, fb_or_null);
    else if (pts_dtype == FOTO_F32)
        k_lk_track<float, double><<<grid, NT, 0, s>>>(lv, par, (const float*)pts, (const double*)prior_or_null, M,
                                                      (double*)out, status, err_or_null, fb_or_null);
    else if (dtype == FOTO_F32)
        k_lk_track<double, float><<<grid, NT, 0, s>>>(lv, par, (const double*)pts, (const float*)prior_or_null, M,
                                                      (float*)out, status, err_or_null, fb_or_null);
    else
        k_lk_track<double, double><<<grid, NT, 0, s>>>(lv, par, (const double*)pts, (const double*)prior_or_null, M,
                                                       (double*)out, status, err_or_null, fb_or_null);
    const hipError_t e = hipGetLastError();
    const int rl = p->link.leave(s, (hipStream_t)stream);
    FOTO_HIP_CHECK(e);
    return rl;
}

int foto_flow_sample_dev(const foto_flow* fl, int w, int h, const void* pts, int pts_dtype, int64_t M, void* out,
                         int dtype, void* stream) {
    static const char* const who = "foto_flow_sample_dev";
    FOTO_TRY(flow_check(fl, w, h, who));
    FOTO_TRY(image_size_check(w, h, 2, who));
    FOTO_TRY(count_check(M, who));
    FOTO_TRY(pairs_check(pts, pts_dtype, who, "pts"));
    FOTO_TRY(pairs_check(out, dtype, who, "out"));
    std::lock_guard<std::mutex> lk(sp_mu);
    int device = 0;
    SparseDev* sd = nullptr;
    FOTO_TRY(sparse_dev(&device, &sd));
    const int64_t total = (int64_t)fl->records * M;
    const size_t out_bytes = (size_t)total * 2 * dtype_bytes(dtype), pts_bytes = (size_t)M * 2 * dtype_bytes(pts_dtype);
    if ((total + NT - 1) / NT > (int64_t)INT32_MAX) {
        set_error("%s: records * M = %lld is too large for one launch", who, (long long)total);
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(dev_ptr_check(fl->data, flow_bytes(fl, w, h), device, who, "flow data"));
    FOTO_TRY(dev_ptr_check(pts, pts_bytes, device, who, "pts"));
    FOTO_TRY(dev_ptr_check(out, out_bytes, device, who, "out"));
    if (overlaps(out, out_bytes, fl->data, flow_bytes(fl, w, h)) || overlaps(out, out_bytes, pts, pts_bytes)) {
        set_error("%s: out may not overlap the flow or the points", who);
        return FOTO_ERR_ARG;
    }
    const FlowSrc src{fl->data, fl->layout, (int64_t)(fl->layout == 0 ? 3 : 2) * w * h};
    hipStream_t s = sd->s;
    FOTO_TRY(sd->link.enter((hipStream_t)stream, s));
    if (fl->dtype == FOTO_F32 && pts_dtype == FOTO_F32) flow_sample_launch<float, float>(src, w, h, M, total, pts, out, dtype, s);
    else if (fl->dtype == FOTO_F32) flow_sample_launch<float, double>(src, w, h, M, total, pts, out, dtype, s);
    else if (pts_dtype == FOTO_F32) flow_sample_launch<double, float>(src, w, h, M, total, pts, out, dtype, s);
    else flow_sample_launch<double, double>(src, w, h, M, total, pts, out, dtype, s);
    const hipError_t e = hipGetLastError();
    const int rl = sd->link.leave(s, (hipStream_t)stream);
    FOTO_HIP_CHECK(e);
    return rl;
}

}  // extern "C"

static_assert(sizeof(foto_corner_opts) == 24, "foto_corner_opts layout");
static_assert(sizeof(foto_lk_opts) == 24, "foto_lk_opts layout");
