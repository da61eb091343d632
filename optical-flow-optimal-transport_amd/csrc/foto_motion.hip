// libfoto: global motion on gfx950 -- a RANSAC fit (Fischler & Bolles 1981) of a translation,
// similarity, affine map or homography to tracks or to a dense flow, in frame-normalised
// coordinates (Hartley & Zisserman 2004, 4.4), refined by least squares over its inliers; the
// model's flow field and the residual flow.  include/foto.h has the arithmetic;
// tests/motion_ref.py restates it in numpy and the device is held to it bit for bit
// (-ffp-contract=off, every floating-point sum in one order fixed by M alone).
//
//   k_motion_mark      a correspondence is valid or not; the count per tile of MO_TILE
//   k_motion_scan      one block: the exclusive scan of the tile counts, n_valid
//   k_motion_compact   the valid ones in index order: normalised x, y, X, Y (four planes), index
//   k_motion_hyp       one thread per hypothesis: the minimal system, eliminated in registers
//   k_motion_score     the hot kernel, H x n_valid evaluations: block (x, y) holds a tile of the list
//                      in registers and walks chunk y of the models, staged in LDS and read as a
//                      broadcast; ballot + popcount per wave, the count of hypothesis j kept in lane
//                      j, one LDS integer add per wave and one global integer add per block and
//                      hypothesis after the loop (DESIGN.md 3.19 has the shapes tried)
//   k_motion_pick      one block: the highest score, the lowest index on a tie; NONE below the bar
//   k_motion_accum     the inliers' normal-equation terms: a partial per tile and quantity
//   k_motion_solve     one wave: the tile partials in tile order, the P x P elimination
//   k_motion_final     the mask (scattered to the caller's indices), the count, the residual sum
//   k_motion_finish    one wave: info, rms, the pixel matrix
//   k_motion_field     the field of a model, or a flow minus it: one pass over the flow buffer
// Counts are integers (any order); no floating-point atomic anywhere.  Nothing waits for the host:
// n_valid, the winner and NONE live in device memory and every later kernel reads them there.
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "foto_devmem.h"
#include "foto_devutil.h"
#include "foto_reduce.h"

namespace foto {
namespace {

constexpr int MO_PER = 4, MO_TILE = MO_PER * NT;   // list entries per thread / per block
static_assert(MO_TILE == FOTO_MOTION_TILE, "the tile of include/foto.h");
constexpr double MO_PIVOT = 1e-12;

__host__ __device__ constexpr int mo_k(int model) { return model + 1; }
__host__ __device__ constexpr int mo_P(int model) { return 2 * (model + 1); }

// what the later kernels read of the earlier ones
struct MoState {
    double m[9];   // the current model, normalised coordinates
    int n_valid, none, winner, status;
};

// where the correspondences come from: point arrays, or the lattice of a flow record
struct MoSrc {
    const void *pts, *disp;            // [M][2]
    const unsigned char* status;       // [M] or null
    int pts_dtype, disp_dtype;
    const void* flow;                  // the record's first element; null: the point arrays
    const unsigned char* mask;         // [h][w] or null
    int fdtype, inter, w, stride, lw;
    int64_t plane;                     // w h
    double s, cx, cy;
};

__device__ __forceinline__ double ld_f(const void* p, int dtype, int64_t i) {
    return dtype == FOTO_F32 ? (double)((const float*)p)[i] : ((const double*)p)[i];
}

// correspondence i: valid or not, and its normalised coordinates
__device__ __forceinline__ bool mo_load(const MoSrc& S, int64_t i, double& x, double& y, double& X, double& Y) {
    double px, py, dx, dy;
    bool ok;
    if (S.flow) {
        const int lj = (int)(i / S.lw), li = (int)(i - (int64_t)lj * S.lw);
        const int64_t pix = (int64_t)(lj * S.stride) * S.w + li * S.stride;
        px = (double)(li * S.stride);
        py = (double)(lj * S.stride);
        dx = ld_f(S.flow, S.fdtype, S.inter ? 2 * pix : pix);
        dy = ld_f(S.flow, S.fdtype, S.inter ? 2 * pix + 1 : S.plane + pix);
        ok = !S.mask || S.mask[pix] != 0;
    } else {
        px = ld_f(S.pts, S.pts_dtype, 2 * i);
        py = ld_f(S.pts, S.pts_dtype, 2 * i + 1);
        dx = ld_f(S.disp, S.disp_dtype, 2 * i);
        dy = ld_f(S.disp, S.disp_dtype, 2 * i + 1);
        ok = !S.status || S.status[i] == 0;
    }
    ok = ok && isfinite(px) && isfinite(py) && isfinite(dx) && isfinite(dy);
    x = (px - S.cx) / S.s;
    y = (py - S.cy) / S.s;
    X = ((px + dx) - S.cx) / S.s;
    Y = ((py + dy) - S.cy) / S.s;
    return ok;
}

// the exclusive prefix of v over the block's threads and the block's total; sh: NT / 64 ints
__device__ __forceinline__ int mo_excl_scan(int v, int* sh, int& total) {
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
    __syncthreads();
    return base + x - v;
}

__global__ __launch_bounds__(NT) void k_motion_mark(MoSrc S, int64_t M, int* __restrict__ tilecnt) {
    __shared__ int sh[NT / 64];
    const int64_t base = (int64_t)blockIdx.x * MO_TILE + (int64_t)threadIdx.x * MO_PER;
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < MO_PER; ++q) {
        double x, y, X, Y;
        if (base + q < M && mo_load(S, base + q, x, y, X, Y)) ++cnt;
    }
    int total;
    (void)mo_excl_scan(cnt, sh, total);
    if (threadIdx.x == 0) tilecnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(NT) void k_motion_scan(int nb, const int* __restrict__ tilecnt, int* __restrict__ off,
                                                    MoState* st) {
    __shared__ int sh[NT / 64];
    int running = 0;
    for (int base = 0; base < nb; base += NT) {
        const int b = base + threadIdx.x;
        const int v = b < nb ? tilecnt[b] : 0;
        int total;
        const int e = mo_excl_scan(v, sh, total);
        if (b < nb) off[b] = running + e;
        running += total;
    }
    if (threadIdx.x == 0) st->n_valid = running;
}

// c: four planes of M doubles (x, y, X, Y of list entry q); idx[q] = the caller's index
__global__ __launch_bounds__(NT) void k_motion_compact(MoSrc S, int64_t M, const int* __restrict__ off,
                                                       double* __restrict__ c, int* __restrict__ idx) {
    __shared__ int sh[NT / 64];
    const int64_t base = (int64_t)blockIdx.x * MO_TILE + (int64_t)threadIdx.x * MO_PER;
    bool ok[MO_PER];
    double v[MO_PER][4];
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < MO_PER; ++q) {
        ok[q] = base + q < M && mo_load(S, base + q, v[q][0], v[q][1], v[q][2], v[q][3]);
        cnt += ok[q] ? 1 : 0;
    }
    int total;
    int64_t pos = off[blockIdx.x] + mo_excl_scan(cnt, sh, total);
#pragma unroll
    for (int q = 0; q < MO_PER; ++q) {
        if (!ok[q]) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) c[e * M + pos] = v[q][e];
        idx[pos] = (int)(base + q);
        ++pos;
    }
}

// ----------------------------------------------------------------------------- the models

// the two rows and right-hand sides of a correspondence (include/foto.h)
template <int MODEL>
__device__ __forceinline__ void mo_rows(double x, double y, double X, double Y, double (&r1)[mo_P(MODEL)],
                                        double (&r2)[mo_P(MODEL)], double& b1, double& b2) {
    if constexpr (MODEL == FOTO_MOTION_TRANSLATION) {
        r1[0] = 1.0; r1[1] = 0.0;
        r2[0] = 0.0; r2[1] = 1.0;
        b1 = X - x;
        b2 = Y - y;
    } else if constexpr (MODEL == FOTO_MOTION_SIMILARITY) {
        r1[0] = x; r1[1] = -y; r1[2] = 1.0; r1[3] = 0.0;
        r2[0] = y; r2[1] = x; r2[2] = 0.0; r2[3] = 1.0;
        b1 = X;
        b2 = Y;
    } else {
        r1[0] = x; r1[1] = y; r1[2] = 1.0; r1[3] = 0.0; r1[4] = 0.0; r1[5] = 0.0;
        r2[0] = 0.0; r2[1] = 0.0; r2[2] = 0.0; r2[3] = x; r2[4] = y; r2[5] = 1.0;
        if constexpr (MODEL == FOTO_MOTION_HOMOGRAPHY) {
            r1[6] = -(X * x); r1[7] = -(X * y);
            r2[6] = -(Y * x); r2[7] = -(Y * y);
        }
        b1 = X;
        b2 = Y;
    }
}

template <int MODEL>
__device__ __forceinline__ void mo_matrix(const double (&p)[mo_P(MODEL)], double* m) {
    if constexpr (MODEL == FOTO_MOTION_TRANSLATION) {
        m[0] = 1.0; m[1] = 0.0; m[2] = p[0];
        m[3] = 0.0; m[4] = 1.0; m[5] = p[1];
        m[6] = 0.0; m[7] = 0.0;
    } else if constexpr (MODEL == FOTO_MOTION_SIMILARITY) {
        m[0] = p[0]; m[1] = -p[1]; m[2] = p[2];
        m[3] = p[1]; m[4] = p[0]; m[5] = p[3];
        m[6] = 0.0; m[7] = 0.0;
    } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) m[i] = p[i];
        m[6] = MODEL == FOTO_MOTION_HOMOGRAPHY ? p[mo_P(MODEL) - 2] : 0.0;
        m[7] = MODEL == FOTO_MOTION_HOMOGRAPHY ? p[mo_P(MODEL) - 1] : 0.0;
    }
    m[8] = 1.0;
}

// The elimination of include/foto.h; false: degenerate.  Every loop unrolls and the pivot row is
// exchanged by a compare per row, not by an index, so A is addressed statically (the 6 x 6 and
// 8 x 8 systems still spill a few hundred bytes: H threads and one thread run them, not the
// hot kernel).
template <int N>
__device__ __forceinline__ bool mo_solve(double (&A)[N][N], double (&b)[N], double (&p)[N]) {
#pragma unroll
    for (int c = 0; c < N; ++c) {
        int piv = c;
        double best = fabs(A[c][c]);
#pragma unroll
        for (int r = c + 1; r < N; ++r) {
            const double a = fabs(A[r][c]);
            if (a > best) {
                best = a;
                piv = r;
            }
        }
        if (!(best > MO_PIVOT)) return false;
#pragma unroll
        for (int r = c + 1; r < N; ++r) {
            if (r != piv) continue;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const double t = A[c][j];
                A[c][j] = A[r][j];
                A[r][j] = t;
            }
            const double t = b[c];
            b[c] = b[r];
            b[r] = t;
        }
#pragma unroll
        for (int r = c + 1; r < N; ++r) {
            const double f = A[r][c] / A[c][c];
#pragma unroll
            for (int j = c + 1; j < N; ++j) A[r][j] = A[r][j] - f * A[c][j];
            b[r] = b[r] - f * b[c];
        }
    }
#pragma unroll
    for (int r = N - 1; r >= 0; --r) {
        double s = b[r];
#pragma unroll
        for (int j = r + 1; j < N; ++j) s = s - A[r][j] * p[j];
        p[r] = s / A[r][r];
    }
    return true;
}

// hyp[j][9]: the model of hypothesis j (NaN when degenerate: it has no inlier); score[j] = 0 or -1
template <int MODEL>
__global__ __launch_bounds__(64) void k_motion_hyp(const MoState* __restrict__ st, int64_t M,
                                                   const double* __restrict__ c, const uint32_t* __restrict__ samples,
                                                   int H, double* __restrict__ hyp, int* __restrict__ score) {
    constexpr int K = mo_k(MODEL), P = mo_P(MODEL);
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= H) return;
    const int n = st->n_valid;
    double m[9];
    bool ok = n >= K;
    if (ok) {
        double A[P][P], b[P], p[P];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const int64_t q = (int64_t)(((uint64_t)samples[4 * j + i] * (uint64_t)n) >> 32);
            mo_rows<MODEL>(c[q], c[M + q], c[2 * M + q], c[3 * M + q], A[2 * i], A[2 * i + 1], b[2 * i], b[2 * i + 1]);
        }
        ok = mo_solve<P>(A, b, p);
        if (ok) mo_matrix<MODEL>(p, m);
    }
    if (!ok) {
#pragma unroll
        for (int i = 0; i < 9; ++i) m[i] = NAN;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) hyp[9 * (int64_t)j + i] = m[i];
    score[j] = ok ? 0 : -1;
}

// the inlier rule of include/foto.h; t2 = (threshold / s)^2
__device__ __forceinline__ bool mo_inlier(const double* __restrict__ m, double x, double y, double X, double Y,
                                          double t2) {
    const double wv = (m[6] * x + m[7] * y) + 1.0;
    const double ex = ((m[0] * x + m[1] * y) + m[2]) - X * wv;
    const double ey = ((m[3] * x + m[4] * y) + m[5]) - Y * wv;
    return wv > 0.0 && ex * ex + ey * ey <= t2 * (wv * wv);
}

// this thread's entries of tile blockIdx.x: q = tile base + slot * NT + thread
struct MoTile {
    double x[MO_PER], y[MO_PER], X[MO_PER], Y[MO_PER];
    bool on[MO_PER];
};
__device__ __forceinline__ void mo_tile_load(MoTile& T, const double* __restrict__ c, int64_t M, int n) {
#pragma unroll
    for (int k = 0; k < MO_PER; ++k) {
        const int64_t q = (int64_t)blockIdx.x * MO_TILE + k * NT + threadIdx.x;
        T.on[k] = q < n;
        const int64_t qq = T.on[k] ? q : 0;
        T.x[k] = c[qq];
        T.y[k] = c[M + qq];
        T.X[k] = c[2 * M + qq];
        T.Y[k] = c[3 * M + qq];
    }
}

constexpr int SC_PER = 2, SC_TILE = SC_PER * NT;   // list entries per thread / block
constexpr int SC_HC = 32;                          // hypotheses per block: a lane each
constexpr int SC_MAX_Y = 256;                      // hypothesis chunks in the grid; a block walks the rest
static_assert(SC_HC <= 64 && SC_HC <= NT, "a hypothesis of the chunk per lane");

// Block (x, y): SC_TILE list entries in registers against the hypotheses of chunk y (and y +
// gridDim.y, ..), staged in LDS and read as a broadcast.  Lane j of a wave keeps the wave's count
// for hypothesis j of the chunk: no atomic inside the loop.
__global__ __launch_bounds__(NT) void k_motion_score(const MoState* __restrict__ st, int64_t M,
                                                     const double* __restrict__ c, const double* __restrict__ hyp,
                                                     int H, double t2, int* score) {
    __shared__ double sm[SC_HC * 9];
    __shared__ int scnt[SC_HC];
    const int n = st->n_valid, lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * SC_TILE;
    if (base >= n) return;   // (the whole block)
    double x[SC_PER], y[SC_PER], X[SC_PER], Y[SC_PER];
    bool on[SC_PER];
#pragma unroll
    for (int k = 0; k < SC_PER; ++k) {
        const int64_t q = base + k * NT + threadIdx.x;
        on[k] = q < n;
        const int64_t qq = on[k] ? q : 0;
        x[k] = c[qq];
        y[k] = c[M + qq];
        X[k] = c[2 * M + qq];
        Y[k] = c[3 * M + qq];
    }
    for (int h0 = blockIdx.y * SC_HC; h0 < H; h0 += gridDim.y * SC_HC) {
        const int hc = min(SC_HC, H - h0);
        for (int l = threadIdx.x; l < hc * 9; l += NT) sm[l] = hyp[9 * (int64_t)h0 + l];
        if (threadIdx.x < SC_HC) scnt[threadIdx.x] = 0;
        __syncthreads();
        int mine = 0;
        for (int j = 0; j < hc; ++j) {
            const double* m = &sm[9 * j];
            int cnt = 0;
#pragma unroll
            for (int k = 0; k < SC_PER; ++k)
                cnt += __popcll(__ballot(on[k] && mo_inlier(m, x[k], y[k], X[k], Y[k], t2)));
            if (lane == j) mine = cnt;
        }
        if (mine) atomicAdd(&scnt[lane], mine);   // (mine != 0 only in a lane < hc)
        __syncthreads();
        if ((int)threadIdx.x < hc && scnt[threadIdx.x]) atomicAdd(&score[h0 + threadIdx.x], scnt[threadIdx.x]);
        __syncthreads();
    }
}

__global__ __launch_bounds__(NT) void k_motion_pick(MoState* st, const double* __restrict__ hyp,
                                                    const int* __restrict__ score, int H, int bar) {
    __shared__ int sbest[NT], sidx[NT];
    int best = -2, at = 0;
    for (int j = threadIdx.x; j < H; j += NT) {
        const int v = score[j];
        if (v > best) {
            best = v;
            at = j;
        }
    }
    sbest[threadIdx.x] = best;
    sidx[threadIdx.x] = at;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {   // the better of two: the higher score, the lower index on a tie
        if ((int)threadIdx.x < o) {
            const int b2 = sbest[threadIdx.x + o], a2 = sidx[threadIdx.x + o];
            if (b2 > sbest[threadIdx.x] || (b2 == sbest[threadIdx.x] && b2 > -2 && a2 < sidx[threadIdx.x])) {
                sbest[threadIdx.x] = b2;
                sidx[threadIdx.x] = a2;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    best = sbest[0];
    at = sidx[0];
    const bool none = best < bar;
    st->none = none ? 1 : 0;
    st->winner = none ? -1 : at;
    st->status = none ? FOTO_MOTION_NONE : 0;
    for (int i = 0; i < 9; ++i) st->m[i] = none ? ((i & 3) == 0 ? 1.0 : 0.0) : hyp[9 * (int64_t)at + i];
}

// The sum order of include/foto.h for one tile: the thread's four slots are already added into v;
// wave tree, then the four waves in order.  The tile's sum in thread 0.  sh: NT / 64 doubles.
__device__ __forceinline__ double mo_tile_sum(double v, double* sh) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __syncthreads();
    return s;
}
static_assert(NT / 64 == 4, "four wave sums per tile");

template <int MODEL>
constexpr int mo_nsum() { return mo_P(MODEL) * (mo_P(MODEL) + 1) / 2 + mo_P(MODEL); }

// part[k * nb + tile]: quantity k = the upper triangle of N row by row, then g; cnt[tile]
template <int MODEL>
__global__ __launch_bounds__(NT) void k_motion_accum(const MoState* __restrict__ st, int64_t M,
                                                     const double* __restrict__ c, double t2,
                                                     double* __restrict__ part, int* __restrict__ cnt) {
    constexpr int P = mo_P(MODEL), NS = mo_nsum<MODEL>();
    __shared__ double sh[NT / 64];
    __shared__ int shc[NT / 64];
    if (st->none) return;
    const int n = st->n_valid, nb = gridDim.x;
    double m[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = st->m[i];
    MoTile T;
    mo_tile_load(T, c, M, n);
    double acc[NS];
    int mine = 0;
#pragma unroll
    for (int k = 0; k < MO_PER; ++k) {
        const bool in = T.on[k] && mo_inlier(m, T.x[k], T.y[k], T.X[k], T.Y[k], t2);
        mine += in ? 1 : 0;
        double r1[P], r2[P], b1, b2;
        mo_rows<MODEL>(T.x[k], T.y[k], T.X[k], T.Y[k], r1, r2, b1, b2);
        int s = 0;
#pragma unroll
        for (int a = 0; a < P; ++a)
#pragma unroll
            for (int b = a; b < P; ++b, ++s) {
                const double t = in ? r1[a] * r1[b] + r2[a] * r2[b] : 0.0;
                acc[s] = k == 0 ? t : acc[s] + t;
            }
#pragma unroll
        for (int a = 0; a < P; ++a, ++s) {
            const double t = in ? r1[a] * b1 + r2[a] * b2 : 0.0;
            acc[s] = k == 0 ? t : acc[s] + t;
        }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const double v = mo_tile_sum(acc[s], sh);
        if (threadIdx.x == 0) part[(int64_t)s * nb + blockIdx.x] = v;
    }
    mine = __popcll(__ballot(mine & 1)) + 2 * __popcll(__ballot(mine & 2)) + 4 * __popcll(__ballot(mine & 4));
    if ((threadIdx.x & 63) == 0) shc[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = shc[0] + shc[1] + shc[2] + shc[3];
}

// 0.0 + p[0] + p[1] + .. in that order; the loads of 16 terms are issued ahead of their adds
__device__ __forceinline__ double mo_serial_sum(const double* __restrict__ p, int nb) {
    double s = 0.0;
    for (int b0 = 0; b0 < nb; b0 += 16) {
        double t[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) t[i] = p[min(b0 + i, nb - 1)];
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (b0 + i < nb) s += t[i];
    }
    return s;
}

// the sum of cnt[0 .. nb) in every lane of the (single) wave
__device__ __forceinline__ int mo_count(const int* __restrict__ cnt, int nb) {
    int v = 0;
    for (int b = threadIdx.x; b < nb; b += 64) v += cnt[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int MODEL>
__global__ __launch_bounds__(64) void k_motion_solve(MoState* st, int nb, const double* __restrict__ part,
                                                     const int* __restrict__ cnt) {
    constexpr int K = mo_k(MODEL), P = mo_P(MODEL), NS = mo_nsum<MODEL>();
    __shared__ double tot[NS];
    if (st->none) return;
    const int inl = mo_count(cnt, nb);
    if (inl < K) {
        if (threadIdx.x == 0) st->status |= FOTO_MOTION_KEPT;
        return;
    }
    if ((int)threadIdx.x < NS) {
        tot[threadIdx.x] = mo_serial_sum(part + (int64_t)threadIdx.x * nb, nb);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double A[P][P], g[P], p[P];
    int s = 0;
#pragma unroll
    for (int a = 0; a < P; ++a)
#pragma unroll
        for (int b = a; b < P; ++b, ++s) {
            A[a][b] = tot[s];
            A[b][a] = tot[s];
        }
#pragma unroll
    for (int a = 0; a < P; ++a, ++s) g[a] = tot[s];
    if (!mo_solve<P>(A, g, p)) {
        st->status |= FOTO_MOTION_KEPT;
        return;
    }
    double m[9];
    mo_matrix<MODEL>(p, m);
    for (int i = 0; i < 9; ++i) st->m[i] = m[i];
}

__global__ __launch_bounds__(NT) void k_motion_final(const MoState* __restrict__ st, int64_t M,
                                                     const double* __restrict__ c, const int* __restrict__ idx,
                                                     double t2, unsigned char* __restrict__ mask,
                                                     double* __restrict__ part, int* __restrict__ cnt) {
    __shared__ double sh[NT / 64];
    __shared__ int shc[NT / 64];
    const int n = st->n_valid;
    const bool none = st->none != 0;
    double m[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = st->m[i];
    MoTile T;
    mo_tile_load(T, c, M, n);
    double acc = 0.0;
    int mine = 0;
#pragma unroll
    for (int k = 0; k < MO_PER; ++k) {
        const bool in = !none && T.on[k] && mo_inlier(m, T.x[k], T.y[k], T.X[k], T.Y[k], t2);
        const double wv = (m[6] * T.x[k] + m[7] * T.y[k]) + 1.0;
        const double rx = ((m[0] * T.x[k] + m[1] * T.y[k]) + m[2]) / wv - T.X[k];
        const double ry = ((m[3] * T.x[k] + m[4] * T.y[k]) + m[5]) / wv - T.Y[k];
        const double t = in ? rx * rx + ry * ry : 0.0;
        acc = k == 0 ? t : acc + t;
        mine += in ? 1 : 0;
        if (T.on[k]) mask[idx[(int64_t)blockIdx.x * MO_TILE + k * NT + threadIdx.x]] = in ? 1 : 0;
    }
    const double v = mo_tile_sum(acc, sh);
    mine = __popcll(__ballot(mine & 1)) + 2 * __popcll(__ballot(mine & 2)) + 4 * __popcll(__ballot(mine & 4));
    if ((threadIdx.x & 63) == 0) shc[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        part[blockIdx.x] = v;
        cnt[blockIdx.x] = shc[0] + shc[1] + shc[2] + shc[3];
    }
}

__global__ __launch_bounds__(64) void k_motion_finish(const MoState* __restrict__ st, int nb,
                                                      const double* __restrict__ part, const int* __restrict__ cnt,
                                                      double s, double cx, double cy, double* __restrict__ model,
                                                      int64_t* __restrict__ info, double* __restrict__ rms) {
    const int inl = mo_count(cnt, nb);
    if (threadIdx.x != 0) return;
    const double S = mo_serial_sum(part, nb);
    rms[0] = s * sqrt(S / (double)inl);
    info[0] = inl;
    info[1] = st->n_valid;
    info[2] = st->winner;
    info[3] = st->status;
    if (st->none) {
        for (int i = 0; i < 9; ++i) model[i] = (i & 3) == 0 ? 1.0 : 0.0;
        return;
    }
    double A[3][3], B[3][3];
    for (int i = 0; i < 3; ++i) {
        const double m0 = st->m[3 * i], m1 = st->m[3 * i + 1], m2 = st->m[3 * i + 2];
        A[i][0] = m0 / s;
        A[i][1] = m1 / s;
        A[i][2] = (m2 - (m0 * cx) / s) - (m1 * cy) / s;
    }
    for (int j = 0; j < 3; ++j) {
        B[0][j] = s * A[0][j] + cx * A[2][j];
        B[1][j] = s * A[1][j] + cy * A[2][j];
        B[2][j] = A[2][j];
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) model[3 * i + j] = B[i][j] / B[2][2];
    model[8] = 1.0;
}

// ----------------------------------------------------------------------------- field and residual

// the field of include/foto.h at pixel (x, y)
__device__ __forceinline__ void mo_field(const double* __restrict__ m, int x, int y, double& u, double& v) {
    const double fx = (double)x, fy = (double)y;
    const double wv = (m[6] * fx + m[7] * fy) + m[8];
    u = ((m[0] * fx + m[1] * fy) + m[2]) / wv - fx;
    v = ((m[3] * fx + m[4] * fy) + m[5]) / wv - fy;
    if (!(wv > 0.0)) u = v = NAN;
}

// One thread per pixel and record.  FLOW: out = flow - field with m copied; else out = field, m = 0.
// mstride: 9 (a model per record) or 0 (one model for all).
template <class TF, bool FLOW>
__global__ __launch_bounds__(NT) void k_motion_field(const TF* __restrict__ fl, const double* __restrict__ models,
                                                     int mstride, int w, int64_t n, int64_t total, int inter,
                                                     TF* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (t >= total) return;
    const int64_t r = t / n, i = t - r * n;
    const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
    double u, v;
    mo_field(models + r * mstride, x, y, u, v);
    const int64_t rec = r * (inter ? 2 : 3) * n;
    const int64_t iu = rec + (inter ? 2 * i : i), iv = rec + (inter ? 2 * i + 1 : n + i);
    if constexpr (FLOW) {
        u = (double)fl[iu] - u;
        v = (double)fl[iv] - v;
    }
    out[iu] = (TF)u;
    out[iv] = (TF)v;
    if (!inter) out[rec + 2 * n + i] = FLOW ? fl[rec + 2 * n + i] : (TF)0.0;
}

// ----------------------------------------------------------------------------- per-device state

// One stream, link, grow-only scratch and sample table per device, kept for the process like
// foto_sparse.hip's.  The calls only enqueue on the stream.
struct MotionDev {
    hipStream_t s = nullptr;
    StreamLink link;
    DevScratch tmp, table;
    std::vector<uint32_t> samples;   // the host copy of what `table` holds
};
std::mutex mo_mu;
std::vector<MotionDev*> mo_dev;

int motion_dev(int* device, MotionDev** out) {   // (mo_mu held by the caller)
    int dev = 0;
    FOTO_HIP_CHECK(hipGetDevice(&dev));
    if ((int)mo_dev.size() <= dev) mo_dev.resize(dev + 1, nullptr);
    if (!mo_dev[dev]) {
        hipStream_t s = nullptr;
        FOTO_TRY(stream_acquire(&s));
        mo_dev[dev] = new MotionDev();
        mo_dev[dev]->s = s;
    }
    *device = dev;
    *out = mo_dev[dev];
    return 0;
}

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// the rules of the fit that need no device
int fit_args_check(int64_t M, int w, int h, const foto_motion_opts* o, const uint32_t* samples, int H,
                   const double* model, const unsigned char* inliers, const int64_t* info, const double* rms,
                   const char* who) {
    if (!o || !samples || !model || !inliers || !info || !rms) { set_error("%s: null argument", who); return FOTO_ERR_ARG; }
    if (M < 1 || M > (int64_t)INT32_MAX) {
        set_error("%s: M = %lld correspondences must be in [1, 2^31 - 1]", who, (long long)M);
        return FOTO_ERR_ARG;
    }
    if (H < 1) { set_error("%s: H = %d hypotheses must be >= 1", who, H); return FOTO_ERR_ARG; }
    if (o->model < FOTO_MOTION_TRANSLATION || o->model > FOTO_MOTION_HOMOGRAPHY) {
        set_error("%s: model = %d is not FOTO_MOTION_TRANSLATION .. FOTO_MOTION_HOMOGRAPHY", who, o->model);
        return FOTO_ERR_ARG;
    }
    if (!std::isfinite(o->threshold) || !(o->threshold > 0)) {
        set_error("%s: threshold = %g must be finite and > 0", who, o->threshold);
        return FOTO_ERR_ARG;
    }
    if (o->rounds < 0 || o->min_inliers < 0) {
        set_error("%s: rounds = %d and min_inliers = %d must be >= 0", who, o->rounds, o->min_inliers);
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(image_size_check(w, h, 2, who));
    if (((uintptr_t)model | (uintptr_t)info | (uintptr_t)rms) % 8 != 0) {
        set_error("%s: model / info / rms is not aligned to 8 bytes", who);
        return FOTO_ERR_ARG;
    }
    return 0;
}

struct FitIn {
    const void* p;
    size_t bytes;
    const char* what;
};

// The fit on correspondences S (the device pointers of `in` and the outputs are checked here).
int fit_run(MoSrc S, int64_t M, int w, int h, const foto_motion_opts& o, const uint32_t* samples, int H,
            const FitIn* in, int n_in, double* model, unsigned char* inliers, int64_t* info, double* rms,
            void* stream, const char* who) {
    std::lock_guard<std::mutex> lk(mo_mu);
    int device = 0;
    MotionDev* md = nullptr;
    FOTO_TRY(motion_dev(&device, &md));
    const FitIn outs[4] = {{model, 9 * sizeof(double), "model"}, {inliers, (size_t)M, "inliers"},
                           {info, 4 * sizeof(int64_t), "info"}, {rms, sizeof(double), "rms"}};
    for (int i = 0; i < n_in; ++i) FOTO_TRY(dev_ptr_check(in[i].p, in[i].bytes, device, who, in[i].what));
    for (const FitIn& t : outs) FOTO_TRY(dev_ptr_check(t.p, t.bytes, device, who, t.what));
    for (int a = 0; a < 4; ++a) {
        for (int i = 0; i < n_in; ++i)
            if (overlaps(outs[a].p, outs[a].bytes, in[i].p, in[i].bytes)) {
                set_error("%s: %s may not overlap %s", who, outs[a].what, in[i].what);
                return FOTO_ERR_ARG;
            }
        for (int b = a + 1; b < 4; ++b)
            if (overlaps(outs[a].p, outs[a].bytes, outs[b].p, outs[b].bytes)) {
                set_error("%s: %s may not overlap %s", who, outs[a].what, outs[b].what);
                return FOTO_ERR_ARG;
            }
    }
    hipStream_t s = md->s;
    // the sample table: uploaded when it differs from the previous call's
    const size_t tbytes = (size_t)H * 4 * sizeof(uint32_t);
    if (md->samples.size() != (size_t)H * 4 || std::memcmp(md->samples.data(), samples, tbytes) != 0) {
        FOTO_HIP_CHECK(hipStreamSynchronize(s));   // (an earlier call may still read the old table)
        FOTO_TRY(md->table.reserve(tbytes, s));
        md->samples.assign(samples, samples + (size_t)H * 4);
        FOTO_HIP_CHECK(hipMemcpyAsync(md->table.p, md->samples.data(), tbytes, hipMemcpyHostToDevice, s));
    }
    const int nb = (int)((M + MO_TILE - 1) / MO_TILE);
    const int K = mo_k(o.model), NS = mo_P(o.model) * (mo_P(o.model) + 1) / 2 + mo_P(o.model);
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t at = off; off += align_up(bytes); return at; };
    const size_t o_st = take(sizeof(MoState)), o_c = take((size_t)M * 4 * 8), o_idx = take((size_t)M * 4);
    const size_t o_tc = take((size_t)nb * 4), o_to = take((size_t)nb * 4), o_hyp = take((size_t)H * 9 * 8);
    const size_t o_sc = take((size_t)H * 4), o_part = take((size_t)NS * nb * 8), o_cnt = take((size_t)nb * 4);
    FOTO_TRY(md->tmp.reserve(off, s));
    char* base = (char*)md->tmp.p;
    MoState* st = (MoState*)(base + o_st);
    double* c = (double*)(base + o_c);
    int *idx = (int*)(base + o_idx), *tilecnt = (int*)(base + o_tc), *tileoff = (int*)(base + o_to);
    double* hyp = (double*)(base + o_hyp);
    int* score = (int*)(base + o_sc);
    double* part = (double*)(base + o_part);
    int* cnt = (int*)(base + o_cnt);
    const uint32_t* table = (const uint32_t*)md->table.p;
    S.s = 0.5 * (double)std::max(w, h);
    S.cx = 0.5 * (double)(w - 1);
    S.cy = 0.5 * (double)(h - 1);
    const double t = o.threshold / S.s, t2 = t * t;
    const int bar = std::max(K, o.min_inliers);
    FOTO_TRY(md->link.enter((hipStream_t)stream, s));
    auto run = [&]() -> int {
        FOTO_HIP_CHECK(hipMemsetAsync(inliers, 0, (size_t)M, s));
        k_motion_mark<<<nb, NT, 0, s>>>(S, M, tilecnt);
        k_motion_scan<<<1, NT, 0, s>>>(nb, tilecnt, tileoff, st);
        k_motion_compact<<<nb, NT, 0, s>>>(S, M, tileoff, c, idx);
        FOTO_HIP_CHECK(hipGetLastError());
        const int hg = (int)(((int64_t)H + 63) / 64);
        switch (o.model) {
        case FOTO_MOTION_TRANSLATION: k_motion_hyp<0><<<hg, 64, 0, s>>>(st, M, c, table, H, hyp, score); break;
        case FOTO_MOTION_SIMILARITY: k_motion_hyp<1><<<hg, 64, 0, s>>>(st, M, c, table, H, hyp, score); break;
        case FOTO_MOTION_AFFINE: k_motion_hyp<2><<<hg, 64, 0, s>>>(st, M, c, table, H, hyp, score); break;
        default: k_motion_hyp<3><<<hg, 64, 0, s>>>(st, M, c, table, H, hyp, score); break;
        }
        k_motion_score<<<dim3((unsigned)((M + SC_TILE - 1) / SC_TILE), (unsigned)std::min<int64_t>(((int64_t)H + SC_HC - 1) / SC_HC, SC_MAX_Y)),
                         NT, 0, s>>>(st, M, c, hyp, H, t2, score);
        k_motion_pick<<<1, NT, 0, s>>>(st, hyp, score, H, bar);
        FOTO_HIP_CHECK(hipGetLastError());
        for (int r = 0; r < o.rounds; ++r) {
            switch (o.model) {
            case FOTO_MOTION_TRANSLATION:
                k_motion_accum<0><<<nb, NT, 0, s>>>(st, M, c, t2, part, cnt);
                k_motion_solve<0><<<1, 64, 0, s>>>(st, nb, part, cnt);
                break;
            case FOTO_MOTION_SIMILARITY:
                k_motion_accum<1><<<nb, NT, 0, s>>>(st, M, c, t2, part, cnt);
                k_motion_solve<1><<<1, 64, 0, s>>>(st, nb, part, cnt);
                break;
            case FOTO_MOTION_AFFINE:
                k_motion_accum<2><<<nb, NT, 0, s>>>(st, M, c, t2, part, cnt);
                k_motion_solve<2><<<1, 64, 0, s>>>(st, nb, part, cnt);
                break;
            default:
                k_motion_accum<3><<<nb, NT, 0, s>>>(st, M, c, t2, part, cnt);
                k_motion_solve<3><<<1, 64, 0, s>>>(st, nb, part, cnt);
                break;
            }
            FOTO_HIP_CHECK(hipGetLastError());
        }
        k_motion_final<<<nb, NT, 0, s>>>(st, M, c, idx, t2, inliers, part, cnt);
        k_motion_finish<<<1, 64, 0, s>>>(st, nb, part, cnt, S.s, S.cx, S.cy, model, info, rms);
        FOTO_HIP_CHECK(hipGetLastError());
        return 0;
    };
    const int rc = run();
    const int rl = md->link.leave(s, (hipStream_t)stream);
    return rc < 0 ? rc : rl;
}

template <class TF>
void field_launch(bool flow, const void* fl, const double* models, int mstride, int w, int64_t n, int64_t total,
                  int inter, void* out, hipStream_t s) {
    const unsigned grid = (unsigned)((total + NT - 1) / NT);
    if (flow) k_motion_field<TF, true><<<grid, NT, 0, s>>>((const TF*)fl, models, mstride, w, n, total, inter, (TF*)out);
    else k_motion_field<TF, false><<<grid, NT, 0, s>>>(nullptr, models, mstride, w, n, total, inter, (TF*)out);
}

// the shared body of the field and the residual: fl null = the field alone
int field_run(const foto_flow* fl, const double* models, int count, int records, int w, int h, void* out, int dtype,
              int layout, void* stream, const char* who) {
    const int64_t n = (int64_t)w * h, total = n * records;
    if ((total + NT - 1) / NT > (int64_t)INT32_MAX) {
        set_error("%s: %d records of %d x %d are too many for one launch", who, records, w, h);
        return FOTO_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(mo_mu);
    int device = 0;
    MotionDev* md = nullptr;
    FOTO_TRY(motion_dev(&device, &md));
    const size_t bytes = (size_t)total * (layout == 0 ? 3 : 2) * dtype_bytes(dtype), mbytes = (size_t)count * 9 * 8;
    FOTO_TRY(dev_ptr_check(models, mbytes, device, who, "models"));
    FOTO_TRY(dev_ptr_check(out, bytes, device, who, "out"));
    if (fl) FOTO_TRY(dev_ptr_check(fl->data, bytes, device, who, "flow data"));
    if (overlaps(out, bytes, models, mbytes) || (fl && overlaps(out, bytes, fl->data, bytes))) {
        set_error("%s: out may not overlap an input", who);
        return FOTO_ERR_ARG;
    }
    hipStream_t s = md->s;
    FOTO_TRY(md->link.enter((hipStream_t)stream, s));
    const int mstride = count == 1 ? 0 : 9;
    if (dtype == FOTO_F32) field_launch<float>(fl != nullptr, fl ? fl->data : nullptr, models, mstride, w, n, total, layout, out, s);
    else field_launch<double>(fl != nullptr, fl ? fl->data : nullptr, models, mstride, w, n, total, layout, out, s);
    const hipError_t e = hipGetLastError();
    const int rl = md->link.leave(s, (hipStream_t)stream);
    FOTO_HIP_CHECK(e);
    return rl;
}

}  // namespace
}  // namespace foto

using namespace foto;

extern "C" {

int foto_motion_opts_default(foto_motion_opts* o) {
    if (!o) { set_error("foto_motion_opts_default: null argument"); return FOTO_ERR_ARG; }
    o->model = -1;
    o->rounds = 3;
    o->min_inliers = 0;
    o->reserved = 0;
    o->threshold = 1.0;
    return 0;
}

int foto_motion_fit_dev(const void* pts, int pts_dtype, const void* disp, int disp_dtype,
                        const unsigned char* status_or_null, int64_t M, int w, int h, const foto_motion_opts* opts,
                        const uint32_t* samples, int H, double* model, unsigned char* inliers, int64_t* info,
                        double* rms, void* stream) {
    static const char* const who = "foto_motion_fit_dev";
    if (!pts || !disp) { set_error("%s: null argument", who); return FOTO_ERR_ARG; }
    FOTO_TRY(fit_args_check(M, w, h, opts, samples, H, model, inliers, info, rms, who));
    FOTO_TRY(track_dtype_check(pts, pts_dtype, who, "pts"));
    FOTO_TRY(track_dtype_check(disp, disp_dtype, who, "disp"));
    MoSrc S{};
    S.pts = pts;
    S.disp = disp;
    S.status = status_or_null;
    S.pts_dtype = pts_dtype;
    S.disp_dtype = disp_dtype;
    const FitIn in[3] = {{pts, (size_t)M * 2 * dtype_bytes(pts_dtype), "pts"},
                         {disp, (size_t)M * 2 * dtype_bytes(disp_dtype), "disp"},
                         {status_or_null, (size_t)M, "status"}};
    return fit_run(S, M, w, h, *opts, samples, H, in, status_or_null ? 3 : 2, model, inliers, info, rms, stream, who);
}

int foto_motion_fit_flow_dev(const foto_flow* fl, int record, int w, int h, int stride,
                             const unsigned char* mask_or_null, const foto_motion_opts* opts, const uint32_t* samples,
                             int H, double* model, unsigned char* inliers, int64_t* info, double* rms, void* stream) {
    static const char* const who = "foto_motion_fit_flow_dev";
    FOTO_TRY(flow_check(fl, w, h, who));
    if (record < 0 || record >= fl->records) {
        set_error("%s: record = %d is outside the buffer's %d", who, record, fl->records);
        return FOTO_ERR_ARG;
    }
    if (stride < 1) { set_error("%s: stride = %d must be >= 1", who, stride); return FOTO_ERR_ARG; }
    if (w < 2 || h < 2) { set_error("%s: w = %d, h = %d: both must be >= 2", who, w, h); return FOTO_ERR_ARG; }
    const int lw = (w - 1) / stride + 1, lh = (h - 1) / stride + 1;
    const int64_t M = (int64_t)lw * lh;
    FOTO_TRY(fit_args_check(M, w, h, opts, samples, H, model, inliers, info, rms, who));
    const int64_t n = (int64_t)w * h;
    MoSrc S{};
    S.flow = (const char*)fl->data + (size_t)record * (fl->layout == 0 ? 3 : 2) * (size_t)n * dtype_bytes(fl->dtype);
    S.mask = mask_or_null;
    S.fdtype = fl->dtype;
    S.inter = fl->layout;
    S.w = w;
    S.stride = stride;
    S.lw = lw;
    S.plane = n;
    const FitIn in[2] = {{fl->data, flow_bytes(fl, w, h), "flow data"}, {mask_or_null, (size_t)n, "mask"}};
    return fit_run(S, M, w, h, *opts, samples, H, in, mask_or_null ? 2 : 1, model, inliers, info, rms, stream, who);
}

int foto_motion_field_dev(const double* models, int count, int w, int h, void* out, int dtype, int layout,
                          void* stream) {
    static const char* const who = "foto_motion_field_dev";
    if (!models || !out) { set_error("%s: null argument", who); return FOTO_ERR_ARG; }
    if (count < 1) { set_error("%s: count = %d must be >= 1", who, count); return FOTO_ERR_ARG; }
    FOTO_TRY(image_size_check(w, h, 1, who));
    if (dtype != FOTO_F32 && dtype != FOTO_F64) { set_error("%s: dtype %d is not FOTO_F32 / FOTO_F64", who, dtype); return FOTO_ERR_ARG; }
    if (layout != 0 && layout != 1) { set_error("%s: layout %d is not 0 / 1", who, layout); return FOTO_ERR_ARG; }
    if ((uintptr_t)models % 8 != 0 || (uintptr_t)out % dtype_bytes(dtype) != 0) {
        set_error("%s: models / out is not aligned to its element", who);
        return FOTO_ERR_ARG;
    }
    return field_run(nullptr, models, count, count, w, h, out, dtype, layout, stream, who);
}

int foto_motion_residual_dev(const foto_flow* fl, const double* models, int count, int w, int h, void* out,
                             void* stream) {
    static const char* const who = "foto_motion_residual_dev";
    FOTO_TRY(flow_check(fl, w, h, who));
    if (!models || !out) { set_error("%s: null argument", who); return FOTO_ERR_ARG; }
    if (count != 1 && count != fl->records) {
        set_error("%s: count = %d models for %d records: 1 or one per record", who, count, fl->records);
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(image_size_check(w, h, 1, who));
    if ((uintptr_t)models % 8 != 0 || (uintptr_t)out % dtype_bytes(fl->dtype) != 0) {
        set_error("%s: models / out is not aligned to its element", who);
        return FOTO_ERR_ARG;
    }
    return field_run(fl, models, count, fl->records, w, h, out, fl->dtype, fl->layout, stream, who);
}

}  // extern "C"

static_assert(sizeof(foto_motion_opts) == 24, "foto_motion_opts layout");
