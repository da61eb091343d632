// libfoto: entropic optimal transport on the pixel grid for gfx950 -- convolutional Sinkhorn
// (Cuturi 2013; Solomon et al. 2015) with the cost |x - y|^2 / 2, whose Gibbs kernel is a separable
// Gaussian truncated to a (2 R + 1)^2 window; the plan's barycentric projection as a flow and its
// cost as a W2.  include/foto.h has the arithmetic; tests/sinkhorn_ref.py restates it in numpy and
// the device is held to it bit for bit (-ffp-contract=off, every tap sum sequential in ascending d).
//
//   k_sk_prepare   the frames cleaned (negative / non-finite -> 0, counted), a = 0, b = 1, the masses
//   k_sk_row       a half-iteration, the default form: the row pass of the whole image into a scratch
//   k_sk_coldiv    image, then column pass + division (the faster of the two forms: DESIGN.md 3.20)
//   k_sk_half      the fused form (FOTO_SK_FUSED=1), one launch: a block stages its SK_TX x SK_TY tile
//                  of the scaling with a halo of R into LDS, runs the row pass for its SK_TY + 2 R rows
//                  into LDS, the column pass out of LDS, divides and stores.  The same bits: a tap sum
//                  has one order
//   k_sk_flow      s = conv(k, k, z), conv(k1, k, z), conv(k, k1, z) from two row passes of one staged
//                  tile; u, v, valid
//   k_sk_terms     per pixel |a s - mu|, a (conv(k2, k, b) + conv(k, k2, b)), unreachable
//   k_sk_sum       their fixed-order sums (foto_reduce.h) and the 8-number record
// The tables come from the host (foto.sinkhorn.tables): the device never evaluates exp.  Every count
// is fixed; nothing waits for the host.  The tap weights are read at wave-uniform addresses.
#include <cmath>
#include <memory>

#include "foto_devmem.h"
#include "foto_devutil.h"
#include "foto_reduce.h"

namespace foto {
namespace {

constexpr int SK_TX = FOTO_SINKHORN_TILE_W, SK_TY = FOTO_SINKHORN_TILE_H, SK_RMAX = FOTO_SINKHORN_MAX_RADIUS;
constexpr int SK_NW = NT / 64;            // waves per block
constexpr int SK_PER = SK_TY / SK_NW;     // consecutive output rows per thread in the column pass
static_assert(SK_TX == 64, "a wave is one row of the tile");
static_assert(SK_TY % SK_NW == 0, "whole rows per wave");

// the LDS image of a block: in[rows][pitch] (the scaling with its halo), t[rows][SK_TX] (the row pass)
__host__ __device__ constexpr int sk_rows_of(int R) { return SK_TY + 2 * R; }
__host__ __device__ constexpr int sk_pitch_of(int R) { return SK_TX + 2 * R; }
constexpr size_t sk_lds_bytes(int R) {
    return (size_t)sk_rows_of(R) * (sk_pitch_of(R) + SK_TX) * sizeof(double);
}
static_assert(sk_lds_bytes(SK_RMAX) <= 160 * 1024, "a block's image fits the CU's LDS at the largest radius");

struct SkTile {
    int x0, y0, R, rows, pitch;
    double* in;
    double* t;
};

__device__ __forceinline__ SkTile sk_tile(int R, double* smem) {
    SkTile T;
    T.x0 = blockIdx.x * SK_TX;
    T.y0 = blockIdx.y * SK_TY;
    T.R = R;
    T.rows = sk_rows_of(R);
    T.pitch = sk_pitch_of(R);
    T.in = smem;
    T.t = smem + T.rows * T.pitch;
    return T;
}

// in[r][c] = z(y0 - R + r, x0 - R + c), 0.0 outside the frame: every load is inside it
__device__ __forceinline__ void sk_stage(const SkTile& T, const double* __restrict__ z, int w, int h) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int r = wv; r < T.rows; r += SK_NW) {
        const int y = T.y0 - T.R + r;
        const bool yin = y >= 0 && y < h;
        for (int c = lane; c < T.pitch; c += 64) {
            const int x = T.x0 - T.R + c;
            const bool in = yin && x >= 0 && x < w;
            T.in[r * T.pitch + c] = in ? z[(int64_t)y * w + x] : 0.0;
        }
    }
}

// t[r][x] = 0.0 + p[0] in[r][x] + p[1] in[r][x + 1] + .. + p[2 R] in[r][x + 2 R], in that order; a wave
// works on four rows at once (four independent chains)
__device__ __forceinline__ void sk_rows(const SkTile& T, const double* __restrict__ p) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int r0 = wv; r0 < T.rows; r0 += 4 * SK_NW) {
        const double* row[4];
        double acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            row[q] = T.in + min(r0 + q * SK_NW, T.rows - 1) * T.pitch + lane;
            acc[q] = 0.0;
        }
        for (int d = 0; d <= 2 * T.R; ++d) {
            const double pd = p[d];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = acc[q] + pd * row[q][d];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (r0 + q * SK_NW < T.rows) T.t[(r0 + q * SK_NW) * SK_TX + lane] = acc[q];
    }
}

// acc[i][k] = 0.0 + q_i[0] t[yb + k][x] + .. + q_i[2 R] t[yb + k + 2 R][x] for the thread's SK_PER
// consecutive rows yb + k (yb = wave * SK_PER) and NQ tables: one LDS read per row of t feeds
// every chain it belongs to, each chain in ascending d
template <int NQ>
__device__ __forceinline__ void sk_cols(const SkTile& T, const double* const (&q)[NQ], double (&acc)[NQ][SK_PER]) {
    const int lane = threadIdx.x & 63, yb = (threadIdx.x >> 6) * SK_PER;
#pragma unroll
    for (int i = 0; i < NQ; ++i)
#pragma unroll
        for (int k = 0; k < SK_PER; ++k) acc[i][k] = 0.0;
    const int last = SK_PER - 1 + 2 * T.R;
    for (int s = 0; s <= last; ++s) {
        const double val = T.t[(yb + s) * SK_TX + lane];
#pragma unroll
        for (int k = 0; k < SK_PER; ++k) {
            const int d = s - k;
            if (d >= 0 && d <= 2 * T.R) {   // (uniform)
#pragma unroll
                for (int i = 0; i < NQ; ++i) acc[i][k] = acc[i][k] + q[i][d] * val;
            }
        }
    }
}

__device__ __forceinline__ double sk_div(double m, double s) { return (m > 0.0 && s > 0.0) ? m / s : 0.0; }

__global__ __launch_bounds__(NT) void k_sk_half(int w, int h, int R, const double* __restrict__ tab,
                                                const double* __restrict__ z, const double* __restrict__ marg,
                                                double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char sk_smem[];
    const SkTile T = sk_tile(R, (double*)sk_smem);
    sk_stage(T, z, w, h);
    __syncthreads();
    sk_rows(T, tab);
    __syncthreads();
    const double* const q[1] = {tab};
    double acc[1][SK_PER];
    sk_cols<1>(T, q, acc);
    const int x = T.x0 + (threadIdx.x & 63), yb = T.y0 + (threadIdx.x >> 6) * SK_PER;
    if (x >= w) return;
#pragma unroll
    for (int k = 0; k < SK_PER; ++k) {
        if (yb + k >= h) break;
        const int64_t i = (int64_t)(yb + k) * w + x;
        out[i] = sk_div(marg[i], acc[0][k]);
    }
}

// tab: [3][2 R + 1] = k, k1, k2 at d = -R .. R
__global__ __launch_bounds__(NT) void k_sk_flow(int w, int h, int R, const double* __restrict__ tab,
                                                const double* __restrict__ z, const double* __restrict__ marg,
                                                double* __restrict__ U, double* __restrict__ V,
                                                unsigned char* __restrict__ valid) {
    extern __shared__ __attribute__((aligned(16))) char sk_smem[];
    const SkTile T = sk_tile(R, (double*)sk_smem);
    const double* const tk = tab;
    const double* const tk1 = tab + (2 * R + 1);
    sk_stage(T, z, w, h);
    __syncthreads();
    sk_rows(T, tk);
    __syncthreads();
    const double* const q2[2] = {tk, tk1};
    double sv[2][SK_PER];   // s and the numerator of v
    sk_cols<2>(T, q2, sv);
    __syncthreads();
    sk_rows(T, tk1);
    __syncthreads();
    const double* const q1[1] = {tk};
    double un[1][SK_PER];
    sk_cols<1>(T, q1, un);
    const int x = T.x0 + (threadIdx.x & 63), yb = T.y0 + (threadIdx.x >> 6) * SK_PER;
    if (x >= w) return;
#pragma unroll
    for (int k = 0; k < SK_PER; ++k) {
        if (yb + k >= h) break;
        const int64_t i = (int64_t)(yb + k) * w + x;
        const double s = sv[0][k];
        const bool ok = marg[i] > 0.0 && s > 0.0;
        U[i] = ok ? un[0][k] / s : 0.0;
        V[i] = ok ? sv[1][k] / s : 0.0;
        if (valid) valid[i] = ok ? 1 : 0;
    }
}

__global__ __launch_bounds__(NT) void k_sk_terms(int w, int h, int R, const double* __restrict__ tab,
                                                 const double* __restrict__ a, const double* __restrict__ b,
                                                 const double* __restrict__ mu, double* __restrict__ e_err,
                                                 double* __restrict__ e_cost, double* __restrict__ e_unr) {
    extern __shared__ __attribute__((aligned(16))) char sk_smem[];
    const SkTile T = sk_tile(R, (double*)sk_smem);
    const double* const tk = tab;
    const double* const tk2 = tab + 2 * (2 * R + 1);
    sk_stage(T, b, w, h);
    __syncthreads();
    sk_rows(T, tk);
    __syncthreads();
    const double* const q2[2] = {tk, tk2};
    double sc[2][SK_PER];   // s and conv(k, k2, b)
    sk_cols<2>(T, q2, sc);
    __syncthreads();
    sk_rows(T, tk2);
    __syncthreads();
    const double* const q1[1] = {tk};
    double c1[1][SK_PER];   // conv(k2, k, b)
    sk_cols<1>(T, q1, c1);
    const int x = T.x0 + (threadIdx.x & 63), yb = T.y0 + (threadIdx.x >> 6) * SK_PER;
    if (x >= w) return;
#pragma unroll
    for (int k = 0; k < SK_PER; ++k) {
        if (yb + k >= h) break;
        const int64_t i = (int64_t)(yb + k) * w + x;
        const double ai = a[i], mi = mu[i], s = sc[0][k];
        e_err[i] = fabs(ai * s - mi);
        e_cost[i] = ai * (c1[0][k] + sc[1][k]);
        e_unr[i] = (mi > 0.0 && s == 0.0) ? 1.0 : 0.0;
    }
}

// ----------------------------------------------------------------------------- the two-pass form

__global__ __launch_bounds__(NT) void k_sk_row(int w, int64_t n, int R, const double* __restrict__ p,
                                               const double* __restrict__ z, double* __restrict__ t) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= n) return;
    const int64_t row = idx / w;
    const int i = (int)(idx - row * w);
    double acc = 0.0;
    for (int d = 0; d <= 2 * R; ++d) {
        const int x = i + d - R;
        const double v = (x >= 0 && x < w) ? z[row * w + x] : 0.0;
        acc = acc + p[d] * v;
    }
    t[idx] = acc;
}

__global__ __launch_bounds__(NT) void k_sk_coldiv(int w, int h, int64_t n, int R, const double* __restrict__ q,
                                                  const double* __restrict__ t, const double* __restrict__ marg,
                                                  double* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= n) return;
    const int j = (int)(idx / w);
    const int i = (int)(idx - (int64_t)j * w);
    double acc = 0.0;
    for (int d = 0; d <= 2 * R; ++d) {
        const int y = j + d - R;
        const double v = (y >= 0 && y < h) ? t[(int64_t)y * w + i] : 0.0;
        acc = acc + q[d] * v;
    }
    out[idx] = sk_div(marg[idx], acc);
}

// ----------------------------------------------------------------------------- frames and sums

// rec: the context's record (include/foto.h); this kernel sets the masses and `bad`
__global__ __launch_bounds__(NT) void k_sk_prepare(int64_t n, const double* __restrict__ r0,
                                                   const double* __restrict__ r1, double* __restrict__ mu,
                                                   double* __restrict__ nu, double* __restrict__ a,
                                                   double* __restrict__ b, RedBuf rb, double* __restrict__ rec) {
    double v[3] = {0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const double x0 = r0[i], x1 = r1[i];
        const bool ok0 = isfinite(x0) && x0 >= 0.0, ok1 = isfinite(x1) && x1 >= 0.0;
        const double m0 = ok0 ? x0 : 0.0, m1 = ok1 ? x1 : 0.0;
        mu[i] = m0;
        nu[i] = m1;
        a[i] = 0.0;
        b[i] = 1.0;
        v[0] += m0;
        v[1] += m1;
        v[2] += (ok0 ? 0.0 : 1.0) + (ok1 ? 0.0 : 1.0);
    }
    double tot[3];
    if (grid_reduce_last<3>(v, rb, tot) && threadIdx.x == 0) {
        rec[0] = tot[0];
        rec[1] = tot[1];
        rec[4] = tot[2];
    }
}

__global__ __launch_bounds__(NT) void k_sk_sum(int64_t n, const double* __restrict__ e_err,
                                               const double* __restrict__ e_cost, const double* __restrict__ e_unr,
                                               RedBuf rb, const double* __restrict__ rec, double iters,
                                               double* __restrict__ out8) {
    double v[3] = {0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        v[0] += e_err[i];
        v[1] += e_cost[i];
        v[2] += e_unr[i];
    }
    double tot[3];
    if (grid_reduce_last<3>(v, rb, tot) && threadIdx.x == 0) {
        out8[0] = rec[0];
        out8[1] = rec[1];
        out8[2] = tot[0];
        out8[3] = tot[1];
        out8[4] = rec[4];
        out8[5] = tot[2];
        out8[6] = iters;
        out8[7] = 0.0;
    }
}

}  // namespace
}  // namespace foto

using namespace foto;

// ============================================================================ the context (host)

struct foto_sinkhorn {
    int w = 0, h = 0, device = 0, R = 0;
    double eps = 0.0;
    bool fused = false;        // Tuning::sk_fused, read once at create
    bool have_frames = false;
    int iters = 0;
    int64_t n = 0;
    hipStream_t s = nullptr;
    DevArena mem;
    double *mu = nullptr, *nu = nullptr, *a = nullptr, *b = nullptr;
    double *p0 = nullptr, *p1 = nullptr, *p2 = nullptr;   // planes: the raw frames, then U, V / the terms; t of the two-pass form
    double* zero = nullptr;    // the m plane of a flow record
    double* tab = nullptr;     // [3][2 R + 1]
    double* rec = nullptr;     // [8]
    RedBuf rb{};
    int sum_blocks = 1;
    StreamLink link;

    ~foto_sinkhorn() {
        if (s) (void)hipStreamSynchronize(s);
        mem.clear();
        stream_release(s);
    }
};

namespace foto {
namespace {

int sk_ctx_check(const foto_sinkhorn* c, const char* who, bool frames) {
    if (!c) { set_error("%s: null context", who); return FOTO_ERR_ARG; }
    if (frames && !c->have_frames) { set_error("%s: no frames yet (foto_sinkhorn_set_frames_dev)", who); return FOTO_ERR_STATE; }
    return 0;
}

dim3 sk_grid(const foto_sinkhorn* c) {
    return dim3((unsigned)((c->w + SK_TX - 1) / SK_TX), (unsigned)((c->h + SK_TY - 1) / SK_TY));
}

// the raw frames are in p0, p1: clean them, reset the scalings and the count
int sk_prepare(foto_sinkhorn* c) {
    k_sk_prepare<<<c->sum_blocks, NT, 0, c->s>>>(c->n, c->p0, c->p1, c->mu, c->nu, c->a, c->b, c->rb, c->rec);
    FOTO_HIP_CHECK(hipGetLastError());
    c->iters = 0;
    c->have_frames = true;
    return 0;
}

int sk_half(foto_sinkhorn* c, const double* z, const double* marg, double* out) {
    if (c->fused) {
        k_sk_half<<<sk_grid(c), NT, sk_lds_bytes(c->R), c->s>>>(c->w, c->h, c->R, c->tab, z, marg, out);
    } else {
        const int nb = flat_blocks(c->n);
        k_sk_row<<<nb, NT, 0, c->s>>>(c->w, c->n, c->R, c->tab, z, c->p2);
        k_sk_coldiv<<<nb, NT, 0, c->s>>>(c->w, c->h, c->n, c->R, c->tab, c->p2, marg, out);
    }
    FOTO_HIP_CHECK(hipGetLastError());
    return 0;
}

int sk_iterate(foto_sinkhorn* c, int n) {
    for (int k = 0; k < n; ++k) {
        FOTO_TRY(sk_half(c, c->b, c->mu, c->a));
        FOTO_TRY(sk_half(c, c->a, c->nu, c->b));
    }
    c->iters += n;
    return 0;
}

// u, v into p0, p1
int sk_flow(foto_sinkhorn* c, int direction, unsigned char* valid) {
    const double* z = direction == 0 ? c->b : c->a;
    const double* marg = direction == 0 ? c->mu : c->nu;
    k_sk_flow<<<sk_grid(c), NT, sk_lds_bytes(c->R), c->s>>>(c->w, c->h, c->R, c->tab, z, marg, c->p0, c->p1, valid);
    FOTO_HIP_CHECK(hipGetLastError());
    return 0;
}

int sk_args_check(int w, int h, const foto_sinkhorn_opts& o, const double* tables, const char* who) {
    FOTO_TRY(image_size_check(w, h, 1, who));
    if (o.radius < 0 || o.radius > SK_RMAX) {
        set_error("%s: radius = %d is outside 0 .. %d", who, o.radius, SK_RMAX);
        return FOTO_ERR_ARG;
    }
    if (!std::isfinite(o.eps) || !(o.eps > 0)) { set_error("%s: eps = %g must be finite and > 0", who, o.eps); return FOTO_ERR_ARG; }
    if (!tables) { set_error("%s: null tables", who); return FOTO_ERR_ARG; }
    return 0;
}

}  // namespace
}  // namespace foto

extern "C" {

int foto_sinkhorn_opts_default(foto_sinkhorn_opts* o) {
    if (!o) { set_error("foto_sinkhorn_opts_default: null argument"); return FOTO_ERR_ARG; }
    o->radius = 16;
    o->per_launch_reserved = 0;
    o->eps = 2.0;
    return 0;
}

int foto_sinkhorn_create(int w, int h, const foto_sinkhorn_opts* opts, const double* tables, foto_sinkhorn** out) {
    static const char* const who = "foto_sinkhorn_create";
    if (!out) { set_error("%s: null argument", who); return FOTO_ERR_ARG; }
    foto_sinkhorn_opts o;
    (void)foto_sinkhorn_opts_default(&o);
    if (opts) o = *opts;
    FOTO_TRY(sk_args_check(w, h, o, tables, who));
    auto C = std::make_unique<foto_sinkhorn>();
    C->w = w; C->h = h; C->R = o.radius; C->eps = o.eps;
    C->n = (int64_t)w * h;
    C->fused = tuning_from_env().sk_fused;
    FOTO_HIP_CHECK(hipGetDevice(&C->device));
    FOTO_TRY(stream_acquire(&C->s));
    const size_t n = (size_t)C->n;
    const int R = C->R, L = 2 * R + 1;
    C->sum_blocks = capped_blocks(C->n, SUM_MAX_BLOCKS);
    double* q = nullptr;   // one block: eight planes, the record, the tables, the partial sums
    FOTO_TRY(C->mem.alloc_n(8 * n + 8 + 3 * (size_t)L + 3 * (size_t)C->sum_blocks, &q));
    C->mu = q; q += n;
    C->nu = q; q += n;
    C->a = q; q += n;
    C->b = q; q += n;
    C->p0 = q; q += n;
    C->p1 = q; q += n;
    C->p2 = q; q += n;
    C->zero = q; q += n;
    C->rec = q; q += 8;
    C->tab = q; q += 3 * (size_t)L;
    C->rb.partials = q;
    C->rb.cap = 3 * C->sum_blocks;
    FOTO_TRY(C->mem.alloc_n(1, &C->rb.ticket));
    // tab[i][R + d] = k[|d|], sign(d) k1[|d|], k2[|d|]
    std::vector<double> full(3 * (size_t)L);
    for (int d = -R; d <= R; ++d) {
        const int m = d < 0 ? -d : d;
        full[0 * L + R + d] = tables[0 * (R + 1) + m];
        full[1 * L + R + d] = d < 0 ? -tables[1 * (R + 1) + m] : tables[1 * (R + 1) + m];
        full[2 * L + R + d] = tables[2 * (R + 1) + m];
    }
    FOTO_HIP_CHECK(hipMemcpyAsync(C->tab, full.data(), full.size() * sizeof(double), hipMemcpyHostToDevice, C->s));
    FOTO_HIP_CHECK(hipMemsetAsync(C->zero, 0, n * sizeof(double), C->s));
    FOTO_HIP_CHECK(hipMemsetAsync(C->rec, 0, 8 * sizeof(double), C->s));
    FOTO_HIP_CHECK(hipMemsetAsync(C->rb.ticket, 0, sizeof(unsigned), C->s));
    FOTO_HIP_CHECK(hipStreamSynchronize(C->s));   // (`full` goes out of scope)
    // a block's LDS image is beyond the default dynamic limit at the larger radii; the attribute is
    // the function's, not the context's, so it is the size of the largest radius
    const int lds = (int)sk_lds_bytes(SK_RMAX);
    FOTO_HIP_CHECK(hipFuncSetAttribute((const void*)k_sk_half, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    FOTO_HIP_CHECK(hipFuncSetAttribute((const void*)k_sk_flow, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    FOTO_HIP_CHECK(hipFuncSetAttribute((const void*)k_sk_terms, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    *out = C.release();
    return 0;
}

void foto_sinkhorn_destroy(foto_sinkhorn* c) { delete c; }

int foto_sinkhorn_set_frames_dev(foto_sinkhorn* c, const foto_image* f0, const foto_image* f1, void* stream) {
    static const char* const who = "foto_sinkhorn_set_frames_dev";
    FOTO_TRY(sk_ctx_check(c, who, false));
    if (!f0 || !f1) { set_error("%s: null argument", who); return FOTO_ERR_ARG; }
    FOTO_TRY(image_dev_check(f0, c->w, c->h, c->device, "foto_sinkhorn_set_frames_dev (f0)"));
    FOTO_TRY(image_dev_check(f1, c->w, c->h, c->device, "foto_sinkhorn_set_frames_dev (f1)"));
    FOTO_TRY(c->link.enter((hipStream_t)stream, c->s));
    auto run = [&]() -> int {
        FOTO_HIP_CHECK(launch_ingest(*f0, c->w, c->h, c->p0, c->s));
        FOTO_HIP_CHECK(launch_ingest(*f1, c->w, c->h, c->p1, c->s));
        return sk_prepare(c);
    };
    const int rc = run();
    const int rl = c->link.leave(c->s, (hipStream_t)stream);
    return rc < 0 ? rc : rl;
}

int foto_sinkhorn_iterate_dev(foto_sinkhorn* c, int n, void* stream) {
    static const char* const who = "foto_sinkhorn_iterate_dev";
    FOTO_TRY(sk_ctx_check(c, who, true));
    if (n < 0) { set_error("%s: n = %d iterations must be >= 0", who, n); return FOTO_ERR_ARG; }
    FOTO_TRY(c->link.enter((hipStream_t)stream, c->s));
    const int rc = sk_iterate(c, n);
    const int rl = c->link.leave(c->s, (hipStream_t)stream);
    return rc < 0 ? rc : rl;
}

int foto_sinkhorn_flow_dev(foto_sinkhorn* c, int direction, void* out, int dtype, int layout,
                           unsigned char* valid_or_null, void* stream) {
    static const char* const who = "foto_sinkhorn_flow_dev";
    FOTO_TRY(sk_ctx_check(c, who, true));
    if (direction != 0 && direction != 1) { set_error("%s: direction %d is not 0 (forward) / 1 (backward)", who, direction); return FOTO_ERR_ARG; }
    if (!out) { set_error("%s: null argument", who); return FOTO_ERR_ARG; }
    FOTO_TRY(export_check(out, dtype, layout, c->n, c->device, who));
    if (valid_or_null) FOTO_TRY(dev_ptr_check(valid_or_null, (size_t)c->n, c->device, who, "valid"));
    FOTO_TRY(c->link.enter((hipStream_t)stream, c->s));
    auto run = [&]() -> int {
        FOTO_TRY(sk_flow(c, direction, valid_or_null));
        FOTO_HIP_CHECK(launch_export(c->n, c->p0, c->p1, c->zero, out, dtype, layout, c->s));
        return 0;
    };
    const int rc = run();
    const int rl = c->link.leave(c->s, (hipStream_t)stream);
    return rc < 0 ? rc : rl;
}

int foto_sinkhorn_info_dev(foto_sinkhorn* c, double* info8, void* stream) {
    static const char* const who = "foto_sinkhorn_info_dev";
    FOTO_TRY(sk_ctx_check(c, who, true));
    if (!info8) { set_error("%s: null argument", who); return FOTO_ERR_ARG; }
    if ((uintptr_t)info8 % 8 != 0) { set_error("%s: info8 is not aligned to 8 bytes", who); return FOTO_ERR_ARG; }
    FOTO_TRY(dev_ptr_check(info8, 8 * sizeof(double), c->device, who, "info8"));
    FOTO_TRY(c->link.enter((hipStream_t)stream, c->s));
    auto run = [&]() -> int {
        k_sk_terms<<<sk_grid(c), NT, sk_lds_bytes(c->R), c->s>>>(c->w, c->h, c->R, c->tab, c->a, c->b, c->mu, c->p0,
                                                               c->p1, c->p2);
        k_sk_sum<<<c->sum_blocks, NT, 0, c->s>>>(c->n, c->p0, c->p1, c->p2, c->rb, c->rec, (double)c->iters, info8);
        FOTO_HIP_CHECK(hipGetLastError());
        return 0;
    };
    const int rc = run();
    const int rl = c->link.leave(c->s, (hipStream_t)stream);
    return rc < 0 ? rc : rl;
}

int foto_sinkhorn_scalings_dev(foto_sinkhorn* c, double* a_out, double* b_out, void* stream) {
    static const char* const who = "foto_sinkhorn_scalings_dev";
    FOTO_TRY(sk_ctx_check(c, who, true));
    if (!a_out || !b_out) { set_error("%s: null argument", who); return FOTO_ERR_ARG; }
    const size_t bytes = (size_t)c->n * sizeof(double);
    FOTO_TRY(dev_ptr_check(a_out, bytes, c->device, who, "a_out"));
    FOTO_TRY(dev_ptr_check(b_out, bytes, c->device, who, "b_out"));
    if (overlaps(a_out, bytes, b_out, bytes)) { set_error("%s: a_out may not overlap b_out", who); return FOTO_ERR_ARG; }
    FOTO_TRY(c->link.enter((hipStream_t)stream, c->s));
    auto run = [&]() -> int {
        FOTO_HIP_CHECK(hipMemcpyAsync(a_out, c->a, bytes, hipMemcpyDeviceToDevice, c->s));
        FOTO_HIP_CHECK(hipMemcpyAsync(b_out, c->b, bytes, hipMemcpyDeviceToDevice, c->s));
        return 0;
    };
    const int rc = run();
    const int rl = c->link.leave(c->s, (hipStream_t)stream);
    return rc < 0 ? rc : rl;
}

int foto_sinkhorn_solve(foto_sinkhorn* c, const double* f0, const double* f1, int n, double* u, double* v, double* m) {
    static const char* const who = "foto_sinkhorn_solve";
    FOTO_TRY(sk_ctx_check(c, who, false));
    if (!f0 || !f1 || !u || !v || !m) { set_error("%s: null argument", who); return FOTO_ERR_ARG; }
    if (n < 0) { set_error("%s: n = %d iterations must be >= 0", who, n); return FOTO_ERR_ARG; }
    const size_t bytes = (size_t)c->n * sizeof(double);
    FOTO_HIP_CHECK(hipMemcpyAsync(c->p0, f0, bytes, hipMemcpyHostToDevice, c->s));
    FOTO_HIP_CHECK(hipMemcpyAsync(c->p1, f1, bytes, hipMemcpyHostToDevice, c->s));
    FOTO_TRY(sk_prepare(c));
    FOTO_TRY(sk_iterate(c, n));
    FOTO_TRY(sk_flow(c, 0, nullptr));
    FOTO_HIP_CHECK(hipMemcpyAsync(u, c->p0, bytes, hipMemcpyDeviceToHost, c->s));
    FOTO_HIP_CHECK(hipMemcpyAsync(v, c->p1, bytes, hipMemcpyDeviceToHost, c->s));
    FOTO_HIP_CHECK(hipMemcpyAsync(m, c->zero, bytes, hipMemcpyDeviceToHost, c->s));
    FOTO_HIP_CHECK(hipStreamSynchronize(c->s));
    return 0;
}

int foto_sinkhorn_solve_dev(foto_sinkhorn* c, const foto_image* f0, const foto_image* f1, int n, void* out, int dtype,
                            int layout, void* stream) {
    static const char* const who = "foto_sinkhorn_solve_dev";
    FOTO_TRY(sk_ctx_check(c, who, false));
    if (!f0 || !f1 || !out) { set_error("%s: null argument", who); return FOTO_ERR_ARG; }
    if (n < 0) { set_error("%s: n = %d iterations must be >= 0", who, n); return FOTO_ERR_ARG; }
    // device memory of the context's device, checked before anything is enqueued
    FOTO_TRY(image_dev_check(f0, c->w, c->h, c->device, "foto_sinkhorn_solve_dev (f0)"));
    FOTO_TRY(image_dev_check(f1, c->w, c->h, c->device, "foto_sinkhorn_solve_dev (f1)"));
    FOTO_TRY(export_check(out, dtype, layout, c->n, c->device, who));
    FOTO_TRY(c->link.enter((hipStream_t)stream, c->s));
    auto run = [&]() -> int {
        FOTO_HIP_CHECK(launch_ingest(*f0, c->w, c->h, c->p0, c->s));
        FOTO_HIP_CHECK(launch_ingest(*f1, c->w, c->h, c->p1, c->s));
        FOTO_TRY(sk_prepare(c));
        FOTO_TRY(sk_iterate(c, n));
        FOTO_TRY(sk_flow(c, 0, nullptr));
        FOTO_HIP_CHECK(launch_export(c->n, c->p0, c->p1, c->zero, out, dtype, layout, c->s));
        return 0;
    };
    const int rc = run();
    const int rl = c->link.leave(c->s, (hipStream_t)stream);
    return rc < 0 ? rc : rl;
}

}  // extern "C"

static_assert(sizeof(foto_sinkhorn_opts) == 16, "foto_sinkhorn_opts layout");
