// Device helpers shared between units: the spectral units' stores and loads (foto_spectral.hip,
// foto_dct.hip, foto_probe.hip), the fixed-order block sum (foto_dev.hip, foto_eval.hip), the
// trajectory step (k_traj, k_track: foto_kernels.hip; k_maps, k_interp: foto_interp.hip), the
// backward warp (k_warp: foto_eval.hip, k_render_warp: foto_render.hip) and the clamped bilinear
// sample (the pyramid: foto_gn_pyr.hip; k_interp).  Outputs that are documented as bit-identical
// to each other are so because they run the one definition here.  The sums across blocks and
// the wave primitives under them are shared the same way in foto_reduce.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace foto {

typedef double dbl4 __attribute__((ext_vector_type(4)));
typedef double dbl2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Write-through 16-B stores (buffer_store_dwordx4 ... sc1): the line leaves the XCD's L2 at
// once instead of staying dirty there.  A streaming kernel that ends with its L2s full of
// dirty lines pays their write-back at the kernel boundary (MI355X_MICROARCH.md price list,
// row "boundary": + B / 6 TB/s for B dirty bytes, up to 32 MiB here).  The resource covers
// [base, base + 2^31 B); offsets are in bytes.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wt_rsrc(double* base) {
    return __builtin_amdgcn_make_buffer_rsrc(base, 0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ void st_wt16(__amdgpu_buffer_rsrc_t rs, int off_bytes, dbl2 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, off_bytes, 0, 16 /* sc1 */);
}

// Loads of a pass's input that is dead after the pass (the DCT chain's intermediates, x^, b^
// in the x^ kernel) are non-temporal: the lines leave the caches first, so the pass's output
// and the next kernel's inputs keep them (A/B against plain loads: DESIGN.md 3.5).
template <class V>
__device__ __forceinline__ V ld_dead(const V* p) {
    return __builtin_nontemporal_load(p);
}

// Fixed-order block sum of Q quantities per thread over N threads (N a power of two): v[q] of
// thread t goes to sh[q * N + t], a halving tree leaves the totals in sh[q * N].  The order
// depends on N alone, so a sum keeps its bits from launch to launch.
template <int N, int Q>
__device__ __forceinline__ void block_tree_sum(const double (&v)[Q], double* sh /* Q * N */) {
#pragma unroll
    for (int q = 0; q < Q; ++q) sh[q * N + threadIdx.x] = v[q];
    __syncthreads();
    for (int st = N / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st)
#pragma unroll
            for (int q = 0; q < Q; ++q) sh[q * N + threadIdx.x] += sh[q * N + threadIdx.x + st];
        __syncthreads();
    }
}

// ----------------------------------------------------------------------------- trajectory step
__device__ __forceinline__ int trunc_clamp(double v, int hi) {
    double t = trunc(v);               // int() truncates toward zero
    if (!(t >= 0.0)) t = 0.0;          // also maps NaN to 0
    if (t > (double)hi) t = (double)hi;
    return (int)t;
}

// One step of reconstructTrajectory (utils.py:44-99): (x, y) += the bilinear sample at (x, y) of
// un = G_x P, vn = G_y P (central differences, bc 'N': zero on the edge columns / rows) of the
// Ny x Nx plane P, Nx, Ny >= 2.  The 12 values of P it needs (the 4 x 4 neighbourhood of
// (tx, ty) without its corners) are loaded together from indices clamped into the plane, and
// the edge zeros selected afterwards: tx in [0, Nx-2] and ty in [0, Ny-2] for every x, y
// (trunc_clamp maps NaN to 0 and clamps +-inf), so every load is inside the plane whatever the
// position -- a non-finite position gives a non-finite position and nothing else.
// traj_vel is the sample alone, (vx, vy) = V(x, y): the step adds it, the inverse step of the
// maps (inv_step below) subtracts a fraction of it.
__device__ __forceinline__ void traj_vel(const double* __restrict__ P, int Nx, int Ny, double x, double y, double& vx,
                                         double& vy) {
    const int tx = trunc_clamp(x, Nx - 2), ty = trunc_clamp(y, Ny - 2);
    const int xm = tx > 0 ? tx - 1 : 0, xp = tx + 2 < Nx ? tx + 2 : Nx - 1;
    const int ym = ty > 0 ? ty - 1 : 0, yp = ty + 2 < Ny ? ty + 2 : Ny - 1;
    const double* r0 = P + (int64_t)ty * Nx;
    const double* r1 = r0 + Nx;
    const double* rm = P + (int64_t)ym * Nx;
    const double* rp = P + (int64_t)yp * Nx;
    // the 12 loads, ahead of their first use
    const double a0 = r0[xm], b0 = r0[tx], c0 = r0[tx + 1], d0 = r0[xp];
    const double a1 = r1[xm], b1 = r1[tx], c1 = r1[tx + 1], d1 = r1[xp];
    const double bm = rm[tx], cm = rm[tx + 1];
    const double bp = rp[tx], cp = rp[tx + 1];
    const double dX = x - tx, dY = y - ty;
    const double w1 = (1 - dY) * (1 - dX), w2 = dX * (1 - dY), w3 = dY * dX, w4 = (1 - dX) * dY;
    const bool xl = tx == 0, xr = tx + 1 == Nx - 1;   // un is 0 on columns 0 and Nx-1
    const bool yl = ty == 0, yr = ty + 1 == Ny - 1;   // vn is 0 on rows 0 and Ny-1
    const double u00 = xl ? 0.0 : 0.5 * (c0 - a0), u01 = xr ? 0.0 : 0.5 * (d0 - b0);
    const double u11 = xr ? 0.0 : 0.5 * (d1 - b1), u10 = xl ? 0.0 : 0.5 * (c1 - a1);
    const double v00 = yl ? 0.0 : 0.5 * (b1 - bm), v01 = yl ? 0.0 : 0.5 * (c1 - cm);
    const double v11 = yr ? 0.0 : 0.5 * (cp - c0), v10 = yr ? 0.0 : 0.5 * (bp - b0);
    vx = w1 * u00 + w2 * u01 + w3 * u11 + w4 * u10;
    vy = w1 * v00 + w2 * v01 + w3 * v11 + w4 * v10;
}

__device__ __forceinline__ void traj_step(const double* __restrict__ P, int Nx, int Ny, double& x, double& y) {
    double vx, vy;
    traj_vel(P, Nx, Ny, x, y, vx, vy);
    x += vx;
    y += vy;
}

// The inverse of a (fraction theta of a) step: the z with z + theta V(z) = (px, py), by `iters`
// rounds of z <- p - theta V(z) from z = p.  A fixed count and no convergence test: the result is
// a function of the inputs alone, and restatable.  It converges where theta V is a contraction
// (DESIGN.md 3.12 has the measured rates); elsewhere it is still inside every bound above.
__device__ __forceinline__ void inv_step(const double* __restrict__ P, int Nx, int Ny, double theta, int iters,
                                         double& x, double& y) {
    const double px = x, py = y;
    for (int k = 0; k < iters; ++k) {
        double vx, vy;
        traj_vel(P, Nx, Ny, x, y, vx, vy);
        x = px - theta * vx;
        y = py - theta * vy;
    }
}

// Middlebury's unknown-flow marker (UNKNOWN_FLOW_THRESH of its flowIO): such a pixel is black in
// the colour code (foto_render.hip) and not evaluated by the scorer (foto_score.hip)
constexpr double UNKNOWN_FLOW_THRESH = 1e9;
__device__ __forceinline__ bool flow_unknown(double u, double v) {
    return fabs(u) > UNKNOWN_FLOW_THRESH || fabs(v) > UNKNOWN_FLOW_THRESH || u != u || v != v;
}

// ----------------------------------------------------------------------------- backward warp
// One output pixel (row i, column j) of utils.apply_opticalflow (utils.py:186-248) in a w x h
// frame, displacement (u, v): the four bilinear weights and the clamped taps, rows a, a1 and
// columns b, b1.  A NaN displacement gives NaN weights, so a NaN pixel; its taps stay in the frame.
struct WarpTaps {
    double w1, w2, w3, w4;
    int64_t a, b, a1, b1;
};

__device__ __forceinline__ WarpTaps warp_taps(int i, int j, double u, double v, int w, int h) {
    double ti = (double)i - v, tj = (double)j - u;
    const double dI = ti - trunc(ti), dJ = tj - trunc(tj);
    WarpTaps T;
    T.w1 = (1 - dI) * (1 - dJ);
    T.w2 = dJ * (1 - dI);
    T.w3 = dI * dJ;
    T.w4 = (1 - dJ) * dI;
    if (ti >= h) ti = h - 1;
    if (tj >= w) tj = w - 1;
    if (ti < 0) ti = 0;
    if (tj < 0) tj = 0;
    if (ti != ti) ti = 0;
    if (tj != tj) tj = 0;
    T.a = (int64_t)ti;
    T.b = (int64_t)tj;
    T.a1 = (T.a < h - 1) ? T.a + 1 : T.a;
    T.b1 = (T.b < w - 1) ? T.b + 1 : T.b;
    return T;
}

// w1 F(a, b) + w2 F(a, b1) + w3 F(a1, b1) + w4 F(a1, b) in the reference's order; F = g f with
// g = 1 + m at the tap, or f alone
__device__ __forceinline__ double warp_sum(const WarpTaps& T, double f1, double f2, double f3, double f4) {
    double x = T.w1 * f1;
    x = x + T.w2 * f2;
    x = x + T.w3 * f3;
    x = x + T.w4 * f4;
    return x;
}
__device__ __forceinline__ double warp_sum(const WarpTaps& T, double g1, double g2, double g3, double g4, double f1,
                                           double f2, double f3, double f4) {
    return warp_sum(T, g1 * f1, g2 * f2, g3 * f3, g4 * f4);
}

// ----------------------------------------------------------------------------- clamped sample
// S(f; x, y): bilinear on a w x h field (w, h >= 2), the coordinate clamped into the frame; a NaN
// coordinate gives NaN, read from in-frame taps (foto_warp's rule).  The cell and the two
// fractions depend on the coordinate alone: a caller with several fields (the channels of
// k_interp) computes them once.
struct SampleTaps {
    int i0, j0;      // the cell's upper-left tap, i0 in [0, w-2], j0 in [0, h-2]
    double ax, ay;
    bool bad;        // a NaN coordinate
};

__device__ __forceinline__ SampleTaps sample_taps(int w, int h, double x, double y) {
    SampleTaps T;
    T.bad = isnan(x) || isnan(y);
    const double xc = T.bad ? 0.0 : fmin(fmax(x, 0.0), (double)(w - 1));
    const double yc = T.bad ? 0.0 : fmin(fmax(y, 0.0), (double)(h - 1));
    T.i0 = min((int)floor(xc), w - 2);
    T.j0 = min((int)floor(yc), h - 2);
    T.ax = xc - (double)T.i0;
    T.ay = yc - (double)T.j0;
    return T;
}

// f00 = f(j0, i0), f01 = f(j0, i0 + 1), f10 = f(j0 + 1, i0), f11 = f(j0 + 1, i0 + 1)
__device__ __forceinline__ double sample_sum(const SampleTaps& T, double f00, double f01, double f10, double f11) {
    const double t = (1.0 - T.ax) * f00 + T.ax * f01;
    const double b = (1.0 - T.ax) * f10 + T.ax * f11;
    const double v = (1.0 - T.ay) * t + T.ay * b;
    return T.bad ? NAN : v;
}

__device__ __forceinline__ double pyr_sample(const double* __restrict__ f, int w, int h, double x, double y) {
    const SampleTaps T = sample_taps(w, h, x, y);
    const double* r0 = f + (int64_t)T.j0 * w + T.i0;
    const double* r1 = r0 + w;
    return sample_sum(T, r0[0], r0[1], r1[0], r1[1]);
}

// ----------------------------------------------------------------------------- central differences
// Gx f and Gy f at (i, j): central differences, zero in the first and last column / row (bc N).
// Both taps are loaded from clamped indices and the edge zero is selected afterwards.  Shared by
// the TV-L1 coefficients (foto_tvl1.hip) and by the corner detector and the Lucas-Kanade windows
// (foto_sparse.hip): a gradient has the same bits wherever it is formed.
__device__ __forceinline__ double cdiff_x(const double* __restrict__ f, int w, int i, int64_t row) {
    const double a = f[row + max(i - 1, 0)], b = f[row + min(i + 1, w - 1)];
    return (i == 0 || i == w - 1) ? 0.0 : 0.5 * (b - a);
}
__device__ __forceinline__ double cdiff_y(const double* __restrict__ f, int w, int h, int i, int j) {
    const double a = f[(int64_t)max(j - 1, 0) * w + i], b = f[(int64_t)min(j + 1, h - 1) * w + i];
    return (j == 0 || j == h - 1) ? 0.0 : 0.5 * (b - a);
}

}  // namespace foto
