// libfoto HIP kernels for the Benamou-Brenier (FOTO) hot path -- gfx950 / CDNA4.
//
// All arithmetic is float64 and is written in the operation order numpy/scipy use
// in the reference (the library is built with -ffp-contract=off: numpy and scipy's
// sparsetools never fuse a*b+c), so every per-voxel result is the reference's bit for
// bit; only global sums (dot products, crit sums) are reduced in a different -- fixed,
// deterministic -- order.
//
// Layout (reference operators.py:124-126): voxel k = n*Nx*Ny + j*Nx + i.  A shard owns
// planes [t0, t0+nloc); arrays carry one halo plane on each side (local l = -1, nloc).
//
// Hot kernels (stencil CG, one per CG iteration each):
//   k_cg_dir : p = r + beta p (fused), A p with a 64x4 LDS tile + 1-voxel halo, marching
//              along t with the t-neighbours in registers; p.Ap block partials.
//   k_cg_upd : x += alpha p, r -= alpha A p (A p recomputed from p: cheaper than storing
//              and re-reading q), r.r partials.
// Both finish with a last-block reduction (grid_reduce_last, foto_reduce.h: write-through
// partials + agent-scope ticket): no extra launch per dot product.
#include <type_traits>

#include "foto_devutil.h"
#include "foto_internal.h"
#include "foto_reduce.h"

namespace foto {

// ============================================================================ stencils

// One row of the space-time operator A = -r L_st + r eps I (benamou_brenier.py:202-203,
// operators.py:144-157) in scipy's CSR column order: t-1, y-1, x-1, diag, x+1, y+1, t+1.
// diag = fl(fl(r*c) + fl(r*eps)) with c = number of existing axis neighbours.
__device__ __forceinline__ double row_A(const Geo& g, int t, int y, int x, double c, double xm, double xp,
                                        double ym, double yp, double tm, double tp, double r, double reps) {
    const bool ht = t > 0, hT = t < g.Nt - 1, hy = y > 0, hY = y < g.Ny - 1, hx = x > 0, hX = x < g.Nx - 1;
    const double cnt = (double)((int)ht + (int)hT + (int)hy + (int)hY + (int)hx + (int)hX);
    const double mr = -r;
    const double dg = r * cnt + reps;
    double s = 0.0;
    if (ht) s += mr * tm;
    if (hy) s += mr * ym;
    if (hx) s += mr * xm;
    s += dg * c;
    if (hX) s += mr * xp;
    if (hY) s += mr * yp;
    if (hT) s += mr * tp;
    return s;
}

// L_st row (entries 1 off-diagonal, -c on the diagonal), same column order.
__device__ __forceinline__ double row_L(const Geo& g, int t, int y, int x, double c, double xm, double xp,
                                        double ym, double yp, double tm, double tp) {
    const bool ht = t > 0, hT = t < g.Nt - 1, hy = y > 0, hY = y < g.Ny - 1, hx = x > 0, hX = x < g.Nx - 1;
    const double cnt = (double)((int)ht + (int)hT + (int)hy + (int)hY + (int)hx + (int)hX);
    double s = 0.0;
    if (ht) s += tm;
    if (hy) s += ym;
    if (hx) s += xm;
    s += (-cnt) * c;
    if (hX) s += xp;
    if (hY) s += yp;
    if (hT) s += tp;
    return s;
}

// 2.5-D march over a 64 x TY xy tile: every thread owns one (x, y) column and walks the
// shard's planes, keeping planes t-1, t, t+1 of its column in registers.  The x/y
// neighbours of plane t come from a double-buffered LDS tile with a 1-voxel halo (one
// barrier per plane).  Loads run one plane ahead of use.
//   val(l, off)  -> field value at local plane l, in-plane offset off (in-domain only)
//   body(l, t, off, x, y, c, xm, xp, ym, yp, tm, tp)   for in-domain voxels
// Block -> tile for the column marches.  Workgroups are dispatched to the 8 XCDs round robin
// (block b on XCD b % 8), each with its own L2; give every XCD a contiguous range of row-major
// tiles instead, so the tile below a tile (ntx blocks later) is read through the same L2 and
// the y-halo rows hit there instead of being fetched from HBM again.
__device__ __forceinline__ int xcd_tile(int b) {
    constexpr int NXCD = 8;
    const int nb = gridDim.x, per = nb / NXCD, rem = nb % NXCD;
    const int xcd = b % NXCD, local = b / NXCD;
    return xcd * per + min(xcd, rem) + local;
}

template <class Val, class Body>
__device__ __forceinline__ void march(const Geo& g, int tile_blk, Val val, Body body) {
    const int tile = xcd_tile(tile_blk);
    constexpr int LW = TX + 2, LP = (TY + 2) * LW;
    __shared__ double lds[2 * LP];
    const int ntx = (g.Nx + TX - 1) / TX;
    const int x0 = (tile % ntx) * TX, y0 = (tile / ntx) * TY;
    const int tid = threadIdx.x, tx = tid & (TX - 1), ty = tid / TX;
    const int x = x0 + tx, y = y0 + ty;
    const bool in = (x < g.Nx) && (y < g.Ny);
    const int64_t off = in ? (int64_t)y * g.Nx + x : 0;
    // halo cell owned by this thread (rows above/below by threads 0..127, columns by 128..135)
    int hx = -1, hy = -1, hl = -1;
    if (tid < TX) { hx = x0 + tid; hy = y0 - 1; hl = tid + 1; }
    else if (tid < 2 * TX) { hx = x0 + tid - TX; hy = y0 + TY; hl = (TY + 1) * LW + (tid - TX) + 1; }
    else if (tid < 2 * TX + TY) { hx = x0 - 1; hy = y0 + (tid - 2 * TX); hl = (tid - 2 * TX + 1) * LW; }
    else if (tid < 2 * TX + 2 * TY) { hx = x0 + TX; hy = y0 + (tid - 2 * TX - TY); hl = (tid - 2 * TX - TY + 1) * LW + TX + 1; }
    const bool hv = hl >= 0 && hx >= 0 && hx < g.Nx && hy >= 0 && hy < g.Ny;
    const int64_t hoff = hv ? (int64_t)hy * g.Nx + hx : 0;
    const int ci = (ty + 1) * LW + tx + 1;
    const bool has_lo = g.t0 > 0, has_hi = g.t0 + g.nloc < g.Nt;

    double cm = 0.0, cc = 0.0, cn = 0.0, hc = 0.0;
    if (in) {
        if (has_lo) cm = val(-1, off);
        cc = val(0, off);
        if (g.nloc > 1 || has_hi) cn = val(1, off);
    }
    if (hv) hc = val(0, hoff);
    for (int l = 0; l < g.nloc; ++l) {
        double* buf = lds + (l & 1) * LP;
        buf[ci] = cc;
        if (hl >= 0) buf[hl] = hc;
        double cnn = 0.0, hnn = 0.0;
        if (in && (l + 2 < g.nloc || (l + 2 == g.nloc && has_hi))) cnn = val(l + 2, off);
        if (hv && l + 1 < g.nloc) hnn = val(l + 1, hoff);
        __syncthreads();
        if (in) {
            body(l, g.t0 + l, off, x, y, cc, buf[ci - 1], buf[ci + 1], buf[ci - LW], buf[ci + LW], cm, cn);
        }
        cm = cc;
        cc = cn;
        cn = cnn;
        hc = hnn;
    }
}

// ----------------------------------------------------------------------------- apply A / L

__global__ __launch_bounds__(NT) void k_apply_A(Geo g, const double* __restrict__ p, double* __restrict__ out,
                                                double r, double reps, int lap_only) {
    const int64_t nxy = g.nxy;
    march(g, blockIdx.x, [&](int l, int64_t off) { return p[l * nxy + off]; },
          [&](int l, int t, int64_t off, int x, int y, double c, double xm, double xp, double ym, double yp,
              double tm, double tp) {
              out[l * nxy + off] = lap_only ? row_L(g, t, y, x, c, xm, xp, ym, yp, tm, tp)
                                            : row_A(g, t, y, x, c, xm, xp, ym, yp, tm, tp, r, reps);
          });
}

hipError_t launch_apply_A(const Geo& g, const double* p, double* out, double r, double eps, int lap_only,
                          hipStream_t s) {
    k_apply_A<<<march_blocks(g), NT, 0, s>>>(g, p, out, r, r * eps, lap_only);
    return hipGetLastError();
}

// ----------------------------------------------------------------------------- CG iteration

struct CGPro {
    bool go;
    double rr, atol, beta;
};

// Top of scipy's cg loop for iteration k: rr = r_k . r_k (sum of the per-rank slots, rank
// order), atol = rtol*||b|| (k = 0: rr = b.b), stop if ||r|| < atol; beta = rr / rho_prev.
__device__ __forceinline__ CGPro cg_prologue(int k, const CGScal* S, const double* gath_rr, const CGArgs& a,
                                             CGScal* Sw) {
    CGPro P;
    P.go = false;
    P.beta = 0.0;
    if (S->done) return P;
    double rr = 0.0;
    for (int i = 0; i < a.world; ++i) rr += gath_rr[i];
    P.rr = rr;
    if (k == 0) {
        P.atol = fmax(0.0, a.rtol * sqrt(rr));
        if (rr == 0.0) {
            if (blockIdx.x == 0 && threadIdx.x == 0) { Sw->done = 1; Sw->iters = 0; }
            return P;
        }
    } else {
        P.atol = S->atol;
    }
    if (sqrt(rr) < P.atol) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { Sw->done = 1; Sw->iters = k; }
        return P;
    }
    P.beta = (k > 0) ? rr / S->rho : 0.0;
    P.go = true;
    return P;
}

template <bool FUSED>
__global__ __launch_bounds__(NT) void k_cg_dir(Geo g, int k, const double* __restrict__ rv,
                                               const double* __restrict__ po, double* __restrict__ pn, CGArgs a,
                                               CGScal* S, RedBuf rb, const double* __restrict__ gath_rr,
                                               double* __restrict__ gath_pap) {
    const CGPro P = cg_prologue(k, S, gath_rr, a, S);
    if (!P.go) return;
    const int64_t nxy = g.nxy;
    const double beta = P.beta, r = a.r, reps = a.r * a.eps;
    double acc = 0.0;
    march(
        g, blockIdx.x,
        [&](int l, int64_t off) -> double {
            const int64_t i = l * nxy + off;
            if (!FUSED) return pn[i];
            if (k == 0) return rv[i];
            return beta * po[i] + rv[i];   // scipy: p *= beta; p += z
        },
        [&](int l, int t, int64_t off, int x, int y, double c, double xm, double xp, double ym, double yp,
            double tm, double tp) {
            const double q = row_A(g, t, y, x, c, xm, xp, ym, yp, tm, tp, r, reps);
            acc += c * q;
            if (FUSED) pn[l * nxy + off] = c;
        });
    double v[1] = {acc}, tot[1];
    if (grid_reduce_last<1>(v, rb, tot) && threadIdx.x == 0) {
        S->rho = P.rr;
        if (k == 0) { S->bb = P.rr; S->atol = P.atol; }
        S->pap = tot[0];
        gath_pap[a.rank] = tot[0];
    }
}

// Pointwise p = r + beta p for the sharded (non-fused) path: the halo planes of the new p
// are then exchanged before k_cg_dir<false> applies A.
__global__ __launch_bounds__(NT) void k_cg_pupd(Geo g, int k, const double* __restrict__ rv,
                                                const double* __restrict__ po, double* __restrict__ pn,
                                                CGScal* S, const double* __restrict__ gath_rr, CGArgs a) {
    // decision only (no state writes: k_cg_dir<false> repeats the prologue and writes)
    if (S->done) return;
    double rr = 0.0;
    for (int i = 0; i < a.world; ++i) rr += gath_rr[i];
    double atol = (k == 0) ? fmax(0.0, a.rtol * sqrt(rr)) : S->atol;
    if (rr == 0.0 || sqrt(rr) < atol) return;
    const double beta = (k > 0) ? rr / S->rho : 0.0;
    const int64_t n = (int64_t)g.nloc * g.nxy;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT)
        pn[i] = (k == 0) ? rv[i] : beta * po[i] + rv[i];
}

__global__ __launch_bounds__(NT) void k_cg_upd(Geo g, int k, const double* __restrict__ p, double* __restrict__ xv,
                                               double* __restrict__ rv, CGArgs a, CGScal* S, RedBuf rb,
                                               const double* __restrict__ gath_pap, double* __restrict__ gath_rr) {
    if (S->done) return;
    double pap = 0.0;
    for (int i = 0; i < a.world; ++i) pap += gath_pap[i];
    const double alpha = S->rho / pap;
    const int64_t nxy = g.nxy;
    const double r = a.r, reps = a.r * a.eps;
    double acc = 0.0;
    march(
        g, blockIdx.x, [&](int l, int64_t off) -> double { return p[l * nxy + off]; },
        [&](int l, int t, int64_t off, int x, int y, double c, double xm, double xp, double ym, double yp,
            double tm, double tp) {
            const double q = row_A(g, t, y, x, c, xm, xp, ym, yp, tm, tp, r, reps);
            const int64_t i = l * nxy + off;
            const double ap = alpha * c;
            xv[i] = (k == 0) ? 0.0 + ap : xv[i] + ap;   // x += alpha*p
            const double rn = rv[i] - alpha * q;       // r -= alpha*q
            rv[i] = rn;
            acc += rn * rn;
        });
    double v[1] = {acc}, tot[1];
    if (grid_reduce_last<1>(v, rb, tot) && threadIdx.x == 0) gath_rr[a.rank] = tot[0];
}

hipError_t launch_cg_dir(const Geo& g, int k, const double* rvec, const double* pold, double* pnew,
                         const CGArgs& a, CGScal* S, RedBuf rb, const double* gath_rr, double* gath_pap,
                         int fused, hipStream_t s) {
    if (fused)
        k_cg_dir<true><<<march_blocks(g), NT, 0, s>>>(g, k, rvec, pold, pnew, a, S, rb, gath_rr, gath_pap);
    else
        k_cg_dir<false><<<march_blocks(g), NT, 0, s>>>(g, k, rvec, pold, pnew, a, S, rb, gath_rr, gath_pap);
    return hipGetLastError();
}

hipError_t launch_cg_pupd(const Geo& g, int k, const double* rvec, const double* pold, double* pnew, CGScal* S,
                          const double* gath_rr, const CGArgs& a, hipStream_t s) {
    const int64_t n = (int64_t)g.nloc * g.nxy;
    int nb = (int)std::min<int64_t>((n + NT - 1) / NT, 4096);
    k_cg_pupd<<<nb, NT, 0, s>>>(g, k, rvec, pold, pnew, S, gath_rr, a);
    return hipGetLastError();
}

hipError_t launch_cg_upd(const Geo& g, int k, const double* p, double* x, double* rvec, const CGArgs& a,
                         CGScal* S, RedBuf rb, const double* gath_pap, double* gath_rr, hipStream_t s) {
    k_cg_upd<<<march_blocks(g), NT, 0, s>>>(g, k, p, x, rvec, a, S, rb, gath_pap, gath_rr);
    return hipGetLastError();
}

// ============================================================================ gradients / divergence

// grad_1d_central_weird (bc 'N', h = 1) row at index k of an axis of length n, given the
// values at k-1, k, k+1 (operators.py:33-48).  (-0.5 a) + (0.5 b) == 0.5 (b - a) exactly.
__device__ __forceinline__ double d1w(int k, int n, double m, double c, double p) {
    if (k == 0) return p - c;
    if (k == n - 1) return c - m;
    return 0.5 * (p - m);
}

__global__ __launch_bounds__(NT) void k_grad_st(Geo g, const double* __restrict__ phi, double* __restrict__ gt,
                                                double* __restrict__ gx, double* __restrict__ gy) {
    const int64_t n = (int64_t)g.nloc * g.nxy;
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int l = (int)(i / g.nxy);
    const int64_t off = i - (int64_t)l * g.nxy;
    const int y = (int)(off / g.Nx), x = (int)(off - (int64_t)y * g.Nx), t = g.t0 + l;
    const double c = phi[i];
    gt[i] = d1w(t, g.Nt, t > 0 ? phi[i - g.nxy] : 0.0, c, t < g.Nt - 1 ? phi[i + g.nxy] : 0.0);
    gx[i] = d1w(x, g.Nx, x > 0 ? phi[i - 1] : 0.0, c, x < g.Nx - 1 ? phi[i + 1] : 0.0);
    gy[i] = d1w(y, g.Ny, y > 0 ? phi[i - g.Nx] : 0.0, c, y < g.Ny - 1 ? phi[i + g.Nx] : 0.0);
}

hipError_t launch_grad_st(const Geo& g, const double* phi, double* gt, double* gx, double* gy, hipStream_t s) {
    k_grad_st<<<flat_blocks((int64_t)g.nloc * g.nxy), NT, 0, s>>>(g, phi, gt, gx, gy);
    return hipGetLastError();
}

// div_st row (operators.py:129-142): scipy's COO matvec accumulates the t-block terms, then
// the x-block, then the y-block, each in ascending column order, starting from 0.
__device__ __forceinline__ void acc_d1w(double& s, int k, int n, double m, double c, double p) {
    if (k == 0) { s += -1.0 * c; s += 1.0 * p; }
    else if (k == n - 1) { s += -1.0 * m; s += 1.0 * c; }
    else { s += -0.5 * m; s += 0.5 * p; }
}

template <class W>
__device__ __forceinline__ double div_st_row(const Geo& g, int64_t i, int t, int y, int x, W w) {
    double s = 0.0;
    acc_d1w(s, t, g.Nt, t > 0 ? w(0, i - g.nxy) : 0.0, w(0, i), t < g.Nt - 1 ? w(0, i + g.nxy) : 0.0);
    acc_d1w(s, x, g.Nx, x > 0 ? w(1, i - 1) : 0.0, w(1, i), x < g.Nx - 1 ? w(1, i + 1) : 0.0);
    acc_d1w(s, y, g.Ny, y > 0 ? w(2, i - g.Nx) : 0.0, w(2, i), y < g.Ny - 1 ? w(2, i + g.Nx) : 0.0);
    return s;
}

__global__ __launch_bounds__(NT) void k_div_st(Geo g, const double* __restrict__ wt, const double* __restrict__ wx,
                                               const double* __restrict__ wy, double* __restrict__ out) {
    const int64_t n = (int64_t)g.nloc * g.nxy;
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int l = (int)(i / g.nxy);
    const int64_t off = i - (int64_t)l * g.nxy;
    const int y = (int)(off / g.Nx), x = (int)(off - (int64_t)y * g.Nx);
    const double* W[3] = {wt, wx, wy};
    out[i] = div_st_row(g, i, g.t0 + l, y, x, [&](int f, int64_t j) { return W[f][j]; });
}

hipError_t launch_div_st(const Geo& g, const double* wt, const double* wx, const double* wy, double* out,
                         hipStream_t s) {
    k_div_st<<<flat_blocks((int64_t)g.nloc * g.nxy), NT, 0, s>>>(g, wt, wx, wy, out);
    return hipGetLastError();
}

// ----------------------------------------------------------------------------- RHS (stepA)

// F = div_st(mu - r q); F[t=0] -= rho0 - rho[0] + r a[0]; F[t=Nt-1] += rhoT - rho + r a
// (benamou_brenier.py:64-82, dt = 1).  F.F partial -> gath[rank] (= b.b for CG).
constexpr int RHS_TY = 1;              // rows per block: the y-neighbour rows a tile re-reads are 2 / RHS_TY extra
constexpr int RHS_NT = TX * RHS_TY;
__global__ __launch_bounds__(RHS_NT) void k_rhs(Geo g, const double* __restrict__ mut, const double* __restrict__ mux,
                                            const double* __restrict__ muy, const double* __restrict__ qt,
                                            const double* __restrict__ qx, const double* __restrict__ qy,
                                            const double* __restrict__ rho0, const double* __restrict__ rhoT,
                                            double r, double* __restrict__ F, RedBuf rb, double* gath, int rank,
                                            int tch) {
    // one thread per (x, y) column of a 64 x RHS_TY tile, marching over a chunk of tch of the
    // shard's planes (chunks: more columns in flight than the 307 k of one full march, at the
    // cost of re-reading the t-field of two planes per chunk); the t-field w_t = mu_t - r q_t
    // of planes t-1, t, t+1 stays in registers (loaded one plane ahead), the x / y fields'
    // neighbours are same-row / adjacent-row loads (L1 / L2 hits).
    const int ntx = (g.Nx + TX - 1) / TX, ntiles = ntx * ((g.Ny + RHS_TY - 1) / RHS_TY);
    const int lin = xcd_tile(blockIdx.x);
    const int ch = lin / ntiles, tile = lin - ch * ntiles;
    const int l0 = ch * tch, l1 = min(g.nloc, l0 + tch);
    const int x = (tile % ntx) * TX + (threadIdx.x & (TX - 1));
    const int y = (tile / ntx) * RHS_TY + threadIdx.x / TX;
    const bool in = x < g.Nx && y < g.Ny && l0 < g.nloc;
    const int64_t nxy = g.nxy, off = in ? (int64_t)y * g.Nx + x : 0;
    const bool has_lo = g.t0 > 0, has_hi = g.t0 + g.nloc < g.Nt;
    auto wt = [&](int l) { const int64_t i = l * nxy + off; return mut[i] - r * qt[i]; };
    auto wx = [&](int64_t i) { return mux[i] - r * qx[i]; };
    auto wy = [&](int64_t i) { return muy[i] - r * qy[i]; };
    double ff = 0.0;
    if (in) {
        double tm = (l0 > 0 || has_lo) ? wt(l0 - 1) : 0.0, tc = wt(l0);
        double tp = (l0 + 1 < g.nloc || has_hi) ? wt(l0 + 1) : 0.0;
        for (int l = l0; l < l1; ++l) {
            const int t = g.t0 + l;
            const double tpp =
                (l + 1 < l1 && (l + 2 < g.nloc || (l + 2 == g.nloc && has_hi))) ? wt(l + 2) : 0.0;
            const int64_t i = l * nxy + off;
            double s = 0.0;
            acc_d1w(s, t, g.Nt, tm, tc, tp);
            acc_d1w(s, x, g.Nx, x > 0 ? wx(i - 1) : 0.0, wx(i), x < g.Nx - 1 ? wx(i + 1) : 0.0);
            acc_d1w(s, y, g.Ny, y > 0 ? wy(i - g.Nx) : 0.0, wy(i), y < g.Ny - 1 ? wy(i + g.Nx) : 0.0);
            if (t == 0) s -= (rho0[off] - mut[i]) + r * qt[i];
            if (t == g.Nt - 1) s += (rhoT[off] - mut[i]) + r * qt[i];
            F[i] = s;
            ff += s * s;
            tm = tc;
            tc = tp;
            tp = tpp;
        }
    }
    if (!gath) return;   // F.F only feeds the stencil CG's stopping rule (the spectral CG takes it from b^)
    double v[1] = {ff}, tot[1];
    if (grid_reduce_last<1, RHS_NT>(v, rb, tot) && threadIdx.x == 0) gath[rank] = tot[0];
}

hipError_t launch_rhs(const Geo& g, const double* mut, const double* mux, const double* muy, const double* qt,
                      const double* qx, const double* qy, const double* rho0, const double* rhoT, double r,
                      double* F, RedBuf rb, double* gath, int rank, hipStream_t s) {
    constexpr int tch = 8;   // planes per chunk: four chunks at Nt = 32
    const int nch = (g.nloc + tch - 1) / tch;
    const int nb = ((g.Nx + TX - 1) / TX) * ((g.Ny + RHS_TY - 1) / RHS_TY) * nch;
    k_rhs<<<nb, RHS_NT, 0, s>>>(g, mut, mux, muy, qt, qx, qy, rho0, rhoT, r, F, rb, gath, rank, tch);
    return hipGetLastError();
}

// ----------------------------------------------------------------------------- transport report

// foto_bb_report: FOTO_REPORT_COLS sums per time plane over (rho, m1, m2) = mu and g = grad_st phi
// (include/foto.h has the terms; benamou_brenier.py:64-82, 246-248, 262-267).  One read of the
// four fields.  A block owns one piece -- REPORT_PIECE consecutive voxels -- of one local plane (the
// grid is pieces x nloc), so the pieces of a plane depend on (Nx, Ny) alone and a plane's sums are
// the same bits however the planes are sharded.  Per plane: block partials to part[plane][col][piece]
// (write-through), a ticket of the plane's own, and the block whose add comes last sums the
// plane's partials in piece order with the fixed tree (grid_reduce_last's hand-off, one ticket
// per plane instead of one per launch).  No floating-point atomics.
// The t-neighbours of a shard's edge planes come through in.rho_lo / rho_hi / phi_lo / phi_hi
// (mu's halo planes are not exchanged on the fused path).  Ordinary loads: the state is read
// again by the next outer iteration.
constexpr int REP_VPT = REPORT_PIECE / NT;   // voxels per thread
__global__ __launch_bounds__(NT) void k_report(Geo g, ReportIn in, double* __restrict__ part, unsigned* ticket,
                                               double* __restrict__ out) {
    constexpr int K = FOTO_REPORT_COLS;
    __shared__ double sh[K * (NT / 64)];
    __shared__ int is_last;
    // block -> (piece, plane).  Which block sums which piece does not enter the result, so the
    // map is free: the blocks go to the 8 XCDs round robin, each with its own L2; every XCD gets
    // a contiguous range of (piece, plane) items, plane fastest, so the three blocks that read a
    // piece of plane l (as t-1, t, t+1) and the blocks of the pieces next to it run close together
    // behind one L2 (152 -> 139 us at 640 x 480 x 32 against piece = blockIdx.x, plane = blockIdx.y)
    const int pieces = gridDim.x;
    int l, piece;
    {
        constexpr int NXCD = 8;
        const int nb = gridDim.x * gridDim.y, b = blockIdx.y * gridDim.x + blockIdx.x;
        const int per = nb / NXCD, rem = nb % NXCD, xcd = b % NXCD;
        const int item = xcd * per + min(xcd, rem) + b / NXCD;
        piece = item / g.nloc;
        l = item - piece * g.nloc;
    }
    const int t = g.t0 + l;
    const int64_t nxy = g.nxy;
    const bool first = t == 0, last = t == g.Nt - 1;
    // the plane and its t-neighbours: the shard's own planes, or at its edges the plane the caller
    // passed (at the global ends the plane itself stands in: the value is selected away below)
    const double* const rc = in.rho + (int64_t)l * nxy;
    const double* const pc = in.phi + (int64_t)l * nxy;
    const double* const m1c = in.m1 + (int64_t)l * nxy;
    const double* const m2c = in.m2 + (int64_t)l * nxy;
    const double* const rm = l > 0 ? rc - nxy : first ? rc : in.rho_lo;
    const double* const pm = l > 0 ? pc - nxy : first ? pc : in.phi_lo;
    const double* const rp = l + 1 < g.nloc ? rc + nxy : last ? rc : in.rho_hi;
    const double* const pp1 = l + 1 < g.nloc ? pc + nxy : last ? pc : in.phi_hi;
    const double* const r0 = first ? in.rho0 : in.rhoT;   // (used on plane 0 only; elsewhere a load of the line rhoT's brings)
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.0;
    // (x, y) of the thread's first voxel by one division, of the next ones (NT voxels on) by steps
    const int64_t off0 = (int64_t)piece * REPORT_PIECE + threadIdx.x;
    const int sy = NT / g.Nx, sx = NT - sy * g.Nx;
    int y = (int)(off0 / g.Nx), x = (int)(off0 - (int64_t)y * g.Nx);
#pragma unroll
    for (int e = 0; e < REP_VPT; ++e, x += sx, y += sy) {
        if (x >= g.Nx) { x -= g.Nx; ++y; }
        const int64_t off = off0 + (int64_t)e * NT;
        if (off >= nxy) continue;
        // every load is unconditional, from an index clamped into the plane, so that they issue
        // together; the edge zeros of the stencils are selected afterwards
        const bool hx = x > 0, hX = x < g.Nx - 1, hy = y > 0, hY = y < g.Ny - 1;
        const int64_t oxm = hx ? off - 1 : off, oxp = hX ? off + 1 : off;
        const int64_t oym = hy ? off - g.Nx : off, oyp = hY ? off + g.Nx : off;
        const double rho = rc[off], rho_m = rm[off], rho_p = rp[off];
        const double m1 = m1c[off], m1_m = m1c[oxm], m1_p = m1c[oxp];
        const double m2 = m2c[off], m2_m = m2c[oym], m2_p = m2c[oyp];
        const double c = pc[off], c_tm = pm[off], c_tp = pp1[off];
        const double c_xm = pc[oxm], c_xp = pc[oxp], c_ym = pc[oym], c_yp = pc[oyp];
        const double rT = in.rhoT[off], rA = r0[off];
        const double gt = d1w(t, g.Nt, !first ? c_tm : 0.0, c, !last ? c_tp : 0.0);
        const double gx = d1w(x, g.Nx, hx ? c_xm : 0.0, c, hX ? c_xp : 0.0);
        const double gy = d1w(y, g.Ny, hy ? c_ym : 0.0, c, hY ? c_yp : 0.0);
        // the continuity residual: div_st_row's three blocks on mu, then k_rhs's boundary planes with q = 0
        double cr = 0.0;
        acc_d1w(cr, t, g.Nt, !first ? rho_m : 0.0, rho, !last ? rho_p : 0.0);
        acc_d1w(cr, x, g.Nx, hx ? m1_m : 0.0, m1, hX ? m1_p : 0.0);
        acc_d1w(cr, y, g.Ny, hy ? m2_m : 0.0, m2, hY ? m2_p : 0.0);
        if (first) cr -= rA - rho;
        if (last) cr += rT - rho;
        const double mm = m1 * m1 + m2 * m2, gg = gx * gx + gy * gy, dT = rho - rT;
        const bool pos = rho > 0.0;   // (false for NaN: a NaN density counts as emptied)
        v[FOTO_REPORT_MASS] += rho;
        v[FOTO_REPORT_KINETIC] += pos ? mm / (rho + rho) : 0.0;
        v[FOTO_REPORT_VACUUM] += pos ? 0.0 : mm;
        v[FOTO_REPORT_CONT] += cr * cr;
        v[FOTO_REPORT_HJ_NUM] += rho * fabs(gt + 0.5 * gg);
        v[FOTO_REPORT_HJ_DEN] += rho * gg;
        v[FOTO_REPORT_DUAL] += first ? -(c * rA) : last ? c * rT : 0.0;
        v[FOTO_REPORT_DIST_T] += dT * dT;
    }
    block_sum<K>(v, sh);
    double* const pp = part + (int64_t)t * K * pieces;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) partial_store(&pp[(int64_t)k * pieces + piece], v[k]);
        is_last = ticket_take_last(&ticket[t], pieces);
    }
    __syncthreads();
    if (!is_last) return;
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (int p = threadIdx.x; p < pieces; p += NT) {
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += partial_load(&pp[(int64_t)k * pieces + p]);
    }
    block_sum<K>(acc, sh);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) out[(int64_t)t * K + k] = acc[k];
        ticket_reset(&ticket[t]);
    }
}

hipError_t launch_report(const Geo& g, const ReportIn& in, double* part, unsigned* ticket, double* out,
                         hipStream_t s) {
    k_report<<<dim3(report_pieces(g.nxy), g.nloc), NT, 0, s>>>(g, in, part, ticket, out);
    return hipGetLastError();
}

// mu_rho[n] = (1 - n/(Nt-1)) rho0 + (n/(Nt-1)) rhoT, m = 0, q = 0 (benamou_brenier.py:191-194)
__global__ __launch_bounds__(NT) void k_init_mu(Geo g, const double* __restrict__ rho0,
                                                const double* __restrict__ rhoT, double* mut, double* mux,
                                                double* muy, double* qt, double* qx, double* qy) {
    const int64_t n = (int64_t)g.nloc * g.nxy;
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int l = (int)(i / g.nxy);
    const int64_t off = i - (int64_t)l * g.nxy;
    const double s = (double)(g.t0 + l) / (double)(g.Nt - 1);
    mut[i] = (1.0 - s) * rho0[off] + s * rhoT[off];
    mux[i] = 0.0;
    muy[i] = 0.0;
    qt[i] = 0.0;
    qx[i] = 0.0;
    qy[i] = 0.0;
}

hipError_t launch_init_mu(const Geo& g, const double* rho0, const double* rhoT, double* mut, double* mux,
                          double* muy, double* qt, double* qx, double* qy, hipStream_t s) {
    k_init_mu<<<flat_blocks((int64_t)g.nloc * g.nxy), NT, 0, s>>>(g, rho0, rhoT, mut, mux, muy, qt, qx, qy);
    return hipGetLastError();
}

// ============================================================================ stepB (A8)

// The projection of benamou_brenier.py:123-148 with the reference's branch tests and
// closed forms, in an algebraically identical but cheaper form: (cos, sin)(atan2(b2, b1))
// = (b1, b2) / |b|, x^(1/3) -> cbrt(x), (a+1)^3 and m^(3/2) by products.  Each changes a
// result by at most an ulp or two (checked to 1e-12 against the reference's stepB in
// tests/golden/stepb.npz, including both branches and the boundary, and held to 4 x the
// reference formulas' own error against the exact projection in tests/test_gpu_projk.py;
// DESIGN.md 3.2 has the figures); stepB runs once per
// outer iteration on every voxel, and atan2 / cos / sin / pow would dominate it.
// rare branch (a < -1, small |b|): kept out of line so its acos / cos do not inflate the
// register allocation of the kernels that inline project_K
__device__ __noinline__ double proj_trig_z(double al, double rho) {
    const double m = -al - 1.0;
    const double sm = sqrt(m);
    // on the seam with the cubic branch the argument is 1 and can round an ulp or two above it
    // (acos -> NaN; the projection itself is smooth there): capped by a select, which unlike
    // fmin lets a NaN argument through
    const double x = 1.8371173070873836 * rho / (m * sm);
    return 1.632993161855452 * sm * cos(0.3333333333333333 * acos(x > 1.0 ? 1.0 : x));
}

// S^(1/3) and S^(-1/3) for finite S > 0 without the library cbrt and a division: S = m 2^e
// (m in [0.5, 1)), e = 3q + s (s in {0, 1, 2}), S' = m 2^s in [0.5, 4); y ~ S'^(-1/3) from the
// fp32 log2 / exp2 (~1e-7 relative), two Newton steps y <- y (4 - S' y^3) / 3 (quadratic:
// rounding level), then S^(1/3) = S' y^2 2^q and S^(-1/3) = y 2^-q.  Within 2-3 ulp of the
// rounded values (the reference's x ** (1/3) is itself within an ulp of them).
__device__ __forceinline__ void cbrt_pair(double S, double& c, double& ic) {
    const int e = __builtin_amdgcn_frexp_exp(S);
    const double m = __builtin_amdgcn_frexp_mant(S);
    const int q = (e >= 0) ? e / 3 : -((2 - e) / 3);   // floor(e / 3)
    const double Sp = __builtin_amdgcn_ldexp(m, e - 3 * q);
    const float yf = __builtin_amdgcn_exp2f(-0.3333333333f * __builtin_amdgcn_logf((float)Sp));
    double y = (double)yf;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double y3 = (y * y) * y;
        y = (y * fma(-Sp, y3, 4.0)) * 0.3333333333333333;
    }
    c = __builtin_amdgcn_ldexp((Sp * y) * y, q);
    ic = __builtin_amdgcn_ldexp(y, -q);
}

__device__ __forceinline__ void project_K(double al, double b1, double b2, double& oa, double& o1, double& o2) {
    if (2.0 * al + b1 * b1 + b2 * b2 <= 0.0) {
        oa = al; o1 = b1; o2 = b2;
        return;
    }
    const double SQRT2 = 1.4142135623730951;
    const double rho = sqrt(b1 * b1 + b2 * b2);
    const double ap1 = al + 1.0;
    double aH, rH;
    if (-32.0 * (ap1 * ap1 * ap1) - 108.0 * (rho * rho) < 0.0) {
        // the polynomial is (4 (a+1)^3 + 13.5 rho^2) / 3 expanded as the reference writes it: > 0
        // in this branch, but next to the seam (a < -1) its terms cancel and the sum can round
        // below 0 (sqrt -> NaN).  Floored by a select (a NaN passes, which fmax would swallow)
        const double D = 1.3333333333333333 * (al * al * al) + 4.0 * (al * al) + 4.5 * (rho * rho) + 4.0 * al +
                         1.3333333333333333;
        const double S = 0.3535533905932738 * rho + 0.16666666666666666 * sqrt(D < 0.0 ? 0.0 : D);
        double c, ic;
        if (S > 0.0 && S <= 1.7976931348623157e308) {
            cbrt_pair(S, c, ic);
        } else {
            c = cbrt(S);
            ic = 1.0 / c;
        }
        const double zh = fma(-0.3333333333333333 * ap1, ic, c);
        aH = -(zh * zh);
        rH = SQRT2 * zh;
    } else {
        const double zh = proj_trig_z(al, rho);
        aH = -0.5 * (zh * zh);
        rH = zh;
    }
    oa = aH;
    if (rho > 0.0) {
        const double ir = 1.0 / rho;
        o1 = rH * (b1 * ir);
        o2 = rH * (b2 * ir);
    } else {   // atan2(+-0, +0) = +-0, atan2(+-0, -0) = +-pi: rH cos = +-rH, rH sin = a zero of
               // rH's sign times b2's (the reference's rH sin(+-pi) is rH * +-1.2e-16 instead)
        o1 = signbit(b1) ? -rH : rH;
        o2 = rH * b2;
    }
}

__global__ __launch_bounds__(NT) void k_stepB(int64_t M, const double* __restrict__ pa, const double* __restrict__ p1,
                                              const double* __restrict__ p2, double* __restrict__ qa,
                                              double* __restrict__ q1, double* __restrict__ q2) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= M) return;
    double a, b, c;
    project_K(pa[i], p1[i], p2[i], a, b, c);
    qa[i] = a;
    q1[i] = b;
    q2[i] = c;
}

hipError_t launch_stepB(int64_t M, const double* pa, const double* p1, const double* p2, double* qa, double* q1,
                        double* q2, hipStream_t s) {
    k_stepB<<<flat_blocks(M), NT, 0, s>>>(M, pa, p1, p2, qa, q1, q2);
    return hipGetLastError();
}

// ============================================================================ stepB + stepC + crit (fused)

// g = grad_st phi; q = Proj_K(g + (1/r) mu); mu += r (g - q); mu_rho = max(mu_rho, 0);
// num += mu_rho |g_t + (g_x^2 + g_y^2)/2|, den += mu_rho (g_x^2 + g_y^2)
// (benamou_brenier.py:213-248).
__global__ __launch_bounds__(NT) void k_prox(Geo g, const double* __restrict__ phi, double* __restrict__ mut,
                                             double* __restrict__ mux, double* __restrict__ muy,
                                             double* __restrict__ qt, double* __restrict__ qx,
                                             double* __restrict__ qy, double r, double inv_r, RedBuf rb,
                                             double* gath, int rank, const int* __restrict__ guard) {
    // 2.5-D march over phi (64 x 4 LDS tile + halo, t-neighbours in registers), then the
    // pointwise stepB / stepC / criterion terms of each voxel.
    // guard: the CG's done flag when the host enqueued this without waiting for the solve; an
    // unfinished solve leaves mu, q untouched and the host re-runs prox after finishing it.
    if (guard && *guard == 0) return;
    const int64_t nxy = g.nxy;
    double num = 0.0, den = 0.0;
    march(g, blockIdx.x, [&](int l, int64_t off) { return phi[l * nxy + off]; },
          [&](int l, int t, int64_t off, int x, int y, double c, double xm, double xp, double ym, double yp,
              double tm, double tp) {
              const int64_t i = l * nxy + off;
              const double gt = d1w(t, g.Nt, tm, c, tp);
              const double gx = d1w(x, g.Nx, xm, c, xp);
              const double gy = d1w(y, g.Ny, ym, c, yp);
              const double m0 = mut[i], m1 = mux[i], m2 = muy[i];
              double a, b1, b2;
              project_K(gt + inv_r * m0, gx + inv_r * m1, gy + inv_r * m2, a, b1, b2);
              qt[i] = a;
              qx[i] = b1;
              qy[i] = b2;
              double n0 = m0 + r * (gt - a);
              n0 = (n0 < 0.0) ? 0.0 : n0;   // np.maximum(mu, 0) (NaN propagates)
              mut[i] = n0;
              mux[i] = m1 + r * (gx - b1);
              muy[i] = m2 + r * (gy - b2);
              const double gg = gx * gx + gy * gy;
              num += n0 * fabs(gt + 0.5 * gg);
              den += n0 * gg;
          });
    double v[2] = {num, den}, tot[2];
    if (grid_reduce_last<2>(v, rb, tot) && threadIdx.x == 0) {
        gath[2 * rank] = tot[0];
        gath[2 * rank + 1] = tot[1];
    }
}

hipError_t launch_prox(const Geo& g, const double* phi, double* mut, double* mux, double* muy, double* qt,
                       double* qx, double* qy, double r, RedBuf rb, double* gath, int rank, hipStream_t s,
                       const int* guard) {
    k_prox<<<march_blocks(g), NT, 0, s>>>(g, phi, mut, mux, muy, qt, qx, qy, r, 1.0 / r, rb, gath, rank, guard);
    return hipGetLastError();
}

// q = Proj_K(grad_st phi + mu / r) alone (k_prox's formulas; mu untouched): the stepB output of
// the last outer iteration, recomputed on demand where the fused kernel below never stores it.
__global__ __launch_bounds__(NT) void k_q_from_phi(Geo g, const double* __restrict__ phi,
                                                   const double* __restrict__ mut, const double* __restrict__ mux,
                                                   const double* __restrict__ muy, double* __restrict__ qt,
                                                   double* __restrict__ qx, double* __restrict__ qy, double inv_r) {
    const int64_t nxy = g.nxy;
    march(g, blockIdx.x, [&](int l, int64_t off) { return phi[l * nxy + off]; },
          [&](int l, int t, int64_t off, int x, int y, double c, double xm, double xp, double ym, double yp,
              double tm, double tp) {
              const int64_t i = l * nxy + off;
              double a, b1, b2;
              project_K(d1w(t, g.Nt, tm, c, tp) + inv_r * mut[i], d1w(x, g.Nx, xm, c, xp) + inv_r * mux[i],
                        d1w(y, g.Ny, ym, c, yp) + inv_r * muy[i], a, b1, b2);
              qt[i] = a;
              qx[i] = b1;
              qy[i] = b2;
          });
}

hipError_t launch_q_from_phi(const Geo& g, const double* phi, const double* mut, const double* mux,
                             const double* muy, double* qt, double* qx, double* qy, double r, hipStream_t s) {
    k_q_from_phi<<<march_blocks(g), NT, 0, s>>>(g, phi, mut, mux, muy, qt, qx, qy, 1.0 / r);
    return hipGetLastError();
}

// ============================================================================ prox + next RHS (fused)
//
// One outer iteration's stepB / stepC / criterion (k_prox) fused with the NEXT iteration's
// right-hand side (k_rhs): F = div_st(mu' - r q) + BC needs only the new mu' and q of a voxel
// and its six neighbours, so the kernel that produces them can finish F itself -- q is never
// stored and mu' is never re-read (k_prox + k_rhs move 80 + 56 B per voxel, this kernel
// 8 (phi) + 24 (mu) + 24 (mu') + 8 (F) = 64 B).  The price is the neighbours' stepB: a block
// owns a 64 x 8 tile of F over a chunk of planes [l0, l1) and computes stepB on the tile plus
// a one-voxel ring (66 x 10: the x / y neighbours F needs) and on the planes l0 - 1 and l1
// (the t neighbours), which needs phi on a two-voxel ring (68 x 12) and planes l0 - 2 .. l1 + 1.
// mu' goes to a second buffer (neighbouring blocks still read the old mu of their ring voxels).
// Time-sharded there are two ways across a slab boundary.  EDGE RECOMPUTE (FOTO_PR_EDGE=0): a
// shard's first and last chunks recompute stepB on the neighbouring ranks' boundary planes
// exactly as the chunk seams do -- phi needs two halo planes and mu one on each side, five
// planes per neighbour on the wire.  EDGE DEFER (default): stepB stays on the own planes, F of a
// plane next to another rank is deferred -- the kernel stores w_t of its two outermost planes on
// each deferred side and (w_x, w_y, mu'_t, q_t) of the edge plane itself, one w_t plane is
// exchanged with each neighbour, and k_rhs_edge finishes F there with the same operations in the
// same order: phi one halo plane, w_t one -- two planes per neighbour.  Plane indices p are local
// (memory: p * nxy); t = t0 + p is global (boundary conditions).  Per voxel the arithmetic is k_prox's and k_rhs's, in the same order:
// mu', F and the crit terms are bit-identical to the unfused kernels; only the crit / F.F sums
// are grouped differently.
//
// Iteration p of the march (p = max(l0 - 1, 0) .. l1): store phi(p + 2) (loaded during the
// previous iteration) into a 4-plane LDS ring, issue the loads of phi(p + 3) and mu(p + 1),
// stepB on plane p (phi planes p - 1 .. p + 1 from the ring) -> w = mu' - r q of plane p into
// a double-buffered LDS image (x, y parts; the own voxel's t part stays in registers), then
// F(p - 1) from w of planes p - 2 .. p; one barrier per iteration.  Threads 0..147 (waves
// 0-2) also take the 148 ring voxels -- on the chunk's own planes only: of the planes l0 - 1 and
// l1, F reads the own voxels' w_t alone, which stays in registers, so those two iterations load
// no ring mu, run no ring stepB and write no w image.  Chunks of FOTO_PR_TCH planes (default 16)
// give the grid more blocks than resident slots (a full-length march leaves a one-sixth-full
// second round at 640 x 480).
// The wait for a plane's loads must not wait for the stores issued behind them (vmcnt retires in
// order: the loads of plane p + 1 go out before the mu' and F stores of plane p).  The compiler
// counts those stores only where every wave executes them, so the iterations in which every
// plane condition holds -- the STEADY planes, 24 of the two chunks' 35 iterations at Nt = 32 --
// run a copy of the iteration without the conditions, and mu(p + 1) alternates between two
// register sets instead of being copied at the back edge (prox_rhs_body has the bounds and the
// argument that every wave runs the same barriers).  Not on a deferred-edge shard (EDGE).
// Addresses: plane base + tile origin in scalar registers, one 32-bit byte offset per voxel and
// thread for all eight arrays (byte_at, in_loop) instead of a 64-bit address pair per array.
// Cache policy of the streams.  mu' is read again only by the next outer iteration's prox,
// ~1.5 GB of other traffic later: stored non-temporal it does not displace the lines the next
// kernels read (F, phi; F itself is stored plainly, the x-DCT reads it next).  The old mu is dead
// after this kernel: its loads, the own and the ring voxels', are non-temporal, so F stays cached
// for the x-DCT.  phi is loaded plainly: its halo is re-read.  (A/B figures: DESIGN.md 3.5.)
constexpr int PR_X = 64, PR_Y = 8;

// base + a 32-bit byte offset: with a block-uniform base the access takes the base from scalar
// registers and one VGPR of offset
template <class T>
__device__ __forceinline__ T* byte_at(T* base, uint32_t off) {
    return (T*)((const char*)base + off);
}
// ... and stays one: an offset the compiler has to take as new at each use, so that it does not
// hoist a 64-bit base + offset per array and thread out of the march's loops
__device__ __forceinline__ uint32_t in_loop(uint32_t off) {
    asm volatile("" : "+v"(off));
    return off;
}
// a block-uniform element offset, held in scalar registers also where it is used under a lane mask
__device__ __forceinline__ int64_t uniform64(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
constexpr int PR_VPT = 1;                                   // own voxels per thread (the march is written over v < PR_VPT)
constexpr int PR_NT = PR_X * PR_Y / PR_VPT;                 // 512 threads (64 x 8)
constexpr int PR_YV = PR_Y / PR_VPT;                        // rows between a thread's own voxels
constexpr int PR_PW = PR_X + 2, PR_PH = PR_Y + 2;         // stepB region
constexpr int PR_FW = PR_X + 4, PR_FH = PR_Y + 4;         // phi region
constexpr int PR_HALO = 2 * PR_PW + 2 * PR_Y;             // 148 ring voxels (64 x 8)
constexpr int PR_FN = PR_FW * PR_FH;                      // 816 phi values per plane
constexpr int PR_FR = (PR_FN + PR_NT - 1) / PR_NT;        // phi loads per thread per plane
static_assert(PR_X == 64 && PR_NT <= 1024 && PR_HALO <= PR_NT && PR_Y % PR_VPT == 0,   // (32 x 16, 16 x 32, 32 x 8: slower, r03)
              "whole rows per thread, ring voxels on the first threads");
constexpr int PR_WPE = 4;                                 // waves per SIMD (VGPR budget 128)

// EDGE: the deferred-edge variant (sharded); the single-shard instantiation carries none of its
// code (its extra registers spilled the kernel at the 128-VGPR cap: 171 -> 184 us)
// INTERIOR (round 6): the block's whole phi region (the tile plus a two-voxel ring) lies inside
// the plane, so every own voxel, ring voxel and phi load is in the grid and every x / y
// neighbour F reads exists -- the per-lane bound tests and the branches around the loads they
// guard fold away (77 % of the blocks at 640 x 480).  The same arithmetic in the same order.
template <bool EDGE, bool INTERIOR>
__device__ __forceinline__ void prox_rhs_body(
        Geo g, const double* __restrict__ phi, const double* __restrict__ mut, const double* __restrict__ mux,
        const double* __restrict__ muy, double* __restrict__ nut, double* __restrict__ nux, double* __restrict__ nuy,
        const double* __restrict__ rho0, const double* __restrict__ rhoT, double r, double inv_r,
        double* __restrict__ F, int tch, int defer_lo, int defer_hi, double* __restrict__ wt_out,
        double* __restrict__ edge, int wt_pre, double (*fr)[PR_FN], double (*wb)[2][PR_PH * PR_PW], int ch, int x0,
        int y0, double& num_out, double& den_out, double& ff_out) {
    const int Nt = g.Nt, Nx = g.Nx, Ny = g.Ny, t0 = g.t0;
    const int64_t nxy = g.nxy;
    const int l0 = ch * tch, l1 = min(g.nloc, l0 + tch);   // own planes of this chunk (local)
    const int tid = threadIdx.x;
    // Global addresses: a plane's base plus the origin of the tile's phi region is block-uniform
    // (scalar registers); a thread adds the 32-bit byte offset of its voxel inside the region, one
    // register for every array (prox_rhs_fits holds the region to 2^32 bytes)
    const int64_t org = (int64_t)(y0 - 2) * Nx + (x0 - 2);
    // own voxels: stepB region positions (1 + tid % 64, 1 + tid / 64 + v PR_YV)
    const int opx = 1 + (tid & (PR_X - 1));
    const int ox = x0 - 1 + opx;
    int opy[PR_VPT], oy[PR_VPT], ooff[PR_VPT];
    uint32_t oob[PR_VPT];
    bool own[PR_VPT];
#pragma unroll
    for (int v = 0; v < PR_VPT; ++v) {
        opy[v] = 1 + tid / PR_X + v * PR_YV;
        oy[v] = y0 - 1 + opy[v];
        own[v] = INTERIOR || (ox < Nx && oy[v] < Ny);
        ooff[v] = own[v] ? oy[v] * Nx + ox : 0;   // in-plane offsets fit 32 bits (the deferred edges')
        oob[v] = own[v] ? 8u * (uint32_t)((opy[v] + 1) * Nx + opx + 1) : 0u;
    }
    // ring voxel of threads 0..PR_HALO-1
    int hpx = 0, hpy = 0;
    if (tid < PR_PW) { hpx = tid; hpy = 0; }
    else if (tid < 2 * PR_PW) { hpx = tid - PR_PW; hpy = PR_PH - 1; }
    else if (tid < 2 * PR_PW + PR_Y) { hpx = 0; hpy = 1 + tid - 2 * PR_PW; }
    else { hpx = PR_PW - 1; hpy = 1 + tid - 2 * PR_PW - PR_Y; }
    const int hx = x0 - 1 + hpx, hy = y0 - 1 + hpy;
    const bool hal = tid < PR_HALO && (INTERIOR || (hx >= 0 && hx < Nx && hy >= 0 && hy < Ny));
    const uint32_t hob = hal ? 8u * (uint32_t)((hpy + 1) * Nx + hpx + 1) : 0u;
    // phi region loads of this thread
    uint32_t fob[PR_FR];
    bool fin[PR_FR];
#pragma unroll
    for (int j = 0; j < PR_FR; ++j) {
        const int idx = tid + j * PR_NT;
        const int fy = idx / PR_FW, fx = idx - fy * PR_FW;
        const int xx = x0 - 2 + fx, yy = y0 - 2 + fy;
        fin[j] = idx < PR_FN && (INTERIOR || (xx >= 0 && xx < Nx && yy >= 0 && yy < Ny));
        fob[j] = fin[j] ? 8u * (uint32_t)(fy * Nx + fx) : 0u;
    }
    // stepB planes (local): one beyond the chunk on each side, within the grid and, where an edge
    // is deferred, within the shard
    if (!EDGE) defer_lo = defer_hi = 0;
    const int pa = max(l0 - 1, defer_lo ? 0 : -t0), pz = min(l1, defer_hi ? g.nloc - 1 : Nt - 1 - t0);
    const int nl = g.nloc;
    // the steady planes: every condition of a step folds (below); none on a deferred-edge shard
    const int ps = max(l0 + 1, 2 - t0), pe = EDGE ? ps - 1 : min(pz - 2, Nt - 4 - t0);
    double fv[PR_FR];
    // ST: a steady plane, in the grid by construction
    auto load_phi_to = [&](auto st, int p, double (&v)[PR_FR]) {   // planes beyond pz + 1 are never read
        constexpr bool ST = decltype(st)::value;
        const bool ok = ST || (t0 + p >= 0 && p <= pz + 1 && t0 + p < Nt);
        const int64_t pb = uniform64(p * nxy + org);
#pragma unroll
        for (int j = 0; j < PR_FR; ++j)
            v[j] = (ok && fin[j]) ? *byte_at(phi + pb, in_loop(fob[j])) : 0.0;
    };
    auto store_phi_from = [&](int p, const double (&v)[PR_FR]) {
#pragma unroll
        for (int j = 0; j < PR_FR; ++j)
            if (tid + j * PR_NT < PR_FN) fr[p & 3][tid + j * PR_NT] = v[j];
    };
    auto store_phi = [&](int p) { store_phi_from(p, fv); };
    // mu of plane p, loaded one plane ahead: the ring voxels' (first: the own voxels' loads are the
    // unconditional ones a wait can count from) only on the chunk's own planes -- F(n) exists for
    // n in [l0, l1) and reads the ring's w of plane n alone -- then the own voxels'
    auto load_mu = [&](auto st, int p, double (&mo)[PR_VPT][3], double (&mh)[3]) {
        constexpr bool ST = decltype(st)::value;
        if (!ST && p > pz) return;
        const int64_t pb = uniform64(p * nxy + org);
        if (hal && (ST || (p >= l0 && p < l1))) {
            const uint32_t o = in_loop(hob);
            mh[0] = __builtin_nontemporal_load(byte_at(mut + pb, o));
            mh[1] = __builtin_nontemporal_load(byte_at(mux + pb, o));
            mh[2] = __builtin_nontemporal_load(byte_at(muy + pb, o));
        }
#pragma unroll
        for (int v = 0; v < PR_VPT; ++v) {
            if (own[v]) {   // (the old mu is dead after this kernel)
                const uint32_t o = in_loop(oob[v]);
                mo[v][0] = __builtin_nontemporal_load(byte_at(mut + pb, o));
                mo[v][1] = __builtin_nontemporal_load(byte_at(mux + pb, o));
                mo[v][2] = __builtin_nontemporal_load(byte_at(muy + pb, o));
            }
        }
    };
    // rho0 / rhoT under the own voxels for F(n) on a boundary plane n, issued ahead of the
    // iteration's other loads (Nt >= 2: a plane is at most one of the two): the wait for it leaves
    // those in flight where the compiler can count them, and falls behind the plane's stepB
    auto load_rho = [&](int n, double (&rc)[PR_VPT]) {
        const int tn = t0 + n;
        if (n < l0) return;
#pragma unroll
        for (int v = 0; v < PR_VPT; ++v) {
            if (own[v] && tn == 0) rc[v] = *byte_at(rho0 + org, in_loop(oob[v]));
            if (own[v] && tn == Nt - 1) rc[v] = *byte_at(rhoT + org, in_loop(oob[v]));
        }
    };
    // stepB / stepC at stepB-region position (px, py) of local plane p (k_prox's body)
    // (a steady plane has both t neighbours: d1w's interior case)
    auto stepb = [&](auto st, int p, int px, int py, int xg, int yg, const double (&m)[3], double (&w)[3],
                     double& n0o, double& ao, double& gto, double& gxo, double& gyo, double (&nu)[3]) {
        constexpr bool ST = decltype(st)::value;
        const int t = t0 + p;
        const int fi = (py + 1) * PR_FW + px + 1;
        const double* P = fr[p & 3];
        const double c = P[fi];
        const double tm = (ST || t > 0) ? fr[(p - 1) & 3][fi] : 0.0;
        const double tp = (ST || t < Nt - 1) ? fr[(p + 1) & 3][fi] : 0.0;
        const double gt = ST ? 0.5 * (tp - tm) : d1w(t, Nt, tm, c, tp);
        const double gx = d1w(xg, Nx, P[fi - 1], c, P[fi + 1]);
        const double gy = d1w(yg, Ny, P[fi - PR_FW], c, P[fi + PR_FW]);
        double a, b1, b2;
        project_K(gt + inv_r * m[0], gx + inv_r * m[1], gy + inv_r * m[2], a, b1, b2);
        double n0 = m[0] + r * (gt - a);
        n0 = (n0 < 0.0) ? 0.0 : n0;   // np.maximum(mu, 0) (NaN propagates)
        nu[0] = n0;
        nu[1] = m[1] + r * (gx - b1);
        nu[2] = m[2] + r * (gy - b2);
        w[0] = nu[0] - r * a;   // k_rhs: mu_t - r q_t, from the stored mu', q
        w[1] = nu[1] - r * b1;
        w[2] = nu[2] - r * b2;
        n0o = n0;
        ao = a;
        gto = gt;
        gxo = gx;
        gyo = gy;
    };
    double num = 0.0, den = 0.0, ff = 0.0;
    // own voxels: w_t of planes p-2, p-1, p; (mu'_t, q_t) of plane p-1 (bcm, bcq) and p (_n)
    double wtm[PR_VPT], wtc[PR_VPT], wtn[PR_VPT], bcm[PR_VPT], bcq[PR_VPT], bcm_n[PR_VPT], bcq_n[PR_VPT];
#pragma unroll
    for (int v = 0; v < PR_VPT; ++v) wtm[v] = wtc[v] = wtn[v] = bcm[v] = bcq[v] = bcm_n[v] = bcq_n[v] = 0.0;
    // plane p's stepB.  An own plane of the chunk: the own and the ring voxels, mu' out, w into
    // wb[p & 1], crit terms.  The planes l0 - 1 and l1 give F only the own voxels' w_t (registers):
    // no ring voxel, no LDS write
    auto plane = [&](auto st, int p, const double (&mo)[PR_VPT][3], const double (&mh)[3]) {
        constexpr bool ST = decltype(st)::value;
        const bool mine = ST || (p >= l0 && p < l1);
#pragma unroll
        for (int v = 0; v < PR_VPT; ++v) {
            if (own[v]) {
                double w[3], nu[3], n0, a, gt, gx, gy;
                stepb(st, p, opx, opy[v], ox, oy[v], mo[v], w, n0, a, gt, gx, gy, nu);
                if (mine) {
                    const uint32_t o = in_loop(oob[v]);
                    const int64_t pb = uniform64(p * nxy + org);
                    __builtin_nontemporal_store(nu[0], byte_at(nut + pb, o));
                    __builtin_nontemporal_store(nu[1], byte_at(nux + pb, o));
                    __builtin_nontemporal_store(nu[2], byte_at(nuy + pb, o));
                    const double gg = gx * gx + gy * gy;
                    num += n0 * fabs(gt + 0.5 * gg);
                    den += n0 * gg;
                    wb[p & 1][0][opy[v] * PR_PW + opx] = w[1];
                    wb[p & 1][1][opy[v] * PR_PW + opx] = w[2];
                }
                wtn[v] = w[0];
                if (!ST) {   // (F of a boundary plane: never next to a steady one)
                    bcm_n[v] = n0;
                    bcq_n[v] = a;
                }
            }
        }
        if (hal && mine) {
            double w[3], nu[3], n0, a, gt, gx, gy;
            stepb(st, p, hpx, hpy, hx, hy, mh, w, n0, a, gt, gx, gy, nu);
            wb[p & 1][0][hpy * PR_PW + hpx] = w[1];
            wb[p & 1][1][hpy * PR_PW + hpx] = w[2];
        }
    };
    // iteration p of the march: mu(p) in (mc, hc); mu(p + 1) into (mn, hn)
    auto step = [&](auto st, int p, const double (&mc)[PR_VPT][3], const double (&hc)[3], double (&mn)[PR_VPT][3],
                    double (&hn)[3]) {
        constexpr bool ST = decltype(st)::value;
        double rc[PR_VPT];
#pragma unroll
        for (int v = 0; v < PR_VPT; ++v) rc[v] = 0.0;
        if (!ST) load_rho(p - 1, rc);
        store_phi(p + 2);   // slot (p+2) & 3 = (p-2) & 3: last read by iteration p-1
        load_phi_to(st, p + 3, fv);
        load_mu(st, p + 1, mn, hn);
        if (ST || p <= pz) plane(st, p, mc, hc);
        else {
#pragma unroll
            for (int v = 0; v < PR_VPT; ++v) wtn[v] = 0.0;   // t0 + p = Nt: F(Nt - 1) reads no w_t(Nt)
        }
        const int n = p - 1, tn = t0 + n;
        const bool deferred = (defer_lo && n == 0) || (defer_hi && n == nl - 1);   // k_rhs_edge's
#pragma unroll
        for (int v = 0; v < PR_VPT; ++v) {
            if (EDGE && own[v] && n >= l0) {
                // what k_rhs_edge needs next to a deferred edge, from the values F(n) would use: w_t
                // of the two outermost planes, and (w_x, w_y, mu'_t, q_t) of the edge plane itself
                // (wt_pre: k_wt_pre wrote the edge planes' w_t, which may be on the wire already)
                if (((defer_lo && n <= 1) || (defer_hi && n >= nl - 2)) && !(wt_pre && deferred))
                    wt_out[n * nxy + ooff[v]] = wtc[v];
                if (deferred) {   // slot 0: plane 0, slot 1: plane nloc - 1 (nloc = 1: both)
                    const int ci = opy[v] * PR_PW + opx;
                    double* E = edge + ooff[v] + ((defer_lo && n == 0) ? 0 : 4 * nxy);
                    E[0] = wb[n & 1][0][ci];
                    E[nxy] = wb[n & 1][1][ci];
                    E[2 * nxy] = bcm[v];
                    E[3 * nxy] = bcq[v];
                    if (defer_lo && defer_hi && nl == 1) {
                        E[4 * nxy] = E[0];
                        E[5 * nxy] = E[nxy];
                        E[6 * nxy] = bcm[v];
                        E[7 * nxy] = bcq[v];
                    }
                }
            }
            if (own[v] && (ST || n >= l0) && !deferred) {
                // F(n) (k_rhs's order: t, x, y terms, then the boundary-plane corrections)
                const double* WX = wb[n & 1][0];
                const double* WY = wb[n & 1][1];
                const int ci = opy[v] * PR_PW + opx;
                const int yv = oy[v];
                double s = 0.0;
                if (ST) {   // 0 < tn < Nt - 1: acc_d1w's interior case
                    s += -0.5 * wtm[v];
                    s += 0.5 * wtn[v];
                } else {
                    acc_d1w(s, tn, Nt, wtm[v], wtc[v], wtn[v]);
                }
                acc_d1w(s, ox, Nx, (INTERIOR || ox > 0) ? WX[ci - 1] : 0.0, WX[ci],
                        (INTERIOR || ox < Nx - 1) ? WX[ci + 1] : 0.0);
                acc_d1w(s, yv, Ny, (INTERIOR || yv > 0) ? WY[ci - PR_PW] : 0.0, WY[ci],
                        (INTERIOR || yv < Ny - 1) ? WY[ci + PR_PW] : 0.0);
                if (!ST && tn == 0) s -= (rc[v] - bcm[v]) + r * bcq[v];        // rho0
                if (!ST && tn == Nt - 1) s += (rc[v] - bcm[v]) + r * bcq[v];   // rhoT
                *byte_at(F + uniform64(n * nxy + org), in_loop(oob[v])) = s;
                ff += s * s;
            }
            wtm[v] = wtc[v];
            wtc[v] = wtn[v];
            if (!ST) {
                bcm[v] = bcm_n[v];
                bcq[v] = bcq_n[v];
            }
        }
        __syncthreads();
    };
    // mu one plane ahead: two register sets.  The steady planes alternate between them; the other
    // planes keep theirs in (mA, hA) by copying
    double mA[PR_VPT][3], hA[3] = {0.0, 0.0, 0.0}, mB[PR_VPT][3], hB[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int v = 0; v < PR_VPT; ++v) mA[v][0] = mA[v][1] = mA[v][2] = mB[v][0] = mB[v][1] = mB[v][2] = 0.0;
    const std::false_type any_plane{};
    const std::true_type steady{};
    // prologue: phi planes pa-1 .. pa+1 in the ring, phi(pa+2) and mu(pa) in flight
    {   // every prologue load in flight before the first LDS store
        double f0[PR_FR], f1[PR_FR], f2[PR_FR];
        load_phi_to(any_plane, pa - 1, f0);
        load_phi_to(any_plane, pa, f1);
        load_phi_to(any_plane, pa + 1, f2);
        load_phi_to(any_plane, pa + 2, fv);
        load_mu(any_plane, pa, mA, hA);
        store_phi_from(pa - 1, f0);   // (pa = 0: plane -1 is never read)
        store_phi_from(pa, f1);
        store_phi_from(pa + 1, f2);
    }
    __syncthreads();
    // Iterations pa .. l1 in order, each once: the planes before the steady ones, the steady ones,
    // the planes after them (tests/test_gpu_prox_march.py restates the bounds and checks them).
    // BARRIERS: one per iteration, at the end of step(), outside every branch of it; pa, ps, pe,
    // l1 and `last` derive from the kernel arguments and the block's chunk alone, so the eight
    // waves of a block run the same iterations and the same number of barriers, and nothing
    // returns between the first barrier and the last.
    // STEADY planes p in [ps, pe]: p and p - 1 are own planes of the chunk (mu' and F(p - 1) are
    // stored: four stores per own voxel, inside no branch), p - 1 and p are no boundary planes (no
    // rho, both t neighbours), p + 1 <= pz and p + 3 is in the grid (every load issued).  With
    // nothing of the iteration under a wave-level branch but the ring voxels -- loaded before the
    // own voxels for that reason -- the compiler counts the step's memory operations: the waits
    // for the loads of the iteration before leave the stores behind them in flight (s_waitcnt
    // vmcnt(7) before the phi ring store, vmcnt(9..7) before stepB on an interior tile, where the
    // general iteration drains them with vmcnt(0) every plane; a bounded tile's stores sit under
    // its lane masks and still drain), and the two register sets alternate without a copy of a
    // loaded value.  The first steady plane stands before the loop of pairs, so that the loop is
    // entered in the state its back edge leaves; a steady-able plane left over by the pairs runs
    // the general iteration.
    int p = pa;
#pragma nounroll
    for (int part = 0; part < 2; ++part) {
        const int last = part == 0 ? min(ps - 1, l1) : l1;
        for (; p <= last; ++p) {
            double cm[PR_VPT][3];
#pragma unroll
            for (int v = 0; v < PR_VPT; ++v) {
                cm[v][0] = mA[v][0];
                cm[v][1] = mA[v][1];
                cm[v][2] = mA[v][2];
            }
            const double chm[3] = {hA[0], hA[1], hA[2]};   // mu(p)
            step(any_plane, p, cm, chm, mA, hA);
        }
        if constexpr (!EDGE) {
            if (part == 0 && p <= pe) {
                step(steady, p, mA, hA, mB, hB);
                for (++p; p + 1 <= pe; p += 2) {
                    step(steady, p, mB, hB, mA, hA);
                    step(steady, p + 1, mA, hA, mB, hB);
                }
#pragma unroll
                for (int v = 0; v < PR_VPT; ++v) {
                    mA[v][0] = mB[v][0];
                    mA[v][1] = mB[v][1];
                    mA[v][2] = mB[v][2];
                    // (no steady plane is a boundary plane or next to one: not carried across them)
                    bcm[v] = bcq[v] = bcm_n[v] = bcq_n[v] = 0.0;
                }
                hA[0] = hB[0];
                hA[1] = hB[1];
                hA[2] = hB[2];
            }
        }
    }
    num_out = num;
    den_out = den;
    ff_out = ff;
}

template <bool EDGE>
__global__ __launch_bounds__(PR_NT) __attribute__((amdgpu_waves_per_eu(PR_WPE))) void k_prox_rhs(
        Geo g, const double* __restrict__ phi, const double* __restrict__ mut, const double* __restrict__ mux,
        const double* __restrict__ muy, double* __restrict__ nut, double* __restrict__ nux, double* __restrict__ nuy,
        const double* __restrict__ rho0, const double* __restrict__ rhoT, double r, double inv_r,
        double* __restrict__ F, RedBuf rb, double* gath_crit, double* gath_rr, const int* __restrict__ guard, int tch,
        int defer_lo, int defer_hi, double* __restrict__ wt_out, double* __restrict__ edge, double* hcrit,
        int wt_pre) {
    if (guard && *guard == 0) return;
    __shared__ double fr[4][PR_FN];                  // phi ring (plane p in slot p & 3)
    __shared__ double wb[2][2][PR_PH * PR_PW];       // [plane & 1][x | y part] of w
    const int Nx = g.Nx, Ny = g.Ny;
    const int ntx = (Nx + PR_X - 1) / PR_X, ntiles = ntx * ((Ny + PR_Y - 1) / PR_Y);
    const int lin = xcd_tile(blockIdx.x);
    const int ch = lin / ntiles, tile = lin - ch * ntiles;
    const int x0 = (tile % ntx) * PR_X, y0 = (tile / ntx) * PR_Y;
    double num, den, ff;
    // tiles whose phi region lies inside the plane run a copy of the march without bound tests
    if (x0 >= 2 && x0 + PR_X + 2 <= Nx && y0 >= 2 && y0 + PR_Y + 2 <= Ny)
        prox_rhs_body<EDGE, true>(g, phi, mut, mux, muy, nut, nux, nuy, rho0, rhoT, r, inv_r, F, tch, defer_lo,
                                  defer_hi, wt_out, edge, wt_pre, fr, wb, ch, x0, y0, num, den, ff);
    else
        prox_rhs_body<EDGE, false>(g, phi, mut, mux, muy, nut, nux, nuy, rho0, rhoT, r, inv_r, F, tch, defer_lo,
                                   defer_hi, wt_out, edge, wt_pre, fr, wb, ch, x0, y0, num, den, ff);
    double v[3] = {num, den, ff}, tot[3];
    if (grid_reduce_last<3, PR_NT>(v, rb, tot) && threadIdx.x == 0) {   // (this rank's slots)
        gath_crit[0] = tot[0];
        gath_crit[1] = tot[1];
        if (gath_rr) gath_rr[0] = tot[2];
        if (hcrit) {   // (pinned, coherent host slot: the crit readback without a copy launch)
            hcrit[0] = tot[0];
            hcrit[1] = tot[1];
            __threadfence_system();
        }
    }
}

// planes per chunk: the configured count (Tuning::pr_tch, FOTO_PR_TCH; default 16), at most the
// slab.  Measured at 640x480x32 (MI355X, 2 blocks of 512 threads per CU): 4 / 8 / 16 / 32 planes
// -> 232 / 195 / 173 / 193 us (more chunks: more recomputed boundary planes; fewer: a partly
// filled last round of blocks).
static int prox_rhs_tch(const Geo& g, int tch) { return std::min(tch, g.nloc); }

int prox_rhs_blocks(const Geo& g, int tch) {
    tch = prox_rhs_tch(g, tch);
    return ((g.Nx + PR_X - 1) / PR_X) * ((g.Ny + PR_Y - 1) / PR_Y) * ((g.nloc + tch - 1) / tch);
}

bool prox_rhs_fits(const Geo& g) { return 8 * ((int64_t)PR_FH * g.Nx + PR_FW) <= (int64_t)UINT32_MAX; }

hipError_t launch_prox_rhs(const Geo& g, const double* phi, const double* mut, const double* mux, const double* muy,
                           double* nut, double* nux, double* nuy, const double* rho0, const double* rhoT, double r,
                           double* F, RedBuf rb, double* gath_crit, double* gath_rr, int tch, hipStream_t s,
                           const int* guard, int defer_lo, int defer_hi, double* wt_out, double* edge, double* hcrit,
                           int wt_pre) {
    const int nb = prox_rhs_blocks(g, tch);
    if (rb.cap < 3 * nb) return hipErrorInvalidValue;
    if (!prox_rhs_fits(g)) return hipErrorInvalidValue;
    if ((defer_lo || defer_hi) && (!wt_out || !edge)) return hipErrorInvalidValue;
    if (defer_lo || defer_hi)
        k_prox_rhs<true><<<nb, PR_NT, 0, s>>>(g, phi, mut, mux, muy, nut, nux, nuy, rho0, rhoT, r, 1.0 / r, F, rb,
                                              gath_crit, gath_rr, guard, prox_rhs_tch(g, tch), defer_lo, defer_hi, wt_out, edge,
                                              hcrit, wt_pre);
    else
        k_prox_rhs<false><<<nb, PR_NT, 0, s>>>(g, phi, mut, mux, muy, nut, nux, nuy, rho0, rhoT, r, 1.0 / r, F, rb,
                                               gath_crit, gath_rr, guard, prox_rhs_tch(g, tch), 0, 0, nullptr, nullptr,
                                               hcrit, 0);
    return hipGetLastError();
}

// (round 5) w_t of a shard's deferred edge planes before k_prox_rhs: per voxel k_prox's stepB
// (the fused kernel's stepb, same operations in the same order, out-of-grid neighbours 0.0 as
// its LDS image holds them), so the w_t plane each neighbour needs can be on the wire while
// k_prox_rhs runs (foto_bb.cpp prox_rhs / wt_overlap).  blockIdx.y: plane pa, then pb.
__global__ __launch_bounds__(NT) void k_wt_pre(Geo g, int pa, int pb, const double* __restrict__ phi,
                                               const double* __restrict__ mut, const double* __restrict__ mux,
                                               const double* __restrict__ muy, double r, double inv_r,
                                               double* __restrict__ wt, const int* __restrict__ guard) {
    if (guard && *guard == 0) return;
    const int64_t nxy = g.nxy;
    const int64_t off = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (off >= nxy) return;
    const int p = blockIdx.y == 0 ? pa : pb;
    const int y = (int)(off / g.Nx), x = (int)(off - (int64_t)y * g.Nx), t = g.t0 + p;
    const int64_t i = (int64_t)p * nxy + off;
    const double c = phi[i];
    const double tm = t > 0 ? phi[i - nxy] : 0.0, tp = t < g.Nt - 1 ? phi[i + nxy] : 0.0;
    const double gt = d1w(t, g.Nt, tm, c, tp);
    const double gx = d1w(x, g.Nx, x > 0 ? phi[i - 1] : 0.0, c, x < g.Nx - 1 ? phi[i + 1] : 0.0);
    const double gy = d1w(y, g.Ny, y > 0 ? phi[i - g.Nx] : 0.0, c, y < g.Ny - 1 ? phi[i + g.Nx] : 0.0);
    const double m0 = mut[i], m1 = mux[i], m2 = muy[i];
    double a, b1, b2;
    project_K(gt + inv_r * m0, gx + inv_r * m1, gy + inv_r * m2, a, b1, b2);
    double n0 = m0 + r * (gt - a);
    n0 = (n0 < 0.0) ? 0.0 : n0;
    wt[i] = n0 - r * a;
}

hipError_t launch_wt_pre(const Geo& g, const double* phi, const double* mut, const double* mux, const double* muy,
                         double r, double* wt, int defer_lo, int defer_hi, hipStream_t s, const int* guard) {
    if (!defer_lo && !defer_hi) return hipSuccess;
    const int pa = defer_lo ? 0 : g.nloc - 1, pb = g.nloc - 1;
    const int np = (defer_lo && defer_hi && g.nloc > 1) ? 2 : 1;
    k_wt_pre<<<dim3((unsigned)flat_blocks(g.nxy), np), NT, 0, s>>>(g, pa, pb, phi, mut, mux, muy, r, 1.0 / r, wt,
                                                                  guard);
    return hipGetLastError();
}

// F on a deferred edge plane of a shard (local plane n = 0 or nloc - 1) from what k_prox_rhs
// stored there and the neighbour's w_t plane (exchanged into wt's halo): k_prox_rhs's F code
// -- t, x, y terms, then the boundary corrections, in the same order -- so F is bit-identical
// to the single-shard kernel's.  F.F of the plane is added to gath_rr[0] (stencil CG).
__global__ __launch_bounds__(NT) void k_rhs_edge(Geo g, int n, const double* __restrict__ wt,
                                                 const double* __restrict__ E, const double* __restrict__ rho0,
                                                 const double* __restrict__ rhoT, double r, double* __restrict__ F,
                                                 RedBuf rb, double* gath_rr, const int* __restrict__ guard) {
    if (guard && *guard == 0) return;
    const int64_t nxy = g.nxy;
    const int64_t off = (int64_t)blockIdx.x * NT + threadIdx.x;
    double ff = 0.0;
    if (off < nxy) {
        const int y = (int)(off / g.Nx), x = (int)(off - (int64_t)y * g.Nx), tn = g.t0 + n;
        const double* WX = E;
        const double* WY = E + nxy;
        const int64_t i = (int64_t)n * nxy + off;
        double s = 0.0;
        acc_d1w(s, tn, g.Nt, wt[i - nxy], wt[i], wt[i + nxy]);
        acc_d1w(s, x, g.Nx, x > 0 ? WX[off - 1] : 0.0, WX[off], x < g.Nx - 1 ? WX[off + 1] : 0.0);
        acc_d1w(s, y, g.Ny, y > 0 ? WY[off - g.Nx] : 0.0, WY[off], y < g.Ny - 1 ? WY[off + g.Nx] : 0.0);
        const double bcm = E[2 * nxy + off], bcq = E[3 * nxy + off];
        if (tn == 0) s -= (rho0[off] - bcm) + r * bcq;
        if (tn == g.Nt - 1) s += (rhoT[off] - bcm) + r * bcq;
        F[i] = s;
        ff = s * s;
    }
    if (!gath_rr) return;
    double v[1] = {ff}, tot[1];
    if (grid_reduce_last<1>(v, rb, tot) && threadIdx.x == 0) gath_rr[0] += tot[0];
}

hipError_t launch_rhs_edge(const Geo& g, int n, const double* wt, const double* edge, const double* rho0,
                           const double* rhoT, double r, double* F, RedBuf rb, double* gath_rr, hipStream_t s,
                           const int* guard) {
    if (n < 0 || n >= g.nloc) return hipErrorInvalidValue;
    k_rhs_edge<<<flat_blocks(g.nxy), NT, 0, s>>>(g, n, wt, edge, rho0, rhoT, r, F, rb, gath_rr, guard);
    return hipGetLastError();
}

// ============================================================================ 2-D operators

// grad_1d_central (operators.py:52-65): bc 'N' end rows zero; bc 'D' zero extension.
__device__ __forceinline__ double d1c(int k, int n, double m, double p, int bcD) {
    if (k == 0) return bcD ? 0.5 * p : 0.0;
    if (k == n - 1) return bcD ? -0.5 * m : 0.0;
    return 0.5 * (p - m);
}

__global__ __launch_bounds__(NT) void k_grad2(int Nx, int Ny, const double* __restrict__ f, double* __restrict__ gx,
                                              double* __restrict__ gy, int bcD) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= (int64_t)Nx * Ny) return;
    const int y = (int)(i / Nx), x = (int)(i - (int64_t)y * Nx);
    gx[i] = d1c(x, Nx, x > 0 ? f[i - 1] : 0.0, x < Nx - 1 ? f[i + 1] : 0.0, bcD);
    gy[i] = d1c(y, Ny, y > 0 ? f[i - Nx] : 0.0, y < Ny - 1 ? f[i + Nx] : 0.0, bcD);
}

hipError_t launch_grad2(int Nx, int Ny, const double* f, double* gx, double* gy, int bcD, hipStream_t s) {
    k_grad2<<<flat_blocks((int64_t)Nx * Ny), NT, 0, s>>>(Nx, Ny, f, gx, gy, bcD);
    return hipGetLastError();
}

// operators.div (operators.py:182-191) row, COO order: x-block terms then y-block terms.
__device__ __forceinline__ void acc_d1c(double& s, int k, int n, double m, double p, int bcD) {
    if (k == 0) { if (bcD) s += 0.5 * p; }
    else if (k == n - 1) { if (bcD) s += -0.5 * m; }
    else { s += -0.5 * m; s += 0.5 * p; }
}

__global__ __launch_bounds__(NT) void k_div2(int Nx, int Ny, const double* __restrict__ u, const double* __restrict__ v,
                                             double* __restrict__ out, int bcD, double sign) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= (int64_t)Nx * Ny) return;
    const int y = (int)(i / Nx), x = (int)(i - (int64_t)y * Nx);
    double s = 0.0;
    acc_d1c(s, x, Nx, x > 0 ? u[i - 1] : 0.0, x < Nx - 1 ? u[i + 1] : 0.0, bcD);
    acc_d1c(s, y, Ny, y > 0 ? v[i - Nx] : 0.0, y < Ny - 1 ? v[i + Nx] : 0.0, bcD);
    out[i] = sign * s;
}

hipError_t launch_div2(int Nx, int Ny, const double* u, const double* v, double* out, int bcD, double sign,
                       hipStream_t s) {
    k_div2<<<flat_blocks((int64_t)Nx * Ny), NT, 0, s>>>(Nx, Ny, u, v, out, bcD, sign);
    return hipGetLastError();
}

// grad_forward bc 'N' (operators.py:67-79, 171-180): z[k+1] - z[k], last row 0.
__global__ __launch_bounds__(NT) void k_grad2_fwd(int Nx, int Ny, const double* __restrict__ f,
                                                  double* __restrict__ gx, double* __restrict__ gy) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= (int64_t)Nx * Ny) return;
    const int y = (int)(i / Nx), x = (int)(i - (int64_t)y * Nx);
    gx[i] = (x < Nx - 1) ? -1.0 * f[i] + 1.0 * f[i + 1] : 0.0;
    gy[i] = (y < Ny - 1) ? -1.0 * f[i] + 1.0 * f[i + Nx] : 0.0;
}

hipError_t launch_grad2_forward(int Nx, int Ny, const double* f, double* gx, double* gy, hipStream_t s) {
    k_grad2_fwd<<<flat_blocks((int64_t)Nx * Ny), NT, 0, s>>>(Nx, Ny, f, gx, gy);
    return hipGetLastError();
}

// ============================================================================ flow extraction (A13/A14)

// reconstructTrajectory (utils.py:44-99) for steps n in [n_lo, n_hi), one thread per pixel.
__global__ __launch_bounds__(NT) void k_traj(Geo g, const double* __restrict__ phi, int n_lo, int n_hi,
                                             double* __restrict__ px, double* __restrict__ py, int init) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= g.nxy) return;
    const int Nx = g.Nx, Ny = g.Ny;
    const int j = (int)(i / Nx), ii = (int)(i - (int64_t)j * Nx);
    double x = init ? (double)ii : px[i];
    double y = init ? (double)j : py[i];
    for (int n = n_lo; n < n_hi; ++n) traj_step(phi + (int64_t)(n - g.t0) * g.nxy, Nx, Ny, x, y);
    px[i] = x;
    py[i] = y;
}

hipError_t launch_traj(const Geo& g, const double* phi, int n_lo, int n_hi, double* px, double* py, int init,
                       hipStream_t s) {
    k_traj<<<flat_blocks(g.nxy), NT, 0, s>>>(g, phi, n_lo, n_hi, px, py, init);
    return hipGetLastError();
}

// One flow record from the positions: u = px - x, v = py - y, m = -div(bc 'D') [u; v] (k_div2's
// sum, sign -1.0; the neighbours' u, v are the same subtractions) and the export, in float64;
// only the stores round (float32).  LAYOUT 0: three planes; 1: interleaved (u, v).
template <class T, int LAYOUT>
__global__ __launch_bounds__(NT) void k_flow_record(int Nx, int Ny, const double* __restrict__ px,
                                                    const double* __restrict__ py, T* __restrict__ ou,
                                                    T* __restrict__ ov, T* __restrict__ om) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= (int64_t)Nx * Ny) return;
    const int y = (int)(i / Nx), x = (int)(i - (int64_t)y * Nx);
    const double u = px[i] - (double)x;
    const double v = py[i] - (double)y;
    if (LAYOUT == 1) {
        ou[2 * i] = (T)u;
        ou[2 * i + 1] = (T)v;
        return;
    }
    double s = 0.0;
    acc_d1c(s, x, Nx, x > 0 ? px[i - 1] - (double)(x - 1) : 0.0, x < Nx - 1 ? px[i + 1] - (double)(x + 1) : 0.0, 1);
    acc_d1c(s, y, Ny, y > 0 ? py[i - Nx] - (double)(y - 1) : 0.0, y < Ny - 1 ? py[i + Nx] - (double)(y + 1) : 0.0, 1);
    ou[i] = (T)u;
    ov[i] = (T)v;
    om[i] = (T)(-1.0 * s);
}

template <class T>
static hipError_t flow_record_t(int Nx, int Ny, const double* px, const double* py, void* ou, void* ov, void* om,
                                int layout, hipStream_t s) {
    const int nb = flat_blocks((int64_t)Nx * Ny);
    if (layout == 0) k_flow_record<T, 0><<<nb, NT, 0, s>>>(Nx, Ny, px, py, (T*)ou, (T*)ov, (T*)om);
    else k_flow_record<T, 1><<<nb, NT, 0, s>>>(Nx, Ny, px, py, (T*)ou, (T*)ov, (T*)om);
    return hipGetLastError();
}

hipError_t launch_flow_record(int Nx, int Ny, const double* px, const double* py, void* ou, void* ov, void* om,
                              int dtype, int layout, hipStream_t s) {
    if (layout != 0 && layout != 1) return hipErrorInvalidValue;
    if (dtype == FOTO_F32) return flow_record_t<float>(Nx, Ny, px, py, ou, ov, om, layout, s);
    if (dtype == FOTO_F64) return flow_record_t<double>(Nx, Ny, px, py, ou, ov, om, layout, s);
    return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------- point tracking
// reconstructTrajectory (utils.py:44-99) from arbitrary start points, one thread per point, for
// the steps n in [n_lo, n_hi) of one base pointer; the position stays in registers (float64)
// from step to step.  A step is k_traj's (traj_step, foto_devutil.h): every load is inside the
// plane whatever the point, a non-finite point gives a non-finite record and nothing else.
// Record n (after step n) is the displacement from the start point, one 16-byte (float64) or
// 8-byte (float32) store per thread, contiguous across the wave; ALL = 0 stores the record of
// step Nt-2 only.  pos_in (may be null: the start points) / pos_out (may be null) carry the
// running float64 positions between the launches of a path whose planes lie in several buffers
// (they may be the same buffer: a thread reads its own pair before the loop and writes it after).
template <class T> struct Pair2;
template <> struct Pair2<float> { using type = float2; };
template <> struct Pair2<double> { using type = double2; };

template <class TI, class TO, int ALL>
__global__ __launch_bounds__(NT) void k_track(Geo g, const double* __restrict__ phi, int n_lo, int n_hi,
                                              const TI* __restrict__ pts, const double* pos_in, double* pos_out,
                                              TO* __restrict__ out, int64_t M) {
    using VI = typename Pair2<TI>::type;
    using VO = typename Pair2<TO>::type;
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= M) return;
    const int Nx = g.Nx, Ny = g.Ny;
    const VI p0 = reinterpret_cast<const VI*>(pts)[i];
    const double x0 = (double)p0.x, y0 = (double)p0.y;
    double x = x0, y = y0;
    if (pos_in) {
        const double2 q = reinterpret_cast<const double2*>(pos_in)[i];
        x = q.x;
        y = q.y;
    }
    VO* const rec = reinterpret_cast<VO*>(out);
    for (int n = n_lo; n < n_hi; ++n) {
        traj_step(phi + (int64_t)(n - g.t0) * g.nxy, Nx, Ny, x, y);
        if (ALL || n == g.Nt - 2) {
            VO r;
            r.x = (TO)(x - x0);
            r.y = (TO)(y - y0);
            rec[(ALL ? (int64_t)n * M : 0) + i] = r;
        }
    }
    if (pos_out) reinterpret_cast<double2*>(pos_out)[i] = make_double2(x, y);
}

template <class TI, class TO>
static hipError_t track_t(const Geo& g, const double* phi, int n_lo, int n_hi, const void* pts, const double* pos_in,
                          double* pos_out, void* out, int64_t M, int all_steps, hipStream_t s) {
    const int nb = flat_blocks(M);
    if (all_steps)
        k_track<TI, TO, 1><<<nb, NT, 0, s>>>(g, phi, n_lo, n_hi, (const TI*)pts, pos_in, pos_out, (TO*)out, M);
    else
        k_track<TI, TO, 0><<<nb, NT, 0, s>>>(g, phi, n_lo, n_hi, (const TI*)pts, pos_in, pos_out, (TO*)out, M);
    return hipGetLastError();
}

hipError_t launch_track(const Geo& g, const double* phi, int n_lo, int n_hi, const void* pts, int pts_dtype,
                        const double* pos_in, double* pos_out, void* out, int dtype, int64_t M, int all_steps,
                        hipStream_t s) {
    if (M < 1 || M > INT32_MAX || g.Nx < 2 || g.Ny < 2) return hipErrorInvalidValue;
    if (n_lo < g.t0 || n_hi > g.t0 + g.nloc || n_hi > g.Nt - 1) return hipErrorInvalidValue;
    if (n_lo >= n_hi) return hipSuccess;
    const bool i32 = pts_dtype == FOTO_F32, o32 = dtype == FOTO_F32;
    if ((!i32 && pts_dtype != FOTO_F64) || (!o32 && dtype != FOTO_F64)) return hipErrorInvalidValue;
    if (i32 && o32) return track_t<float, float>(g, phi, n_lo, n_hi, pts, pos_in, pos_out, out, M, all_steps, s);
    if (i32) return track_t<float, double>(g, phi, n_lo, n_hi, pts, pos_in, pos_out, out, M, all_steps, s);
    if (o32) return track_t<double, float>(g, phi, n_lo, n_hi, pts, pos_in, pos_out, out, M, all_steps, s);
    return track_t<double, double>(g, phi, n_lo, n_hi, pts, pos_in, pos_out, out, M, all_steps, s);
}

}  // namespace foto

namespace foto {

// x.x partial sums -> gath[rank] (used to seed CG with b.b when b comes from the host)
__global__ __launch_bounds__(NT) void k_dot_self(int64_t n, const double* __restrict__ x, RedBuf rb, double* gath,
                                                 int rank) {
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) acc += x[i] * x[i];
    double v[1] = {acc}, tot[1];
    if (grid_reduce_last<1>(v, rb, tot) && threadIdx.x == 0) gath[rank] = tot[0];
}

hipError_t launch_dot_self(int64_t n, const double* x, RedBuf rb, double* gath, int rank, hipStream_t s) {
    int nb = (int)std::min<int64_t>((n + NT - 1) / NT, 2048);
    k_dot_self<<<nb, NT, 0, s>>>(n, x, rb, gath, rank);
    return hipGetLastError();
}

}  // namespace foto
