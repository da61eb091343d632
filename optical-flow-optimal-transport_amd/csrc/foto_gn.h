// What foto_gn.hip shares with the coarse-to-fine driver (foto_gn_pyr.hip): the per-pixel stencil
// algebra of the GN operator and the plan's internal entry points.
#pragma once

#include "foto_internal.h"

namespace foto {

// ----------------------------------------------------------------------------- operator stencil

struct GNPix {
    int x, y;
    bool hy, hx, hX, hY;
    double c;   // neighbour count = diagonal of G^T G
};

__device__ __forceinline__ GNPix gn_pix(int w, int h, int64_t i) {
    GNPix P;
    // 32-bit division (w h < 2^31): the 64-bit one is a long software sequence per pixel
    P.y = (int)((unsigned)i / (unsigned)w);
    P.x = (int)i - P.y * w;
    P.hy = P.y > 0; P.hY = P.y < h - 1; P.hx = P.x > 0; P.hX = P.x < w - 1;
    P.c = (double)((int)P.hy + (int)P.hY + (int)P.hx + (int)P.hX);
    return P;
}

// The five stencil indices of pixel i in CSR order: (y-1), (x-1), centre, (x+1), (y+1).  A missing
// neighbour is fetched at the centre's index (clamped) and skipped by a select in gn_lap_row:
// with the fetches behind branches every neighbour was its own memory round trip (~25 us per
// PCG kernel at 640x480).
__device__ __forceinline__ void gn_idx5(const GNPix& P, int w, int64_t i, int64_t (&j)[5]) {
    j[0] = P.hy ? i - w : i; j[1] = P.hx ? i - 1 : i; j[2] = i; j[3] = P.hX ? i + 1 : i; j[4] = P.hY ? i + w : i;
}

// v[f][k] = val(f, j_k): the stencil values of all three fields at pixel i
template <class F>
__device__ __forceinline__ void gn_gather5(const GNPix& P, int w, int64_t i, F val, double (&v)[3][5]) {
    int64_t j[5];
    gn_idx5(P, w, i, j);
#pragma unroll
    for (int f = 0; f < 3; ++f)
#pragma unroll
        for (int k = 0; k < 5; ++k) v[f][k] = val(f, j[k]);
}

// one field's Laplacian block row in CSR order over its five fetched values val(k)
template <class F>
__device__ __forceinline__ double gn_lap_row(const GNPix& P, double coef, double dg, F val, double s) {
    const double m = -coef;
    s = P.hy ? s + m * val(0) : s;
    s = P.hx ? s + m * val(1) : s;
    s += dg * val(2);
    s = P.hX ? s + m * val(3) : s;
    s = P.hY ? s + m * val(4) : s;
    return s;
}

// ----------------------------------------------------------------------------- the plan, for the pyramid

// b -= [alpha N u0; alpha N v0; lambda N m0], N = -Lambda2 as gn_lap_row applies it (foto_gn_pyr.hip)
hipError_t launch_gn_rhs_prior(int w, int h, double alpha, double lam, const double* x0, double* b, hipStream_t s);
// x[i] += x0[i], i < n (foto_gn_pyr.hip)
hipError_t launch_gn_add(int64_t n, double* x, const double* x0, hipStream_t s);

// The pyramid's grid transfers (foto_gn_pyr.hip), shared with the TV-L1 solver (foto_tvl1.hip):
// both frames of a w x h level restricted to ceil(w/2) x ceil(h/2); [3][wc hc] = u, v, m prolonged
// to [3][w h] with the displacement scales (m unscaled)
hipError_t launch_pyr_down(int w, int h, const double* f1, const double* f2, double* c1, double* c2, hipStream_t s);
hipError_t launch_pyr_up(int wc, int hc, int w, int h, const double* c, double* o, hipStream_t s);

// foto_gn_plan_create's plan on `shared` (null: a stream of its own): the pyramid's plans run on
// the pyramid's one stream, which the plan then neither synchronises for others nor releases
int gn_plan_make(int w, int h, double alpha, double lam, double rtol, int maxiter, hipStream_t shared,
                 foto_gn_plan** out);

// the plan's buffers a caller of gn_plan_solve_prior fills and reads, all on stream s
struct GnBufs {
    int w, h, device;
    hipStream_t s;
    double *d1, *d2;   // the two frames, w h doubles each
    double* x;         // the solution, [3][w h] = u, v, m
};
GnBufs gn_plan_bufs(foto_gn_plan* P);

// One increment solve, used by the pyramid only: the frames are already in d1 / d2 on the plan's
// stream; x0 is a device prior [3][w h] or null.  gn_setup -> b -= [alpha N u0; alpha N v0;
// lambda N m0] -> gn_run_pcg -> x += x0, so x holds the total flow.  With x0 null this is
// gn_plan_solve between its upload and its download, bit for bit.  *done: the stop test fired.
int gn_plan_solve_prior(foto_gn_plan* P, const double* x0, int* iterations, bool* done);

}  // namespace foto
