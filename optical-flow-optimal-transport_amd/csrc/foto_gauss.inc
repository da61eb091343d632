// Gauss-compressed spectral CG (included by foto_spectral.hip; uses SpecTab, spec_lam, the
// t-column constants and the DPP helpers defined there).
//
// In the DCT-II eigenbasis A is diagonal, so CG from x0 = 0 is a function of the discrete measure
// sigma = sum_i b^_i^2 delta(lam - lam_i) alone: its k-th iterate depends only on the moments of
// sigma up to degree 2k (benamou_brenier.py:85 calls scipy's cg; every quantity it computes --
// rho = r.r, p.Ap, the stop test -- is an integral of a polynomial against sigma).  sigma has
// one point per voxel (9.8 M on the bench grid), but CG only ever integrates polynomials of
// degree <= 2K (K = the iteration count, ~200), and such polynomials are smooth on a fine enough
// partition of the spectrum.  So:
//   1. k_gq_hist: partition theta = acos(lam~) in [0, pi] (lam~ = lam scaled to [-1, 1]) into
//      GQ_NB equal bins and take each bin's first 2 GQ_M Chebyshev moments in its local variable
//      u in [-1, 1]: one read of b^, no other state.
//   2. k_gq_nodes_w: per bin, the GQ_M-point Gauss rule of those moments (modified Chebyshev
//      algorithm -> Jacobi matrix -> eigenvalues by Sturm bisection, Christoffel weights).  A
//      degree-2K polynomial is a trig polynomial of degree 2K in theta; on a bin of width
//      pi / GQ_NB its local Taylor remainder of order 2 GQ_M is (2K pi / 2 GQ_NB)^16 / 16! --
//      the 2048 weighted nodes integrate everything CG computes to ~1e-13 relative
//      (tools/gautschi_proto.py: residual norms within 1.5e-13 of the literal CG for all ~200
//      iterations, the same iteration counts, phi within 2e-14 of scipy's).
//   3. k_gq_cg: scipy's CG recurrence on the 2048-node measure, in one block: alpha_k, beta_k,
//      the stop test norm(r) < rtol norm(b), maxiter.
//   4. k_gq_qtab: x^ = Q(lam) b^ with Q the degree-(K-1) solution polynomial (x after K steps of
//      the scalar recurrence from r = 1).  Q is tabulated as GQ_QN Chebyshev coefficients per
//      theta bin (GQ_QB bins), evaluated at the Chebyshev points of each bin by the recurrence.
//   5. the inverse t-DCT column kernels evaluate Q per voxel from the table in LDS (Clenshaw)
//      and transform x^ back -- x^ never goes to HBM.
// So the Poisson solve costs one read of b^ plus a few microseconds of serial work on a tiny
// measure, instead of ~24 s-step passes over (r^, q^).  The result is the CG iterate (not the
// exact solve): the same iteration count, and the same x up to the literal CG's own rounding.
// If a table cannot represent the solve (K > GQ_KMAX, or a non-positive p.Ap), k_gq_cg says so
// (status) and the host redoes the solve with the s-step CG.

constexpr int GQ_NB = 256;                 // theta bins of the measure
constexpr int GQ_M = 8;                    // Gauss nodes per bin
constexpr int GQ_NM = 2 * GQ_M;            // Chebyshev moments per bin
constexpr int GQ_NODES = GQ_NB * GQ_M;     // compressed measure size
constexpr int GQ_HIST = GQ_NM * GQ_NB;     // doubles per histogram [moment][bin]
// CG steps the solution table covers (beyond: status 2, the s-step CG redoes the solve).  Round 4
// raised it from 512 to 1024: main.py's default reg_epsilon 1e-3 needs K = 640-720 at the bench
// grid, which the compressed measure still integrates to phi 1.3e-11 / crit 8e-12 of the s-step
// CG (K = 580 on a noisy 96x80x16 pair: 1e-9 / 5e-10; tools/kmax_check.py, profiles/r04_kmax.txt)
#ifndef FOTO_GQ_KMAX
#define FOTO_GQ_KMAX 1024
#endif
constexpr int GQ_KMAX = FOTO_GQ_KMAX;
constexpr int GQ_QB = 512;                 // half-bins of the solution table (two per measure bin)
constexpr int GQ_QN = 32;                  // Chebyshev coefficients per table bin
constexpr int GQ_TAB = GQ_QN * GQ_QB;      // [coefficient][bin]
constexpr size_t GQ_TAB_BYTES = sizeof(double) * GQ_TAB;   // [coefficient][half-bin]
constexpr int GQ_CGNTH = 256;              // CG block: GQ_NODES / GQ_CGNTH nodes per thread

struct GqState {
    int K;          // CG iterations (scipy's count)
    int status;     // 0 ok; 1 breakdown (p.Ap <= 0 or not finite); 2 K > GQ_KMAX
    int conv;       // 1 stop test passed, 0 maxiter reached
    int done;       // 1: x is final (guard of the prox launched behind the solve)
    int qn;         // Chebyshev terms of the solution table that matter for this K (<= GQ_QN)
    int broken;     // 1: this or an earlier solve of the chain failed (done stays 0 until the
                    // host, having redone that solve, clears it): with two outer iterations in
                    // flight, the second one's prox must not run behind a failed first solve
    double bn2;     // ||b||^2 (the measure's mass)
    double rn2;     // ||r_K||^2
    double alpha[GQ_KMAX], beta[GQ_KMAX];
};

struct GqNodes {
    double lam[GQ_NODES];
    double w[GQ_NODES];
};

// Bins: GQ_NB equal steps of theta = acos(lam~) in [0, pi] (lam~ = lam scaled to [-1, 1]),
// written in the offset variable s = lam~ + 1 = (lam - r eps) / c1 in [0, 2]: lam - r eps =
// r (mu_t + mu_y + mu_x) is a sum of non-negative terms, so s keeps full relative precision at
// the low end of the spectrum, where the smooth modes (most of b^'s mass) live -- lam~ itself
// is ~ -1 + 1e-4 there and c0 + c1 lam~ loses 1e-13 of lam = r eps.  Bin b holds
// hi[b + 1] < s <= hi[b], hi[b] = 1 + cos(pi b / GQ_NB) = 2 cos^2(pi b / (2 GQ_NB)).  Inside a
// bin the local variable is linear in s: u = (s - mid[b]) / hw[b] in [-1, 1].  (Round 3 first
// used a theta-linear u, one acos per voxel; the lam~-linear u integrates CG's polynomials as
// well -- tools/gauss_lin_proto.py: residual norms within 2.4e-13 of the literal CG, the same
// counts -- and a voxel's bin follows from comparisons with the edges.)  cell[c] is the bin of
// the upper end of s-cell c (GQ_NCELL equal cells of [0, 2]): a lookup plus a short fix-up finds
// any voxel's bin; along a row, whose eigenvalues increase with kx, the bin only steps down.
constexpr int GQ_NCELL = 2048;
struct GqBins {
    double hi[GQ_NB + 2];   // [GQ_NB + 1]: padding (16-B multiple)
    double mid[GQ_NB];
    double hw[GQ_NB];
    double ihw[GQ_NB];
    unsigned char cell[GQ_NCELL];
};
static_assert(GQ_NB <= 256, "bins fit the cell table's bytes");

__global__ __launch_bounds__(256) void k_gq_bins(GqBins* __restrict__ B) {
    __shared__ double hi[GQ_NB + 1];
    for (int b = threadIdx.x; b <= GQ_NB; b += 256)
        hi[b] = (b == GQ_NB) ? 0.0 : 2.0 * cos(M_PI * (double)b / (2 * GQ_NB)) * cos(M_PI * (double)b / (2 * GQ_NB));
    __syncthreads();
    for (int b = threadIdx.x; b <= GQ_NB; b += 256) B->hi[b] = hi[b];
    for (int b = threadIdx.x; b < GQ_NB; b += 256) {
        B->mid[b] = 0.5 * (hi[b] + hi[b + 1]);
        const double hw = 0.5 * (hi[b] - hi[b + 1]);
        B->hw[b] = hw;
        B->ihw[b] = 1.0 / hw;
    }
    for (int c = threadIdx.x; c < GQ_NCELL; c += 256) {
        const double uc = (double)(c + 1) * (2.0 / GQ_NCELL);
        int b = 0;
        while (b < GQ_NB - 1 && hi[b + 1] >= uc) ++b;
        B->cell[c] = (unsigned char)b;
    }
}

// s = (lam - r eps) / c1 from d = r (mu_t + mu_y + mu_x) (spec_lam without its r eps)
__device__ __forceinline__ double gq_s(double d, double ic1) { return fmin(2.0, fmax(0.0, d * ic1)); }

// bin of s from a guess: the edges of bin b are hi[b + 1] < s <= hi[b] (bins 0 and NB - 1
// take the clamped ends)
__device__ __forceinline__ int gq_fix_bin(const double* hi, double lt, int b) {
    while (b > 0 && lt > hi[b]) --b;
    while (b < GQ_NB - 1 && lt <= hi[b + 1]) ++b;
    return b;
}

__device__ __forceinline__ int gq_find_bin(const double* hi, const unsigned char* cell, double lt) {
    const int c = min(GQ_NCELL - 1, max(0, (int)(lt * (0.5 * GQ_NCELL))));
    return gq_fix_bin(hi, lt, cell[c]);
}

// the bin tables into LDS (all threads of the block; followed by a barrier in the caller)
__device__ __forceinline__ void gq_load_bins(GqBins* L, const GqBins* __restrict__ B) {
    static_assert(sizeof(GqBins) % 16 == 0, "dwordx4 copy");
    for (int e = threadIdx.x; e < (int)(sizeof(GqBins) / 16); e += blockDim.x)
        reinterpret_cast<dbl2*>(L)[e] = reinterpret_cast<const dbl2*>(B)[e];
}

__device__ __forceinline__ double gq_uniform_sum(double v) {   // wave total, the same in every lane
    dpp_row_sums(v);
    return ((dbl_readlane(v, 15) + dbl_readlane(v, 31)) + dbl_readlane(v, 47)) + dbl_readlane(v, 63);
}

// ---------------------------------------------------------------------------- 1. histogram (bin order)
// The bin of a voxel depends on its indices only (lam = r eps + r (mu_t + mu_y + mu_x)), so the
// voxels can be grouped by bin once per plan: perm lists the box's voxels bin by bin (rows in
// order inside a bin, kx in order inside a row: the order is fixed, so the sums are
// deterministic), and the per-solve histogram walks that list in chunks of GQ_PCH voxels that
// never straddle a bin.  A wave then works on one bin: no per-voxel bin search, no run flushes,
// no LDS histograms -- its 16 moment sums stay in registers and are reduced across the wave
// (DPP rows, then the four row totals in order) once per chunk.  Entries pack (row, kx) as
// row << GQ_PXB | kx (row = kt nyl + kyl, the box's row index); boxes the packing does not
// cover (Nx > 4096, >= 2^20 rows) run the s-step CG instead.  (Round 3 first binned with a
// row scan into four private 32 KB LDS histograms per block, flushing a lane's run at every
// bin change: 108 us at 640x480x32 against 43 here.)
//
// Exact bins.  A bin holding at most GQ_XS distinct eigenvalues (the spectrum's ends; most
// bins of a small grid) is not compressed: its slots carry the weight sum of each distinct
// eigenvalue instead of Chebyshev moments, and its Gauss rule comes from those points (or is
// them).  The moments of a measure with fewer support points than GQ_M are singular, and the
// modified Chebyshev algorithm's cut-off then decides on rounding noise: a 1e-15 change of the
// moments (the summation order of a sharded run) moved CG counts by up to 7 on a 24x18x5 grid
// (tools/gauss_lin_proto.py's restatement; with exact bins: the oracle's counts every time).
constexpr int GQ_PXB = 12;
// (round 5: 8 x 4 instead of 16 x 2 -- the same voxel order per lane, so the same sums bit for
// bit, at 120 instead of 153 VGPRs: four waves per SIMD, 36.6 -> 35.6 us, profiles/r05_hist_ab.txt)
constexpr int GQ_PE = 8;                   // voxels per lane per batch
constexpr int GQ_PB = 4;                   // batches per chunk (the wave reduction is per chunk)
constexpr int GQ_PCH = 64 * GQ_PE * GQ_PB; // voxels per chunk
struct GqChunk {
    int bin, start, len;
    int id;   // slot of its sums in part[] (the list is in dispatch order; -1: an idle wave)
};

constexpr int GQ_XS = 16;   // exact bins: at most GQ_XS distinct eigenvalues (one hist slot each)
static_assert(GQ_XS <= GQ_NM, "slot weights live in the moment slots");
struct GqExact {
    int n[GQ_NB];                // distinct eigenvalues of the bin; GQ_XS + 1: more (a moment bin)
    double lam[GQ_NB][GQ_XS];    // ascending
    double sv[GQ_NB][GQ_XS];     // their s = (lam - r eps) / c1
    double cut[GQ_NB][GQ_XS];    // cut[j] between lam[j] and lam[j + 1]: slot = #cuts below lam
};

__host__ __device__ inline bool gq_perm_ok(int Nx, int rows) { return Nx <= (1 << GQ_PXB) && rows < (1 << (31 - GQ_PXB)); }

// the box's row sums mu_t + mu_y (spec_lam's rowmu), one per row kt nyl + kyl
__global__ __launch_bounds__(256) void k_gq_rowmu(SpecTab T, double* __restrict__ rowmu) {
    const int R = blockIdx.x * 256 + threadIdx.x;
    if (R >= T.Nt * T.nyl) return;
    const int kt = R / T.nyl, kyl = R - kt * T.nyl;
    rowmu[R] = T.mt[kt] + T.my[T.y0 + kyl];
}

// one thread per row: walk kx (the eigenvalues increase, so the bins step down) and emit each
// run (bin, kx0, len) to f(bin, kx0, len)
template <class F>
__device__ __forceinline__ void gq_row_runs(const SpecTab& T, const GqBins* __restrict__ B, double rowmu, double ic1,
                                            F f) {
    int b = -1, kx0 = 0;
    for (int kx = 0; kx < T.Nx; ++kx) {
        const double lt = gq_s(T.r * (rowmu + T.mx[kx]), ic1);
        const int nb = (b < 0) ? gq_find_bin(B->hi, B->cell, lt) : gq_fix_bin(B->hi, lt, b);
        if (nb != b) {
            if (b >= 0) f(b, kx0, kx - kx0);
            b = nb;
            kx0 = kx;
        }
    }
    if (b >= 0) f(b, kx0, T.Nx - kx0);
}

// cnt[b][R] = voxels of row R in bin b (cnt zeroed by the caller)
__global__ __launch_bounds__(256) void k_gq_perm_count(SpecTab T, const GqBins* __restrict__ B, const double* __restrict__ rowmu,
                                                       double ic1, int* __restrict__ cnt) {
    const int rows = T.Nt * T.nyl;
    const int R = blockIdx.x * 256 + threadIdx.x;
    if (R >= rows) return;
    gq_row_runs(T, B, rowmu[R], ic1, [&](int b, int, int len) { cnt[(int64_t)b * rows + R] += len; });
}

// per bin (one block each): exclusive scan of cnt[b][.] over the rows, in place; tot[b] = the sum
__global__ __launch_bounds__(256) void k_gq_perm_scan(int rows, int* __restrict__ cnt, int* __restrict__ tot) {
    __shared__ int ws[4];
    int* c = cnt + (int64_t)blockIdx.x * rows;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int base = 0;
    for (int r0 = 0; r0 < rows; r0 += 256) {
        const int R = r0 + threadIdx.x;
        const int v = (R < rows) ? c[R] : 0;
        int x = v;   // inclusive wave scan
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63) ws[wv] = x;
        __syncthreads();
        int pre = base;
        for (int q = 0; q < wv; ++q) pre += ws[q];
        const int total = ws[0] + ws[1] + ws[2] + ws[3];
        if (R < rows) c[R] = pre + x - v;
        base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) tot[blockIdx.x] = base;
}

// perm[first[b] + cnt[b][R] + j] = (R, kx of the j-th voxel of row R in bin b)
__global__ __launch_bounds__(256) void k_gq_perm_fill(SpecTab T, const GqBins* __restrict__ B, const double* __restrict__ rowmu,
                                                      double ic1, const int* __restrict__ off,
                                                      const int* __restrict__ first, unsigned* __restrict__ perm) {
    const int rows = T.Nt * T.nyl;
    const int R = blockIdx.x * 256 + threadIdx.x;
    if (R >= rows) return;
    gq_row_runs(T, B, rowmu[R], ic1, [&](int b, int kx0, int len) {
        unsigned* dst = perm + first[b] + off[(int64_t)b * rows + R];
        for (int j = 0; j < len; ++j) dst[j] = ((unsigned)R << GQ_PXB) | (unsigned)(kx0 + j);
    });
}

// one thread per bin: the bin's distinct eigenvalues over the whole grid (perm / first / tot of
// the global box), up to GQ_XS of them; values within 4 ulp are one point (lam = mu sums in
// different association orders, e.g. mu_y[a] + mu_x[b] and mu_y[b] + mu_x[a] on a square grid)
__global__ __launch_bounds__(64) void k_gq_exact(SpecTab T, const unsigned* __restrict__ perm, const int* __restrict__ first,
                                                 const int* __restrict__ tot, const double* __restrict__ rowmu,
                                                 double ic1, int xmax, GqExact* __restrict__ X) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= GQ_NB) return;
    if (xmax < 0) {   // exact bins off (A/B runs)
        X->n[b] = GQ_XS + 1;
        return;
    }
    double v[GQ_XS + 1], vs[GQ_XS + 1];
    int n = 0;
    const int cnt = tot[b];
    // a bin with more than 256 voxels per possible exact point cannot be exact in practice (the
    // eigenvalue sum of three axes repeats a value at most a few times); skip the scan
    if (cnt > 256 * GQ_XS) n = GQ_XS + 1;
    for (int i = 0; i < cnt && n <= GQ_XS; ++i) {
        const unsigned pv = perm[first[b] + i];
        const int R = (int)(pv >> GQ_PXB), kx = (int)(pv & ((1u << GQ_PXB) - 1));
        const double d = T.r * (rowmu[R] + T.mx[kx]);
        const double lam = T.reps + d;
        bool seen = false;
        for (int j = 0; j < n; ++j)
            if (fabs(lam - v[j]) <= 8.9e-16 * fmax(fabs(lam), fabs(v[j]))) seen = true;
        if (!seen) {
            vs[n] = gq_s(d, ic1);
            v[n++] = lam;
        }
    }
    if (n > xmax) n = GQ_XS + 1;   // (xmax < GQ_XS: fewer exact bins, A/B runs)
    X->n[b] = n;
    if (n > GQ_XS) return;
    for (int i = 1; i < n; ++i)   // insertion sort
        for (int j = i; j > 0 && v[j - 1] > v[j]; --j) {
            const double t = v[j], ts = vs[j];
            v[j] = v[j - 1];
            v[j - 1] = t;
            vs[j] = vs[j - 1];
            vs[j - 1] = ts;
        }
    for (int j = 0; j < GQ_XS; ++j) {
        X->lam[b][j] = (j < n) ? v[j] : 0.0;
        X->sv[b][j] = (j < n) ? vs[j] : 0.0;
        X->cut[b][j] = (j + 1 < n) ? 0.5 * (v[j] + v[j + 1]) : 1e300;
    }
}

// one wave per chunk (grid-stride): the chunk's 16 moment sums -> part[chunk][m]
__global__ __launch_bounds__(256) void k_gq_hist_perm(SpecTab T, const double* __restrict__ bh, const unsigned* __restrict__ perm,
                                                      const GqChunk* __restrict__ chunks, int nchunks,
                                                      const GqBins* __restrict__ B, const GqExact* __restrict__ X,
                                                      const double* __restrict__ rowmu, double ic1,
                                                      double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int nw = gridDim.x * 4;
    for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < nchunks; c += nw) {
        const GqChunk ch = chunks[c];
        if (ch.id < 0) continue;
        const int bin = __builtin_amdgcn_readfirstlane(ch.bin);
        const int start = __builtin_amdgcn_readfirstlane(ch.start), len = __builtin_amdgcn_readfirstlane(ch.len);
        const double mid = B->mid[bin], ihw = B->ihw[bin];
        const int xn = __builtin_amdgcn_readfirstlane(X->n[bin]);
        double cut[GQ_XS];
#pragma unroll
        for (int j = 0; j < GQ_XS; ++j) cut[j] = X->cut[bin][j];   // (exact bins only; uniform)
        double acc[GQ_NM];
#pragma unroll
        for (int m = 0; m < GQ_NM; ++m) acc[m] = 0.0;
        for (int bt = 0; bt < GQ_PB; ++bt) {
            unsigned pv[GQ_PE];
#pragma unroll
            for (int e = 0; e < GQ_PE; ++e) {
                const int i = (bt * GQ_PE + e) * 64 + lane;
                pv[e] = (i < len) ? perm[start + i] : 0xffffffffu;
            }
            double x[GQ_PE], rm[GQ_PE], mxv[GQ_PE];
#pragma unroll
            for (int e = 0; e < GQ_PE; ++e) {
                const bool ok = pv[e] != 0xffffffffu;
                const int R = ok ? (int)(pv[e] >> GQ_PXB) : 0;
                const int kx = ok ? (int)(pv[e] & ((1u << GQ_PXB) - 1)) : 0;
                x[e] = ok ? bh[(int64_t)R * T.Nx + kx] : 0.0;
                rm[e] = rowmu[R];
                mxv[e] = T.mx[kx];
            }
            if (xn <= GQ_XS) {   // exact bin (wave-uniform): weight sums per distinct eigenvalue
#pragma unroll
                for (int e = 0; e < GQ_PE; ++e) {
                    const double lam = T.reps + T.r * (rm[e] + mxv[e]);
                    const double w = x[e] * x[e];
                    int sl = 0;
#pragma unroll
                    for (int j = 0; j + 1 < GQ_XS; ++j) sl += (lam > cut[j]) ? 1 : 0;
#pragma unroll
                    for (int m = 0; m < GQ_XS; ++m) acc[m] += (sl == m) ? w : 0.0;
                }
                continue;
            }
#pragma unroll
            for (int e = 0; e < GQ_PE; ++e) {
                // spec_lam's operations without r eps: r (rowmu + mu_x)
                const double lt = gq_s(T.r * (rm[e] + mxv[e]), ic1);
                const double u = (lt - mid) * ihw;
                const double w = x[e] * x[e];   // 0 for the padding lanes
                acc[0] += w;
                acc[1] = fma(w, u, acc[1]);
                const double u2 = u + u;
                double tm2 = 1.0, tm1 = u;
#pragma unroll
                for (int m = 2; m < GQ_NM; ++m) {
                    const double tt = fma(u2, tm1, -tm2);
                    acc[m] = fma(w, tt, acc[m]);
                    tm2 = tm1;
                    tm1 = tt;
                }
            }
        }
        // wave totals in lane 63: the row tree (lane 15 of each row holds its row), then
        // row_bcast:15 into rows 1, 3 and row_bcast:31 into rows 2, 3: (R3 + R2) + (R1 + R0)
#pragma unroll
        for (int m = 0; m < GQ_NM; ++m) {
            double v = acc[m];
            dpp_row_sums(v);
            v += dbl_dpp<0x142, 0xa>(v);
            v += dbl_dpp<0x143, 0xc>(v);
            acc[m] = v;
        }
        if (lane == 63) {
            double* dst = part + (int64_t)ch.id * GQ_NM;
#pragma unroll
            for (int m = 0; m < GQ_NM; m += 2) *reinterpret_cast<dbl2*>(dst + m) = dbl2{acc[m], acc[m + 1]};
        }
    }
}

// the first row of each chunk (plan time: the XCD grouping of the chunk list)
__global__ __launch_bounds__(256) void k_gq_chunk_rows(const GqChunk* __restrict__ chunks, int n,
                                                       const unsigned* __restrict__ perm, int* __restrict__ row) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < n) row[c] = (int)(perm[chunks[c].start] >> GQ_PXB);
}

// hist[m][b] = the sum of bin b's chunk sums (chunks cfirst[b] .. cfirst[b + 1]): one wave per
// (m, b), lane l adding chunks l, l + 64, ... in order, then the fixed wave tree (row_shr, the
// four row totals in order) -- deterministic, and one load latency per 64 chunks (a thread per
// (m, b) looping over a C4-size bin's 128 chunks took 56 us)
__global__ __launch_bounds__(256) void k_gq_perm_reduce(const double* __restrict__ part, const int* __restrict__ cfirst,
                                                        double* __restrict__ hist) {
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);   // (m, b) = e / GQ_NB, e % GQ_NB
    const int lane = threadIdx.x & 63;
    if (e >= GQ_HIST) return;
    const int m = e / GQ_NB, b = e - m * GQ_NB;
    double t = 0.0;
    for (int c = cfirst[b] + lane; c < cfirst[b + 1]; c += 64) t += part[(int64_t)c * GQ_NM + m];
    t = gq_uniform_sum(t);
    if (lane == 0) hist[e] = t;
}

// ---------------------------------------------------------------------------- 2. Gauss rules
// Modified Chebyshev algorithm (Gautschi) for one bin: recurrence coefficients al[k], be[k]
// (k < GQ_M) of the bin's measure in u from its Chebyshev moments mu[j] (monic Chebyshev
// auxiliaries: a_k = 0, b_1 = 1/2, b_k = 1/4).  Returns n: the leading steps with be[k] > 0
// (a bin with fewer support points than GQ_M, or an empty one, gets a shorter rule).
__device__ int gq_mcheb(const double (&mu)[GQ_NM], double (&al)[GQ_M], double (&be)[GQ_M]) {
    double sig[GQ_NM], sigm[GQ_NM], nw[GQ_NM];
#pragma unroll
    for (int j = 0; j < GQ_NM; ++j) {
        sig[j] = (j == 0) ? mu[0] : ldexp(mu[j], 1 - j);   // monic: p_j = T_j / 2^(j-1)
        sigm[j] = 0.0;
        nw[j] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < GQ_M; ++k) { al[k] = 0.0; be[k] = 0.0; }
    if (!(sig[0] > 0.0)) return 0;
    al[0] = sig[1] / sig[0];
    be[0] = sig[0];
    int n = GQ_M;
#pragma unroll
    for (int k = 1; k < GQ_M; ++k) {
#pragma unroll
        for (int l = k; l < GQ_NM - k; ++l) {
            const double bl = (l == 1) ? 0.5 : 0.25;
            nw[l] = sig[l + 1] - al[k - 1] * sig[l] - be[k - 1] * sigm[l] + bl * sig[l - 1];
        }
        const double a = nw[k + 1] / nw[k] - sig[k] / sig[k - 1];
        const double b = nw[k] / sig[k - 1];
        if (n == GQ_M && !(b > 1e-13 && isfinite(a) && isfinite(b))) n = k;
        al[k] = a;
        be[k] = b;
#pragma unroll
        for (int l = 0; l < GQ_NM; ++l) {
            sigm[l] = sig[l];
            sig[l] = nw[l];
        }
    }
    return n;
}

// eigenvalues of the leading n x n Jacobi matrix below x: sign changes of the Sturm sequence of
// characteristic polynomials p_i(x) = (al_i - x) p_{i-1} - be_i p_{i-2} (no divisions; |u| <= 1
// and be <= 1 keep p_i within 3^8).  A zero takes the sign opposite to its predecessor (the
// standard convention).  The signs are taken from the bit patterns with 32-bit integer logic:
// the same tests as fp64 compares (v < 0: sign bit set and not +-0), but no VALU -> SGPR mask
// -> SALU -> VALU round trips -- those made a Sturm evaluation ~1400 cycles (the node lab at cb85e44:
// 24 bisections = 33.5 k of a node thread's 46 k cycles).  Equal to the compare form on 3 M random
// and quantised (exact-zero) cases.
__device__ __forceinline__ void gq_sign(double v, unsigned& neg, unsigned& nz) {
    const long long b = __double_as_longlong(v);
    const unsigned hi = (unsigned)(b >> 32), lo = (unsigned)b;
    const unsigned m = (hi & 0x7fffffffu) | lo;
    nz = (m | (0u - m)) >> 31;   // v != +-0
    neg = (hi >> 31) & nz;       // v < 0
}

__device__ __forceinline__ int gq_sturm(const double (&al)[GQ_M], const double (&be)[GQ_M], int n, double x) {
    double pm = 1.0, p = al[0] - x;
    unsigned negp, nzp, negpm = 0u, nzpm = 1u;
    gq_sign(p, negp, nzp);
    unsigned cnt = negp;   // sign change between p_0 = 1 and p_1
#pragma unroll
    for (int i = 1; i < GQ_M; ++i) {
        if (i < n) {
            const double pn = (al[i] - x) * p - be[i] * pm;
            unsigned negn, nzn;
            gq_sign(pn, negn, nzn);
            // pn == 0 counts; otherwise a change unless pn has p's sign (a zero p: negative
            // exactly when pm > 0)
            const unsigned pmpos = nzpm & (negpm ^ 1u);
            const unsigned pneg = negp | ((nzp ^ 1u) & pmpos);
            cnt += (nzn ^ 1u) | (negn ^ pneg);
            negpm = negp;
            nzpm = nzp;
            negp = negn;
            nzp = nzn;
            pm = p;
            p = pn;
        }
    }
    return (int)cnt;
}

// Stieltjes procedure for an exact bin's discrete measure (points u[j], weights w[j], j < np):
// the same monic recurrence coefficients as gq_mcheb (be[0] = the mass) and the same cut-off,
// here on the points themselves -- no moment cancellation
__device__ int gq_stieltjes(const double (&u)[GQ_XS], const double (&w)[GQ_XS], int np, double (&al)[GQ_M],
                            double (&be)[GQ_M]) {
    double pm[GQ_XS], pc[GQ_XS];
    double ncur = 0.0;
#pragma unroll
    for (int j = 0; j < GQ_XS; ++j) {
        pm[j] = 0.0;
        pc[j] = (j < np) ? 1.0 : 0.0;
        ncur += (j < np) ? w[j] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < GQ_M; ++k) { al[k] = 0.0; be[k] = 0.0; }
    if (!(ncur > 0.0)) return 0;
    be[0] = ncur;
#pragma unroll
    for (int k = 0; k < GQ_M; ++k) {
        double sa = 0.0;
#pragma unroll
        for (int j = 0; j < GQ_XS; ++j) sa += w[j] * u[j] * pc[j] * pc[j];
        al[k] = sa / ncur;
        if (k + 1 == GQ_M) break;
        const double bk = (k == 0) ? 0.0 : be[k];
        double nn = 0.0;
#pragma unroll
        for (int j = 0; j < GQ_XS; ++j) {
            const double pn = (u[j] - al[k]) * pc[j] - bk * pm[j];
            pm[j] = pc[j];
            pc[j] = pn;
            nn += w[j] * pn * pn;
        }
        const double b = nn / ncur;
        if (!(b > 1e-13 && isfinite(b))) return k + 1;
        be[k + 1] = b;
        ncur = nn;
    }
    return GQ_M;
}

// One wave per bin (round 5).  The round-4 form ran a thread per node (k_gq_nodes, and its lab
// tools/gqnodes_lab.hip, in the history at cb85e44): a node thread spent 28 k of its 38 k cycles
// in 24 serial Sturm bisections, and only 32 waves ran on a 256-CU chip.  Here lanes 8k .. 8k+7 find
// node k together by 9-section -- each lane evaluates the Sturm count at one of the 8 interior
// points of the bracket, a ballot picks the sub-interval -- 3.17 bits per round, so 8 rounds
// replace the 24 bisections, and 256 waves fill the chip.  n, the bracket and the counts are the
// same in the 8 lanes of a node (the same arithmetic on the same values), so the Newton polish
// and the Christoffel weight run redundantly and lane 8k stores.
// part != null (single shard): the bin's 16 moments are summed here from the chunk sums, in
// k_gq_perm_reduce's order (lane l: chunks l, l + 64, ..., then gq_uniform_sum) -- the same bits,
// one launch less; otherwise hist holds the world's histograms, summed in rank order.
__global__ __launch_bounds__(256) void k_gq_nodes_w(const double* __restrict__ hist, const double* __restrict__ part,
                                                    const int* __restrict__ cfirst, const GqBins* __restrict__ B,
                                                    const GqExact* __restrict__ X, int world, double lmin, double c1,
                                                    GqNodes* __restrict__ nd) {
    const int bin = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, k = lane >> 3, sub = lane & 7;
    const int id = bin * GQ_M + k;
    double mu[GQ_NM];
    if (part) {
        double t[GQ_NM];
#pragma unroll
        for (int m = 0; m < GQ_NM; ++m) t[m] = 0.0;
        const int ce = cfirst[bin + 1];
        for (int c = cfirst[bin] + lane; c < ce; c += 64) {
            const dbl2* src = reinterpret_cast<const dbl2*>(part + (int64_t)c * GQ_NM);
#pragma unroll
            for (int m = 0; m < GQ_NM; m += 2) {
                const dbl2 v = src[m >> 1];
                t[m] += v.x;
                t[m + 1] += v.y;
            }
        }
#pragma unroll
        for (int m = 0; m < GQ_NM; ++m) mu[m] = 0.0 + gq_uniform_sum(t[m]);   // (0 + sum: the bits of the hist path below)
    } else {
#pragma unroll
        for (int j = 0; j < GQ_NM; ++j) {
            double v = 0.0;
            for (int g = 0; g < world; ++g) v += hist[(int64_t)g * GQ_HIST + j * GQ_NB + bin];   // rank order
            mu[j] = v;
        }
    }
    const int xn = X->n[bin];
    if (xn <= GQ_M) {   // exact bin with at most GQ_M points: they are the rule (zero weights allowed)
        if (sub == 0) {
            nd->lam[id] = (k < xn) ? X->lam[bin][k] : lmin;
            nd->w[id] = (k < xn) ? mu[k] : 0.0;
        }
        return;
    }
    double al[GQ_M], be[GQ_M];
    int n;
    if (xn <= GQ_XS) {   // exact bin: the Gauss rule of its points
        // points closer than 1e-8 in u (eigenvalues a few ulp apart that the 4-ulp merge kept
        // apart) go into their weighted mean first: a rule's moments of degree < 16 move by
        // ~(16 d)^2, while a cluster of nodes makes the Christoffel weights lose digits
        // (a 1e-13-wide pair cost 7e-9 of a weight in the numpy restatement)
        double u[GQ_XS], w[GQ_XS];
        int m = 0;
        double ustart = 0.0;
        for (int j = 0; j < xn; ++j) {
            const double uj = (X->sv[bin][j] - B->mid[bin]) * B->ihw[bin], wj = mu[j];
            if (m > 0 && uj - ustart < 1e-8) {
                const double W = w[m - 1] + wj;
                if (W > 0.0) u[m - 1] = (u[m - 1] * w[m - 1] + uj * wj) / W;
                w[m - 1] = W;
            } else {
                u[m] = uj;
                w[m] = wj;
                ustart = uj;
                ++m;
            }
        }
        for (int j = m; j < GQ_XS; ++j) { u[j] = 0.0; w[j] = 0.0; }
        if (m <= GQ_M) {
            if (sub == 0) {
                nd->lam[id] = (k < m) ? lmin + c1 * fma(B->hw[bin], u[k], B->mid[bin]) : lmin;
                nd->w[id] = (k < m) ? w[k] : 0.0;
            }
            return;
        }
        n = gq_stieltjes(u, w, m, al, be);
    } else {
        n = gq_mcheb(mu, al, be);
    }
    n = __builtin_amdgcn_readfirstlane(n);   // the same in every lane: the Sturm loop's i < n is scalar
    double lamk = lmin, wk = 0.0;
    if (k < n) {
        double sb[GQ_M], isb[GQ_M];
#pragma unroll
        for (int i = 0; i < GQ_M; ++i) {
            sb[i] = (i < n) ? sqrt(be[i]) : 0.0;
            isb[i] = (i < n) ? 1.0 / sb[i] : 0.0;
        }
        double lo = 1e300, hi = -1e300;
#pragma unroll
        for (int i = 0; i < GQ_M; ++i) {
            if (i < n) {
                const double r = ((i > 0) ? sb[i] : 0.0) + ((i + 1 < n) ? sb[i + 1] : 0.0);
                lo = fmin(lo, al[i] - r);
                hi = fmax(hi, al[i] + r);
            }
        }
        // 9-section until the bracket holds this eigenvalue alone and has shrunk 9^8 > 2^24 (the
        // bisection's bar); counts c(x) = eigenvalues below x rise with x, so the first of the 8
        // points whose count exceeds k is the new upper end and the point before it the lower
        int clo = 0, chi = n;
        const double frac = (double)(sub + 1) * (1.0 / 9.0);
        const int gbase = lane & ~7;
        auto msect = [&](int itmin, int itmax) {
            for (int it = 0; it < itmax; ++it) {
                if (it >= itmin && chi - clo == 1) break;
                const double h = hi - lo;
                const double x = fma(h, frac, lo);
                // a bracket at rounding: the end points no longer move
                const unsigned long long stuck = __ballot(x <= lo || x >= hi);
                if ((stuck >> gbase) & 0xffull) break;
                const int c = gq_sturm(al, be, n, x);
                const unsigned g = (unsigned)(__ballot(c > k) >> gbase) & 0xffu;
                const int j = g ? __builtin_ctz(g) : 8;   // first point above node k
                const int cj = __shfl(c, gbase + min(j, 7));
                const int cjm = __shfl(c, gbase + max(j - 1, 0));
                if (j < 8) {
                    hi = fma(h, (double)(j + 1) * (1.0 / 9.0), lo);
                    chi = cj;
                }
                if (j > 0) {
                    lo = fma(h, (double)j * (1.0 / 9.0), lo);
                    clo = cjm;
                }
            }
        };
        auto bisect = [&](int itmax) {   // (rounding: the last bits)
            for (int it = 0; it < itmax; ++it) {
                const double mid = 0.5 * (lo + hi);
                if (mid <= lo || mid >= hi) break;
                const int c = gq_sturm(al, be, n, mid);
                if (c > k) { hi = mid; chi = c; }
                else { lo = mid; clo = c; }
            }
        };
        msect(8, 32);
        double u = 0.5 * (lo + hi);
        bool newton_ok = true;
        for (int it = 0; it < 6; ++it) {
            double pm = 1.0, p = al[0] - u, dm = 0.0, d = -1.0;
#pragma unroll
            for (int i = 1; i < GQ_M; ++i) {
                if (i < n) {
                    const double pn = (al[i] - u) * p - be[i] * pm;
                    const double dn = (al[i] - u) * d - p - be[i] * dm;
                    pm = p;
                    p = pn;
                    dm = d;
                    d = dn;
                }
            }
            if (d == 0.0 || p == 0.0) break;
            const double un = u - p / d;
            if (!(un > lo && un < hi)) { newton_ok = false; break; }
            if (un == u) break;
            u = un;
        }
        if (!newton_ok) {
            msect(64, 64);
            bisect(8);
            u = 0.5 * (lo + hi);
        }
        double pm = 0.0, p = isb[0], ssum = p * p;
#pragma unroll
        for (int j = 0; j + 1 < GQ_M; ++j) {
            if (j + 1 < n) {
                const double pn = ((u - al[j]) * p - ((j > 0) ? sb[j] : 0.0) * pm) * isb[j + 1];
                pm = p;
                p = pn;
                ssum += p * p;
            }
        }
        wk = 1.0 / ssum;
        lamk = lmin + c1 * fma(B->hw[bin], u, B->mid[bin]);
    }
    if (sub == 0) {
        nd->lam[id] = lamk;
        nd->w[id] = wk;
    }
}

// ---------------------------------------------------------------------------- 3. CG on the nodes
// scipy's cg (x0 = 0, M = I) on the compressed measure: rho_k = r.r, stop if norm(r) < rtol norm(b),
// beta = rho_k / rho_{k-1}, p = r + beta p, alpha = rho_k / p.Ap, r -= alpha A p.  p.Ap comes from
// the same reduction as rho (Chronopoulos-Gear: p_k.Ap_k = r_k.Ar_k - beta_k rho_k / alpha_{k-1},
// exact in exact arithmetic), so a step is one block reduction of two sums and one barrier
// (the LDS slots alternate between steps).  The node vectors are carried scaled by sqrt(w)
// (r~ = sqrt(w) r: the same recurrence, rho = sum r~^2), and only A p is kept, not p: with
// lr = lam r, a step is ap = beta ap + lr, r -= alpha ap, lr = lam r, then the two sums r r and
// lr r -- five VALU operations per node (seven with p).
// A step's serial chain is the reduction: each wave sums its lanes (DPP rows, then the row
// totals by row_bcast), lane 63 stores the wave's pair, and after the barrier every lane reads
// the GQ_CGNW pairs (same-address LDS reads broadcast) and adds them in wave order.
// (tools/gqcg_lab.hip, 180 steps on 2048 nodes: 103.8 us for the first version -- p kept, lane
// 0 reading the pairs and readlane-broadcasting them -- against 85.9 here; one wave of 32 nodes
// per lane 193, 128 or 512 threads 103 / 111, the row totals through LDS 113.)
constexpr int GQ_CGNW = GQ_CGNTH / 64;
constexpr int GQ_CGN = GQ_NODES / GQ_CGNTH;   // nodes per thread
constexpr int GQ_CGACC = GQ_CGN >= 2 ? 2 : 1; // partial sums per thread (two chains)
static_assert(GQ_NODES % GQ_CGNTH == 0 && GQ_CGNTH % 64 == 0 && GQ_CGNTH <= 1024, "whole waves, whole nodes");

// klim: the step beyond which the solve reports status 2 (GQ_KMAX; FOTO_GQ_KLIM lowers it in tests
// to force the s-step redo path).  H (may be null): a pinned, coherent host copy of the header --
// the host reads the result there after its sync, with no copy launch on the stream.
// (alpha_k, beta_k) published step by step for the table blocks of k_gq_cgtab (round 6): NaN
// until the CG stores them (write-through, agent scope), kdone = K once the CG has ended
// (release), the last table block resets the slots it saw used for the next solve.
struct GqPub {
    double ab[GQ_KMAX][2];   // [k] = (alpha_k, beta_k)
    int kdone;           // -1 while the CG runs
    unsigned ticket;     // table blocks done
};

// pub (may be null): k_gq_cgtab's publication slots
__device__ __forceinline__ void gq_cg_body(const GqNodes* __restrict__ nd, double rtol, int maxiter, int klim,
                                           GqState* __restrict__ S, GqState* H, GqPub* pub, dbl2 (*red)[GQ_CGNW],
                                           double (*abL)[GQ_KMAX]) {
    // alpha_k, beta_k go to LDS during the loop and to S after it
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double lam[GQ_CGN], r[GQ_CGN], ap[GQ_CGN], lr[GQ_CGN];
    double mass = 0.0;
#pragma unroll
    for (int j = 0; j < GQ_CGN; ++j) {
        const int id = threadIdx.x * GQ_CGN + j;
        lam[j] = nd->lam[id];
        const double w = nd->w[id];
        r[j] = sqrt(w);
        ap[j] = 0.0;
        lr[j] = lam[j] * r[j];
        mass += w;
    }
    // block sums of (a, b), the same in every lane
    auto reduce2 = [&](double a, double b, int slot, double* ra, double* rb) {
        // the two wave sums side by side (two independent DPP chains), totals in lane 63:
        // row_shr tree, then row_bcast 15 / 31 -- (R3 + R2) + (R1 + R0).  The tree is
        // dpp_row_sums' (foto_reduce.h), written out for the pair: through a two-value form of
        // that function the pair's last adds land in other VGPRs, and the interleaved A/B
        // (profiles/reduce_refactor_ab.txt) did not keep every repetition inside the old code's spread
        a += dbl_dpp<0x111>(a);
        b += dbl_dpp<0x111>(b);
        a += dbl_dpp<0x112>(a);
        b += dbl_dpp<0x112>(b);
        a += dbl_dpp<0x114>(a);
        b += dbl_dpp<0x114>(b);
        a += dbl_dpp<0x118>(a);
        b += dbl_dpp<0x118>(b);
        a += dbl_dpp<0x142, 0xa>(a);
        b += dbl_dpp<0x142, 0xa>(b);
        a += dbl_dpp<0x143, 0xc>(a);
        b += dbl_dpp<0x143, 0xc>(b);
        if (lane == 63) red[slot][wv] = dbl2{a, b};
        __syncthreads();
        dbl2 t = red[slot][0];
#pragma unroll
        for (int q = 1; q < GQ_CGNW; ++q) t += red[slot][q];
        *ra = t[0];
        *rb = t[1];
    };
    double bn2, unused;
    reduce2(mass, 0.0, 1, &bn2, &unused);
    const double atol = rtol * sqrt(bn2);
    const double atol2 = atol * atol;
    int status = 0, conv = 0, K = maxiter;
    double rho = bn2, irho_prev = 1.0, sigma_prev = 1.0;
    if (!(bn2 > 0.0)) {   // scipy: b = 0 returns x = 0 after 0 iterations
        K = 0;
        conv = 1;
        maxiter = 0;
    }
    // the first step's sums (r0 = sqrt(w))
    double sa[GQ_CGACC], sd[GQ_CGACC];
#pragma unroll
    for (int q = 0; q < GQ_CGACC; ++q) { sa[q] = 0.0; sd[q] = 0.0; }
#pragma unroll
    for (int j = 0; j < GQ_CGN; ++j) {
        sa[j % GQ_CGACC] = fma(r[j], r[j], sa[j % GQ_CGACC]);
        sd[j % GQ_CGACC] = fma(lr[j], r[j], sd[j % GQ_CGACC]);
    }
    for (int k = 0; k < maxiter; ++k) {
#pragma unroll
        for (int h = GQ_CGACC / 2; h >= 1; h >>= 1)
#pragma unroll
            for (int q = 0; q < h; ++q) { sa[q] += sa[q + h]; sd[q] += sd[q + h]; }
        double delta;
        reduce2(sa[0], sd[0], k & 1, &rho, &delta);
        // norm(r) < atol, squared: the compressed measure carries rho to ~1e-13 anyway
        if (rho < atol2) { K = k; conv = 1; break; }
        if (k >= klim) { K = k; status = 2; break; }
        const double beta = (k == 0) ? 0.0 : rho * irho_prev;
        const double sigma = (k == 0) ? delta : fma(-beta * beta, sigma_prev, delta);
        if (!(sigma > 0.0) || !isfinite(sigma)) { K = k; status = 1; break; }
        // alpha = rho / sigma by a reciprocal and two Newton steps plus one residual
        // correction (a shorter dependent chain than the IEEE division sequence; within an ulp)
        double y = __builtin_amdgcn_rcp(sigma);
        y = fma(y, fma(-sigma, y, 1.0), y);
        y = fma(y, fma(-sigma, y, 1.0), y);
        double alpha = rho * y;
        alpha = fma(fma(-sigma, alpha, rho), y, alpha);
        irho_prev = 1.0 / rho;   // off the critical path (independent of alpha)
#pragma unroll
        for (int q = 0; q < GQ_CGACC; ++q) { sa[q] = 0.0; sd[q] = 0.0; }
#pragma unroll
        for (int j = 0; j < GQ_CGN; ++j) {
            ap[j] = fma(beta, ap[j], lr[j]);
            r[j] = fma(-alpha, ap[j], r[j]);
            lr[j] = lam[j] * r[j];
            sa[j % GQ_CGACC] = fma(r[j], r[j], sa[j % GQ_CGACC]);
            sd[j % GQ_CGACC] = fma(lr[j], r[j], sd[j % GQ_CGACC]);
        }
        if (threadIdx.x == 0) {
            abL[0][k] = alpha;
            abL[1][k] = beta;
            if (pub) {   // (no wait: the barrier of the next step does not wait for global stores)
                __hip_atomic_store(&pub->ab[k][1], beta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&pub->ab[k][0], alpha, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        sigma_prev = sigma;
    }
    if (pub && threadIdx.x == 0) __hip_atomic_store(&pub->kdone, K, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const int kst = (K < GQ_KMAX) ? K : GQ_KMAX;
    for (int e = threadIdx.x; e < kst; e += GQ_CGNTH) {
        S->alpha[e] = abL[0][e];
        S->beta[e] = abL[1][e];
    }
    if (threadIdx.x == 0) {
        const int ok = (status == 0 && S->broken == 0) ? 1 : 0;
        S->K = K;
        S->status = status;
        S->conv = conv;
        S->done = ok;
        S->broken = ok ? 0 : 1;
        S->bn2 = bn2;
        S->rn2 = rho;
        // solution-table terms: the Chebyshev coefficients of Q on a half-bin of half-width
        // h = pi / (2 GQ_QB) in theta decay like (K h)^n / n!; keep those above 1e-18 of the
        // leading one (K = 180: 16 terms; 20 with the whole bins of the first version)
        const double kh = (double)(K > 0 ? K : 1) * (M_PI / (2.0 * GQ_QB));
        double term = 1.0;
        int qn = 1;
        while (qn < GQ_QN && term > 1e-18) {
            term *= kh / (double)qn;
            ++qn;
        }
        S->qn = qn;
        if (H) {
            H->K = K;
            H->status = status;
            H->conv = conv;
            H->done = ok;
            H->qn = qn;
            H->broken = ok ? 0 : 1;
            H->bn2 = bn2;
            H->rn2 = rho;
            __threadfence_system();
        }
    }
}

__global__ __launch_bounds__(GQ_CGNTH) void k_gq_cg(const GqNodes* __restrict__ nd, double rtol, int maxiter,
                                                    int klim, GqState* __restrict__ S, GqState* H) {
    __shared__ __attribute__((aligned(16))) dbl2 red[2][GQ_CGNW];
    __shared__ double abL[2][GQ_KMAX];
    gq_cg_body(nd, rtol, maxiter, klim, S, H, nullptr, red, abL);
}

// ---------------------------------------------------------------------------- 4. solution table
// The constants of the table transform, once per plan (k_gq_qtab took 1024 + 256 fp64 cosines
// per block on every solve): cs[k][j] = cos(pi k (j + 1/2) / QN), v[j] = cos(pi (j + 1/2) / QN).
struct GqQCos {
    double cs[GQ_QN][GQ_QN];
    double v[GQ_QN];
};
__global__ __launch_bounds__(256) void k_gq_qcos(GqQCos* __restrict__ Q) {
    for (int e = threadIdx.x; e < GQ_QN * GQ_QN; e += 256) {
        const int kk = e / GQ_QN, jj = e - kk * GQ_QN;
        Q->cs[kk][jj] = cos(M_PI * (double)kk * ((double)jj + 0.5) / GQ_QN);
    }
    if (threadIdx.x < GQ_QN) Q->v[threadIdx.x] = cos(M_PI * ((double)threadIdx.x + 0.5) / GQ_QN);
}

// thread = (bin, point j): Q at the j-th Chebyshev point of the bin (the scalar recurrence from
// r = 1, K steps), then the bin's GQ_QN Chebyshev coefficients (thread j computes coefficient j).
// The recurrence's dependent chain is p -> r -> p (alpha lam is formed off the chain), alpha and
// beta are read from LDS as one 16-byte pair per step.
__global__ __launch_bounds__(256) void k_gq_qtab(const GqState* __restrict__ S, const GqBins* __restrict__ B,
                                                 const GqQCos* __restrict__ Q, double lmin, double c1,
                                                 double* __restrict__ tab) {
    static_assert(256 % GQ_QN == 0, "whole bins per block");
    __shared__ double v[256];
    __shared__ double cs[GQ_QN][GQ_QN];
    __shared__ __attribute__((aligned(16))) dbl2 ab[GQ_KMAX];   // (alpha, beta) of step k
    for (int e = threadIdx.x; e < GQ_QN * GQ_QN; e += 256) (&cs[0][0])[e] = (&Q->cs[0][0])[e];
    const int K = (S->status == 0) ? S->K : 0;
    for (int e = threadIdx.x; e < K; e += 256) ab[e] = dbl2{S->alpha[e], S->beta[e]};
    __syncthreads();
    const int id = blockIdx.x * 256 + threadIdx.x;
    const int hb = id / GQ_QN, j = id - hb * GQ_QN;   // half-bin hb = 2 bin + (u > 0)
    const int bin = hb >> 1;
    const double uj = 0.5 * (Q->v[j] + ((hb & 1) ? 1.0 : -1.0));   // Chebyshev point of the half-bin
    const double lam = lmin + c1 * fma(B->hw[bin], uj, B->mid[bin]);
    double x = 0.0, r = 1.0, p = 0.0;
    for (int k = 0; k < K; ++k) {
        const dbl2 q = ab[k];
        const double al = q.x * lam;
        p = fma(q.y, p, r);
        x = fma(q.x, p, x);
        r = fma(-al, p, r);
    }
    v[threadIdx.x] = x;
    __syncthreads();
    const int base = threadIdx.x - j;
    double c = 0.0;
#pragma unroll 8
    for (int jj = 0; jj < GQ_QN; ++jj) c = fma(v[base + jj], cs[j][jj], c);
    c *= (j == 0 ? 1.0 : 2.0) / GQ_QN;
    tab[j * GQ_QB + hb] = c;
}

// k_gq_cg and k_gq_qtab in one launch (round 6, FOTO_GQ_CGTAB=1): block 0 runs the node CG and
// publishes each step's (alpha, beta) as it goes (GqPub); blocks 1 .. GQ_TAB / 256 are
// k_gq_qtab's blocks, running the scalar recurrence of their Chebyshev points on the steps
// published so far, so the table is finished a few microseconds after the CG instead of one
// 8.8 us kernel later.  A wave polls 64 slots at once (agent-scope loads) and runs the ready
// prefix; the same alpha, beta, the same operations in the same order as k_gq_qtab: the same
// table.  Every wave leaves: after K steps once kdone = K is seen, or after GQ_SPIN_MAX empty
// polls (a NaN table then -- the solve fails loudly, never silently).  The grid (65 blocks) is
// resident at once on the otherwise idle device (the previous kernel of the stream has ended).
constexpr unsigned GQ_SPIN_MAX = 1u << 22;
__global__ __launch_bounds__(256) void k_gq_cgtab(const GqNodes* __restrict__ nd, double rtol, int maxiter, int klim,
                                                  GqState* __restrict__ S, GqState* H, GqPub* pub,
                                                  const GqBins* __restrict__ B, const GqQCos* __restrict__ Q,
                                                  double lmin, double c1, double* __restrict__ tab) {
    static_assert(GQ_CGNTH == 256 && 256 % GQ_QN == 0, "one block size for the CG and the table blocks");
    __shared__ __attribute__((aligned(16))) dbl2 red[2][GQ_CGNW];
    __shared__ double abL[2][GQ_KMAX];
    __shared__ double v[256];
    __shared__ double cs[GQ_QN][GQ_QN];
    __shared__ int last;
    if (blockIdx.x == 0) {
        gq_cg_body(nd, rtol, maxiter, klim, S, H, pub, red, abL);
        return;
    }
    for (int e = threadIdx.x; e < GQ_QN * GQ_QN; e += 256) (&cs[0][0])[e] = (&Q->cs[0][0])[e];
    const int id = (blockIdx.x - 1) * 256 + threadIdx.x;
    const int hb = id / GQ_QN, j = id - hb * GQ_QN;   // half-bin hb = 2 bin + (u > 0)
    const int bin = hb >> 1;
    const double uj = 0.5 * (Q->v[j] + ((hb & 1) ? 1.0 : -1.0));
    const double lam = lmin + c1 * fma(B->hw[bin], uj, B->mid[bin]);
    const int lane = threadIdx.x & 63;
    double x = 0.0, r = 1.0, p = 0.0;
    int k = 0;
    unsigned spins = 0;
    for (;;) {
        double qa = __builtin_nan(""), qb = __builtin_nan("");
        if (k + lane < GQ_KMAX) {
            qa = __hip_atomic_load(&pub->ab[k + lane][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            qb = __hip_atomic_load(&pub->ab[k + lane][1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const unsigned long long ready = __ballot(!(qa != qa) && !(qb != qb));
        const int n = (~ready == 0ull) ? 64 : __builtin_ctzll(~ready);   // the ready prefix
        if (n == 0) {
            const int kd = __hip_atomic_load(&pub->kdone, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            if (kd >= 0 && k >= kd) break;
            if (++spins > GQ_SPIN_MAX) {
                x = __builtin_nan("");
                break;
            }
            if (kd < 0) __builtin_amdgcn_s_sleep(2);
            continue;
        }
        for (int i = 0; i < n; ++i) {
            const double qx = dbl_readlane(qa, i), qy = dbl_readlane(qb, i);
            const double al = qx * lam;
            p = fma(qy, p, r);
            x = fma(qx, p, x);
            r = fma(-al, p, r);
        }
        k += n;
    }
    v[threadIdx.x] = x;
    __syncthreads();
    const int base = threadIdx.x - j;
    double c = 0.0;
#pragma unroll 8
    for (int jj = 0; jj < GQ_QN; ++jj) c = fma(v[base + jj], cs[j][jj], c);
    c *= (j == 0 ? 1.0 : 2.0) / GQ_QN;
    tab[j * GQ_QB + hb] = c;
    // the last table block to finish resets the slots for the next solve
    if (threadIdx.x == 0) last = (atomicAdd(&pub->ticket, 1u) == gridDim.x - 2) ? 1 : 0;
    __syncthreads();
    if (last) {
        const int kd = __hip_atomic_load(&pub->kdone, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        const int ku = (kd >= 0 && kd < GQ_KMAX) ? kd : GQ_KMAX;
        for (int e = threadIdx.x; e < ku; e += 256) {
            __hip_atomic_store(&pub->ab[e][0], __builtin_nan(""), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&pub->ab[e][1], __builtin_nan(""), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (threadIdx.x == 0) {
            __hip_atomic_store(&pub->kdone, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&pub->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// Q from the table in LDS ([coefficient][bin]) at local variable u of bin b, Clenshaw over the
// qn leading terms
static_assert(GQ_QB == 2 * GQ_NB, "the solution table halves the measure's bins");
// Rows k >= ql are not in LDS (the launch sized its table for ql rows) and come from tabG (the
// global table, L2-resident) -- the highest-order terms, first in Clenshaw's order; same values,
// same arithmetic.
__device__ __forceinline__ double gq_q(const double* tabL, const double* __restrict__ tabG, int bin, double uu,
                                       int qn, int ql) {
    // half-bin of bin's local variable uu in [-1, 1] and its own local variable u
    const bool up = uu > 0.0;
    const int b = 2 * bin + (up ? 1 : 0);
    const double u = fma(2.0, uu, up ? -1.0 : 1.0);
    const double u2 = u + u;
    double b1 = 0.0, b2 = 0.0;
    int k = qn - 1;
    for (; k >= ql; --k) {
        const double t = fma(u2, b1, tabG[k * GQ_QB + b] - b2);
        b2 = b1;
        b1 = t;
    }
    // blocks of 8 coefficients read together, then their FMA chain (a read per chain step
    // leaves the LDS latency on the critical path)
    for (; k >= 8; k -= 8) {
        double cf[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) cf[i] = tabL[(k - i) * GQ_QB + b];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const double t = fma(u2, b1, cf[i] - b2);
            b2 = b1;
            b1 = t;
        }
    }
    for (; k >= 1; --k) {
        const double t = fma(u2, b1, tabL[k * GQ_QB + b] - b2);
        b2 = b1;
        b1 = t;
    }
    return fma(u, b1, tabL[b] - b2);
}

// the min(qn, ql) leading coefficient rows of the table into LDS; returns qn (block-uniform)
__device__ __forceinline__ int gq_load_tab(double* tabL, const double* __restrict__ tab, const GqState* S, int ql) {
    const int qn = __builtin_amdgcn_readfirstlane(S->qn);
    for (int e = threadIdx.x; e < min(qn, ql) * GQ_QB / 2; e += blockDim.x)
        reinterpret_cast<dbl2*>(tabL)[e] = reinterpret_cast<const dbl2*>(tab)[e];
    __syncthreads();
    return qn;
}

// ---------------------------------------------------------------------------- 5. x^ = Q(lam) b^
// An elementwise kernel (k_gq_xhat) writes x^ into the box, then the plain inverse t-DCT column
// kernels transform it.  Fusing the Q evaluations into the column kernels was measured slower
// (105 us vs ~60 for the pair): a column kernel holds the 64 KB table at 2 waves per SIMD and
// could keep only one or two b^ loads per lane in flight ahead of its long acos + Clenshaw
// chains, while the elementwise kernel runs 1024-thread blocks (16 waves per CU) over
// coalesced pairs of elements.  Round 5 tried again with cheaper elements and 512-thread
// blocks (k_dct_t_inv_gq, bit-identical): 92 us against 74 for the pair; it is in the history
// at cb85e44.

// x^ = Q(lam) b^ over the whole box: persistent 1024-thread blocks (the table loaded once per
// block); a wave takes whole rows (one division per row), two elements per lane when Nx is even.
// (Round 4: a whole 640-wide row's loads issued before any use, 5 or 8 pairs per lane: DCT chain
// 143 vs 139-140 us, not kept.)
constexpr int GQ_XNTH = 1024;
constexpr int GQ_XQL = 17;   // table rows a block holds in LDS (68 KB: two blocks per CU); rows beyond from global
__global__ __launch_bounds__(GQ_XNTH) void k_gq_xhat(SpecTab T, const double* __restrict__ bh,
                                                     const double* __restrict__ tab, const GqState* __restrict__ S,
                                                     const GqBins* __restrict__ Bg, double ic1, double* __restrict__ out,
                                                     int ql) {
    extern __shared__ double tabL[];
    __shared__ __attribute__((aligned(16))) GqBins L;
    gq_load_bins(&L, Bg);
    const int qn = gq_load_tab(tabL, tab, S, ql);   // (its barrier covers the bins too)
    const int rows = T.Nt * T.nyl;
    const int lane = threadIdx.x & 63;
    const int nw = gridDim.x * (GQ_XNTH / 64);
    for (int row = blockIdx.x * (GQ_XNTH / 64) + (threadIdx.x >> 6); row < rows; row += nw) {
        const int kt = row / T.nyl, ky = T.y0 + (row - kt * T.nyl);
        const double rowmu = T.mt[kt] + T.my[ky];   // spec_lam's rowmu
        const double* src = bh + (int64_t)row * T.Nx;
        double* dst = out + (int64_t)row * T.Nx;
        if ((T.Nx % 2) == 0) {
            for (int kx = 2 * lane; kx < T.Nx; kx += 128) {
                const dbl2 v = ld_dead(reinterpret_cast<const dbl2*>(src + kx));
                const double lt0 = gq_s(T.r * (rowmu + T.mx[kx]), ic1);
                const double lt1 = gq_s(T.r * (rowmu + T.mx[kx + 1]), ic1);
                const int b0 = gq_find_bin(L.hi, L.cell, lt0);
                const int b1 = gq_fix_bin(L.hi, lt1, b0);   // lam increases with kx: the same bin or lower
                const double x0 = gq_q(tabL, tab, b0, (lt0 - L.mid[b0]) * L.ihw[b0], qn, ql) * v[0];
                const double x1 = gq_q(tabL, tab, b1, (lt1 - L.mid[b1]) * L.ihw[b1], qn, ql) * v[1];
                *reinterpret_cast<dbl2*>(dst + kx) = dbl2{x0, x1};
            }
        } else {
            for (int kx = lane; kx < T.Nx; kx += 64) {
                const double lt = gq_s(T.r * (rowmu + T.mx[kx]), ic1);
                const int b = gq_find_bin(L.hi, L.cell, lt);
                dst[kx] = gq_q(tabL, tab, b, (lt - L.mid[b]) * L.ihw[b], qn, ql) * src[kx];
            }
        }
    }
}
