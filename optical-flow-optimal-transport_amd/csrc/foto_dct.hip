// Per-axis DCT-II (forward) / DCT-III (inverse) passes of the spectral solver -- gfx950.
//
// Two implementations of the orthonormal transform along one axis of an array viewed as
// [outer][n][inner], both in fp64:
//   GEMM   (k_dct_axis, k_dct_axis_l): the n x n matrix applied on f64 MFMA
//          (v_mfma_f64_16x16x4_f64), 64 x 64 or 128 x 128 block tiles staged through LDS; any n.
//   FFT    (k_dct_fft_fwd / k_dct_fft_inv): Makhoul's reordering and a two-stage Cooley-Tukey
//          DFT of half the length with compile-time roots, lines staged in LDS; the lengths of
//          FOTO_FFT_SIZES from 64 up.
// The plan (foto_spectral.hip) calls the host wrappers declared in foto_dct.h; foto_dct at the
// end is the C test entry for one axis.
#include <cmath>
#include <cstdlib>
#include <vector>

#include "foto_dct.h"
#include "foto_devmem.h"
#include "foto_devutil.h"
#include "foto_twiddles.h"

namespace foto {

// ============================================================================ DCT along one axis (f64 MFMA GEMM)

constexpr int BM = 64, BN = 64, BK = 16;
constexpr int AS_LD = BK + 1;   // 17 doubles: column reads across 16 rows hit 16 distinct bank pairs
constexpr int BS_LD = BN + 16;  // 80 doubles = 160 dwords = 32 mod 64: the 4 k-rows of a read split the banks

// out[o][k][i] = sum_j M[k][j] in[o][j][i] over an array viewed as [outer][n][inner].
// CONTIG (inner == 1): GEMM rows = o, cols = k   (A = in rows, B = M^T)
// otherwise          : GEMM rows = k, cols = i, batch o = blockIdx.z (A = M, B = in[o])
template <bool CONTIG>
__global__ __launch_bounds__(256) void k_dct_axis(int outer, int n, int inner, const double* __restrict__ M,
                                                  const double* __restrict__ in, double* __restrict__ out) {
    __shared__ double As[BM * AS_LD];
    __shared__ double Bs[BK * BS_LD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w >> 1, wn = w & 1;
    int row0, col0;
    const double* inb;
    double* outb;
    int nrows, ncols;
    if (CONTIG) {
        row0 = blockIdx.y * BM;   // o
        col0 = blockIdx.x * BN;   // k
        nrows = outer;
        ncols = n;
        inb = in;
        outb = out;
    } else {
        row0 = blockIdx.y * BM;   // k
        col0 = blockIdx.x * BN;   // i
        nrows = n;
        ncols = inner;
        inb = in + (int64_t)blockIdx.z * n * inner;
        outb = out + (int64_t)blockIdx.z * n * inner;
    }
    dbl4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = dbl4{0.0, 0.0, 0.0, 0.0};

    for (int j0 = 0; j0 < n; j0 += BK) {
        // ---- stage A (BM x BK) and B (BK x BN)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + 256 * q;
            {   // A[m][kk]
                const int m = e >> 4, kk = e & 15;
                const int gr = row0 + m, gj = j0 + kk;
                double v = 0.0;
                if (gr < nrows && gj < n) v = CONTIG ? inb[(int64_t)gr * n + gj] : M[(int64_t)gr * n + gj];
                As[m * AS_LD + kk] = v;
            }
            if (CONTIG) {   // B[kk][c] = M[col0 + c][j0 + kk]
                const int c = e >> 4, kk = e & 15;
                const int gk = col0 + c, gj = j0 + kk;
                Bs[kk * BS_LD + c] = (gk < ncols && gj < n) ? M[(int64_t)gk * n + gj] : 0.0;
            } else {        // B[kk][c] = in[j0 + kk][col0 + c]
                const int kk = e >> 6, c = e & 63;
                const int gj = j0 + kk, gi = col0 + c;
                Bs[kk * BS_LD + c] = (gj < n && gi < ncols) ? inb[(int64_t)gj * inner + gi] : 0.0;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k4 = 0; k4 < BK / 4; ++k4) {
            const int kk = k4 * 4 + (lane >> 4);
            double a[2], b[2];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) a[mi] = As[(wm * 32 + mi * 16 + (lane & 15)) * AS_LD + kk];
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) b[ni] = Bs[kk * BS_LD + wn * 32 + ni * 16 + (lane & 15)];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
        }
        __syncthreads();
    }
    // ---- store: D[row = (lane>>4) + 4 r][col = lane & 15]
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gr = row0 + wm * 32 + mi * 16 + (lane >> 4) + 4 * r;
                const int gc = col0 + wn * 32 + ni * 16 + (lane & 15);
                if (gr < nrows && gc < ncols) {
                    if (CONTIG) outb[(int64_t)gr * n + gc] = acc[mi][ni][r];
                    else outb[(int64_t)gr * inner + gc] = acc[mi][ni][r];
                }
            }
}

// Large-tile variant: BM x BN = 128 x 128 per 256-thread block, each wave a 64 x 64
// sub-tile (4 x 4 MFMA 16x16x4 accumulators), BK = 16.  The next K-step's A/B elements are
// loaded into registers before the current step's MFMAs and written to the other LDS
// buffer after them (one barrier per K-step): global latency overlaps the matrix work and
// the loaded bytes per MFMA are half those of the 64 x 64 kernel.
constexpr int LBM = 128, LBN = 128, LBK = 16;
constexpr int LAS = LBK + 1;      // A row stride (doubles)
constexpr int LBS = LBN + 16;     // B row stride: 144 doubles = 288 dwords = 32 mod 64

template <bool CONTIG>
__global__ __launch_bounds__(256) void k_dct_axis_l(int outer, int n, int inner, const double* __restrict__ M,
                                                    const double* __restrict__ in, double* __restrict__ out) {
    __shared__ double As[2][LBM * LAS];
    __shared__ double Bs[2][LBK * LBS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w >> 1, wn = w & 1;
    const int row0 = blockIdx.y * LBM, col0 = blockIdx.x * LBN;
    const int nrows = CONTIG ? outer : n;
    const int ncols = CONTIG ? n : inner;
    const double* inb = CONTIG ? in : in + (int64_t)blockIdx.z * n * inner;
    double* outb = CONTIG ? out : out + (int64_t)blockIdx.z * n * inner;

    // staging map: 2048 A and 2048 B elements per K-step, 8 + 8 per thread
    double ra[8], rb[8];
    auto gload = [&](int j0) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = tid + 256 * q;
            {   // A[m][kk], m = e / 16
                const int m = e >> 4, kk = e & 15;
                const int gr = row0 + m, gj = j0 + kk;
                ra[q] = (gr < nrows && gj < n) ? (CONTIG ? inb[(int64_t)gr * n + gj] : M[(int64_t)gr * n + gj]) : 0.0;
            }
            if (CONTIG) {   // B[kk][c] = M[col0 + c][j0 + kk]
                const int c = e >> 4, kk = e & 15;
                const int gk = col0 + c, gj = j0 + kk;
                rb[q] = (gk < ncols && gj < n) ? M[(int64_t)gk * n + gj] : 0.0;
            } else {        // B[kk][c] = in[j0 + kk][col0 + c]
                const int kk = e >> 7, c = e & 127;
                const int gj = j0 + kk, gi = col0 + c;
                rb[q] = (gj < n && gi < ncols) ? inb[(int64_t)gj * inner + gi] : 0.0;
            }
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = tid + 256 * q;
            As[buf][(e >> 4) * LAS + (e & 15)] = ra[q];
            if (CONTIG) Bs[buf][(e & 15) * LBS + (e >> 4)] = rb[q];
            else Bs[buf][(e >> 7) * LBS + (e & 127)] = rb[q];
        }
    };

    dbl4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = dbl4{0.0, 0.0, 0.0, 0.0};

    gload(0);
    lstore(0);
    __syncthreads();
    int buf = 0;
    for (int j0 = 0; j0 < n; j0 += LBK) {
        const bool more = j0 + LBK < n;
        if (more) gload(j0 + LBK);
#pragma unroll
        for (int k4 = 0; k4 < LBK / 4; ++k4) {
            const int kk = k4 * 4 + (lane >> 4);
            double a[4], b[4];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) a[mi] = As[buf][(wm * 64 + mi * 16 + (lane & 15)) * LAS + kk];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) b[ni] = Bs[buf][kk * LBS + wn * 64 + ni * 16 + (lane & 15)];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
        }
        if (more) lstore(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gr = row0 + wm * 64 + mi * 16 + (lane >> 4) + 4 * r;
                const int gc = col0 + wn * 64 + ni * 16 + (lane & 15);
                if (gr < nrows && gc < ncols) {
                    if (CONTIG) outb[(int64_t)gr * n + gc] = acc[mi][ni][r];
                    else outb[(int64_t)gr * inner + gc] = acc[mi][ni][r];
                }
            }
}

hipError_t dct_axis(int outer, int n, int inner, const double* M, const double* in, double* out,
                           hipStream_t s) {
    // the t-axis (n = Nt, small) keeps the 64 x 64 tile; x and y use 128 x 128
    const bool large = n >= 96;
    if (inner == 1) {
        if (large) {
            dim3 grid((n + LBN - 1) / LBN, (outer + LBM - 1) / LBM, 1);
            k_dct_axis_l<true><<<grid, 256, 0, s>>>(outer, n, inner, M, in, out);
        } else {
            dim3 grid((n + BN - 1) / BN, (outer + BM - 1) / BM, 1);
            k_dct_axis<true><<<grid, 256, 0, s>>>(outer, n, inner, M, in, out);
        }
    } else {
        if (large) {
            dim3 grid((inner + LBN - 1) / LBN, (n + LBM - 1) / LBM, outer);
            k_dct_axis_l<false><<<grid, 256, 0, s>>>(outer, n, inner, M, in, out);
        } else {
            dim3 grid((inner + BN - 1) / BN, (n + BM - 1) / BM, outer);
            k_dct_axis<false><<<grid, 256, 0, s>>>(outer, n, inner, M, in, out);
        }
    }
    return hipGetLastError();
}

// ============================================================================ DCT along one axis (FFT)
//
// Orthonormal DCT-II (forward) / DCT-III (inverse) of real lines of even length N = 2M
// through a length-M complex DFT (Makhoul's reordering): v = (x0, x2, x4, ..., x5, x3, x1),
// z_j = v_2j + i v_2j+1, Z = DFT_M(z), then with C_k = conj Z_{(M-k) mod M}
//     V_k = (Z_k + C_k) / 2 + e^{-2 pi i k/N} (Z_k - C_k) / (2i)      (= DFT_N(v)_k)
//     Y_k = e^{-i pi k/(2N)} V_k,   X_k = s_k Re Y_k,   X_{N-k} = -s_{N-k} Im Y_k,
// s_0 = sqrt(1/N), s_k = sqrt(2/N).  The inverse runs the same steps backwards (V from X by
// Hermitian symmetry, Z_k = Ve_k + i Vo_k, z = IDFT_M(Z), x from v).  DFT_M is two-stage
// Cooley-Tukey, M = M1 M2: M2 DFTs of length M1 over the stride-M2 subsequences, twiddle
// e^{-2 pi i j2 k1 / M}, M1 DFTs of length M2; the small DFTs are direct with compile-time
// roots (foto_twiddles.h), so multiplications by 0 / +-1 fold away.  About 2 (M1 + M2) + 8
// fp64 FMA per element (75 at N = 640) instead of the GEMM's N; each axis pass reads and
// writes the volume once.  LPB lines per block are staged in LDS; transforms are in place
// within a line.  Lines are contiguous rows (CONTIG, the x axis) or strided columns (y, t)
// taken LPB consecutive columns at a time so global loads and stores stay coalesced.
//
// Per-axis table (fp64): WM[2M] = e^{-2 pi i p/M}, PA[2(M+1)] = e^{-2 pi i k/N},
// PB[2(M+1)] = e^{-i pi k/(2N)}, then s_0, s.

// LDS image of a line: complex element j (natural order, index M2 j1 + j2) at position
// j1 (M2 + 1) + j2 -- each M2-row padded by one complex, so stage 2 (one thread per row,
// lane stride M2 + 1 complex) is free of bank conflicts (unpadded, the stride is 2 M2
// doubles: 32-way conflicts at M2 = 16), while stage 1 still touches only its own
// positions (. (M2 + 1) + j2) and runs in place.
// Strided (y-axis) lines get a slightly larger LDS budget: at N = 1024 a line image is 8448 B,
// so 64 KB held 4 lines (32-B row segments) and 68 KB holds 8 (64 B; still two blocks per CU)
constexpr int FFT_STRIDED_LDS = 69632;
template <int M1, int M2, bool CONTIG = true>
struct FftGeom {
    static constexpr int M = M1 * M2, N = 2 * M;
    static constexpr int LS = 2 * M1 * (M2 + 1);   // doubles per line in LDS
    // lines per block: the LDS lines <= 64 KB (contiguous lines) / FFT_STRIDED_LDS; power-of-two
    // counts only (whole 128-B segments on strided axes)
    static constexpr int lpb() {
        const int c[7] = {64, 32, 16, 8, 4, 2, 1};
        const int budget = CONTIG ? 65536 : FFT_STRIDED_LDS;
        for (int i = 0; i < 7; ++i)
            if (c[i] * LS * 8 <= budget) return c[i];
        return 1;
    }
    static constexpr int LPB = lpb();
    static constexpr int TAB = 6 * M + 6;
    // the output / input phase twiddles (PA, PB of the table: 4 doubles per k = 0 .. M) staged in
    // LDS when that keeps the blocks per CU the LDS allows (x at 640: 3 of 43 + 10 KB; y at 480: 2
    // of 65 + 8 KB; not y at 1024, whose 8 lines already take 66 KB)
    static constexpr int PTN = 4 * (M + 1);
    static constexpr int LDS_B = LPB * LS * 8 + 16;
    static constexpr bool PT_LDS = (163840 / (LDS_B + 8 * PTN)) == (163840 / LDS_B);
};

// PT[4k .. 4k + 3] = (PA_k, PB_k): e^{-2 pi i k / N}, e^{-i pi k / (2N)}
template <class G>
__device__ __forceinline__ void fft_pt_fill(double* PT, const double* __restrict__ tab) {
    if constexpr (G::PT_LDS) {
        const double* PA = tab + 2 * G::M;
        const double* PB = PA + 2 * (G::M + 1);
        for (int p = threadIdx.x; p < G::M + 1; p += blockDim.x) {
            const double a0 = PA[2 * p], a1 = PA[2 * p + 1], b0 = PB[2 * p], b1 = PB[2 * p + 1];
            PT[4 * p] = a0;
            PT[4 * p + 1] = a1;
            PT[4 * p + 2] = b0;
            PT[4 * p + 3] = b1;
        }
    }
}

template <int M2>
__device__ __forceinline__ int fft_zpos(int j) { return j + j / M2; }   // natural index -> LDS complex position

template <int R, bool INV>
__device__ __forceinline__ constexpr double root_re(int p) { return Roots<R>::re[p]; }
template <int R, bool INV>
__device__ __forceinline__ constexpr double root_im(int p) { return INV ? -Roots<R>::im[p] : Roots<R>::im[p]; }

// acc += x * w (complex) with w a compile-time root: zero / unit parts fold away
template <int R, bool INV>
__device__ __forceinline__ void cmac_root(double& ar, double& ai, double xr, double xi, int p) {
    const double wr = root_re<R, INV>(p), wi = root_im<R, INV>(p);
    if (wr == 1.0) { ar += xr; ai += xi; }
    else if (wr == -1.0) { ar -= xr; ai -= xi; }
    else if (wr != 0.0) { ar = fma(xr, wr, ar); ai = fma(xi, wr, ai); }
    if (wi == 1.0) { ar -= xi; ai += xr; }
    else if (wi == -1.0) { ar += xi; ai -= xr; }
    else if (wi != 0.0) { ar = fma(-xi, wi, ar); ai = fma(xr, wi, ai); }
}

// In-register DFT of length R (natural order in and out), mixed radix: R = R1 R2 with R1
// the smallest of {4, 2, 3, 5} dividing R; R2 DFTs of length R1 over the stride-R2
// subsequences, twiddles e^{-+2 pi i n2 k1 / R}, R1 DFTs of length R2 -- all indices
// compile-time, roots folded (16 points: ~300 flops instead of 1024 FMA direct).
template <int R>
constexpr int dft_radix() {
    return (R % 4 == 0 && R > 4) ? 4 : (R % 2 == 0 && R > 2) ? 2 : (R % 3 == 0 && R > 3) ? 3 : (R % 5 == 0 && R > 5) ? 5 : R;
}

// Odd prime R (3, 5, 7, 19: the 640-, 480-, 420- and 380-point plans) by the symmetric pairs
// t_j = x_j + x_{R-j}, d_j = x_j - x_{R-j} (j = 1 .. H = (R - 1) / 2):
//   A_k = x_0 + sum_j cos(2 pi jk / R) t_j,  B_k = sum_j sin(2 pi jk / R) d_j,
//   forward X_k = A_k - i B_k, X_{R-k} = A_k + i B_k (inverse: swapped),
// about R real FMA per output instead of the direct codelet's 4R (roots compile-time).
template <int R, bool INV>
__device__ __forceinline__ void dft_sym(double (&xr)[R], double (&xi)[R]) {
    constexpr int H = (R - 1) / 2;
    double tr[H + 1], ti[H + 1], dr[H + 1], di[H + 1];
    double s0r = 0.0, s0i = 0.0;
#pragma unroll
    for (int j = 1; j <= H; ++j) {
        tr[j] = xr[j] + xr[R - j];
        ti[j] = xi[j] + xi[R - j];
        dr[j] = xr[j] - xr[R - j];
        di[j] = xi[j] - xi[R - j];
        s0r += tr[j];
        s0i += ti[j];
    }
    double ar[H + 1], ai[H + 1], br[H + 1], bi[H + 1];
#pragma unroll
    for (int k = 1; k <= H; ++k) {
        ar[k] = xr[0];
        ai[k] = xi[0];
        br[k] = 0.0;
        bi[k] = 0.0;
#pragma unroll
        for (int j = 1; j <= H; ++j) {
            const int p = (j * k) % R;
            const double c = Roots<R>::re[p], sn = -Roots<R>::im[p];   // cos, sin of 2 pi p / R
            ar[k] = fma(c, tr[j], ar[k]);
            ai[k] = fma(c, ti[j], ai[k]);
            br[k] = fma(sn, dr[j], br[k]);
            bi[k] = fma(sn, di[j], bi[k]);
        }
    }
    xr[0] += s0r;
    xi[0] += s0i;
#pragma unroll
    for (int k = 1; k <= H; ++k) {
        // A - i B = (ar + bi, ai - br);  A + i B = (ar - bi, ai + br)
        const int kf = INV ? R - k : k, kb = INV ? k : R - k;
        xr[kf] = ar[k] + bi[k];
        xi[kf] = ai[k] - br[k];
        xr[kb] = ar[k] - bi[k];
        xi[kb] = ai[k] + br[k];
    }
}

template <int R, bool INV>
__device__ __forceinline__ void dft_reg(double (&xr)[R], double (&xi)[R]) {
    constexpr int R1 = dft_radix<R>();
    if constexpr (R1 == R && R % 2 == 1 && R > 1) {
        dft_sym<R, INV>(xr, xi);
    } else if constexpr (R1 == R) {   // codelet: direct with compile-time roots
        double yr[R], yi[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            double ar = 0.0, ai = 0.0;
#pragma unroll
            for (int n = 0; n < R; ++n) cmac_root<R, INV>(ar, ai, xr[n], xi[n], (n * k) % R);
            yr[k] = ar;
            yi[k] = ai;
        }
#pragma unroll
        for (int k = 0; k < R; ++k) { xr[k] = yr[k]; xi[k] = yi[k]; }
    } else {
        constexpr int R2 = R / R1;
        double ar[R1][R2], ai[R1][R2];   // A[k1][n2]
#pragma unroll
        for (int n2 = 0; n2 < R2; ++n2) {
            double tr[R1], ti[R1];
#pragma unroll
            for (int n1 = 0; n1 < R1; ++n1) { tr[n1] = xr[R2 * n1 + n2]; ti[n1] = xi[R2 * n1 + n2]; }
            dft_reg<R1, INV>(tr, ti);
#pragma unroll
            for (int k1 = 0; k1 < R1; ++k1) {
                const int p = (n2 * k1) % R;
                const double wr = root_re<R, INV>(p), wi = root_im<R, INV>(p);
                if (p == 0) { ar[k1][n2] = tr[k1]; ai[k1][n2] = ti[k1]; }
                else { ar[k1][n2] = fma(tr[k1], wr, -ti[k1] * wi); ai[k1][n2] = fma(tr[k1], wi, ti[k1] * wr); }
            }
        }
#pragma unroll
        for (int k1 = 0; k1 < R1; ++k1) {
            dft_reg<R2, INV>(ar[k1], ai[k1]);
#pragma unroll
            for (int k2 = 0; k2 < R2; ++k2) { xr[k1 + R1 * k2] = ar[k1][k2]; xi[k1 + R1 * k2] = ai[k1][k2]; }
        }
    }
}

// stage 1 (in place on the LDS lines): for each (line, j2): the length-M1 DFT of
// z[M2 j1 + j2] (dft_reg), times e^{-+2 pi i j2 k1 / M}, stored at row k1, column j2
template <int M1, int M2, bool INV, int LPB, int NTH = 256>
__device__ __forceinline__ void fft_stage1(double* L, const double* TW) {
    constexpr int LS = FftGeom<M1, M2>::LS;
    for (int task = threadIdx.x; task < LPB * M2; task += NTH) {
        const int l = task / M2, j2 = task - (task / M2) * M2;
        double* Ll = L + l * LS;
        double xr[M1], xi[M1];
#pragma unroll
        for (int j1 = 0; j1 < M1; ++j1) {
            xr[j1] = Ll[2 * ((M2 + 1) * j1 + j2)];
            xi[j1] = Ll[2 * ((M2 + 1) * j1 + j2) + 1];
        }
        dft_reg<M1, INV>(xr, xi);
#pragma unroll
        for (int k1 = 0; k1 < M1; ++k1) {
            const int q = j2 * k1;   // < M
            const double tr = TW[2 * q];
            const double ti = INV ? -TW[2 * q + 1] : TW[2 * q + 1];
            Ll[2 * ((M2 + 1) * k1 + j2)] = fma(xr[k1], tr, -xi[k1] * ti);
            Ll[2 * ((M2 + 1) * k1 + j2) + 1] = fma(xr[k1], ti, xi[k1] * tr);
        }
    }
}

// stage 2 (in place): for each (line, k1): the length-M2 DFT of row k1; element
// k = k1 + M1 k2 of the result lands at row k1, column k2
template <int M1, int M2, bool INV, int LPB, int NTH = 256>
__device__ __forceinline__ void fft_stage2(double* L) {
    constexpr int LS = FftGeom<M1, M2>::LS;
    for (int task = threadIdx.x; task < LPB * M1; task += NTH) {
        const int l = task / M1, k1 = task - (task / M1) * M1;
        double* Lr = L + l * LS + 2 * (M2 + 1) * k1;
        double xr[M2], xi[M2];
#pragma unroll
        for (int j2 = 0; j2 < M2; ++j2) {
            xr[j2] = Lr[2 * j2];
            xi[j2] = Lr[2 * j2 + 1];
        }
        dft_reg<M2, INV>(xr, xi);
#pragma unroll
        for (int k2 = 0; k2 < M2; ++k2) {
            Lr[2 * k2] = xr[k2];
            Lr[2 * k2 + 1] = xi[k2];
        }
    }
}

// Stage 2 for a prime row length P too long for an in-register codelet (~2P live fp64
// registers: Middlebury's half-lengths 292 = 4 * 73 and 194 = 2 * 97).  Symmetric direct DFT:
// with u_j = z_j + z_{P-j}, v_j = z_j - z_{P-j} (j = 1 .. H, H = (P - 1) / 2),
//     A_k = z_0 + sum_j u_j cos(2 pi jk/P),   B_k = sum_j v_j sin(2 pi jk/P),   k = 0 .. H,
//     forward Z_k = A_k - i B_k, Z_{P-k} = A_k + i B_k       (inverse: the conjugate pairing).
// For all ROWS rows of the block the two sums are real GEMMs, (2 ROWS x H) (H x (H + 1)),
// run on the f64 MFMA (v_mfma_f64_16x16x4_f64): an M tile is 8 complex rows (tile rows 0-7
// their real parts, 8-15 their imaginary parts, so a lane's four results are the real and
// imaginary parts of two rows in one output column), K = H (a multiple of 4), N = H + 1
// padded to 16.  The B operands (cos, sin of 2 pi q / P) come from the P-entry root table CS in
// LDS, one 16-B read per k-step and N tile for both GEMMs.  (A direct per-output loop read
// ~48 B of LDS per multiply-add and was LDS-bound: 70-95 us per axis pass at 584x388x32.)
template <int P>
struct LdsPrime { static constexpr bool value = P > 32; };

template <int M1, int P, bool INV, int LPB, int NTH = 256>
__device__ __forceinline__ void fft_stage2_prime(double* L, const double* CS) {
    constexpr int LS = FftGeom<M1, P>::LS;
    constexpr int H = (P - 1) / 2;
    constexpr int ROWS = LPB * M1;
    constexpr int KS = H / 4, NTL = (H + 1 + 15) / 16, MT = ROWS / 8;
    constexpr int NW = NTH / 64;   // waves of the block (the M tiles are dealt to them)
    static_assert(H % 4 == 0 && ROWS % 8 == 0, "prime stage: K steps of 4, M tiles of 8 rows");
    static_assert(NTH % 64 == 0, "whole waves");
    for (int task = threadIdx.x; task < ROWS * H; task += NTH) {   // u, v in place
        const int row = task / H, j = 1 + task - row * H;
        const int l = row / M1, k1 = row - l * M1;
        double* Lr = L + l * LS + 2 * (P + 1) * k1;
        const double ar = Lr[2 * j], ai = Lr[2 * j + 1], br = Lr[2 * (P - j)], bi = Lr[2 * (P - j) + 1];
        Lr[2 * j] = ar + br;
        Lr[2 * j + 1] = ai + bi;
        Lr[2 * (P - j)] = ar - br;
        Lr[2 * (P - j) + 1] = ai - bi;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int am = lane & 15, ak = lane >> 4;   // A operand: row am, k ak of the step
    constexpr int MTW = (MT + NW - 1) / NW;     // M tiles per wave
    dbl4 dc[MTW][NTL], ds[MTW][NTL];
    double z0r[MTW][2], z0i[MTW][2];
#pragma unroll
    for (int w = 0; w < MTW; ++w) {
        const int mt = wave + NW * w;
        if (MT % NW != 0 && mt >= MT) continue;
        // this lane's A row: complex row 8 mt + (am & 7), real (am < 8) or imaginary part
        const int rowa = 8 * mt + (am & 7);
        const int offa = (rowa / M1) * LS + 2 * (P + 1) * (rowa % M1) + (am >> 3);
#pragma unroll
        for (int t = 0; t < NTL; ++t) { dc[w][t] = dbl4{0.0, 0.0, 0.0, 0.0}; ds[w][t] = dbl4{0.0, 0.0, 0.0, 0.0}; }
#pragma unroll 3
        for (int ks = 0; ks < KS; ++ks) {
            const int j = 4 * ks + ak + 1;
            const double au = L[offa + 2 * j], av = L[offa + 2 * (P - j)];
#pragma unroll
            for (int t = 0; t < NTL; ++t) {
                const int n = 16 * t + am;   // B operand: k ak, column n
                double bc = 0.0, bs = 0.0;
                if (n <= H) {
                    const int q = (j * n) % P;
                    bc = CS[2 * q];
                    bs = CS[2 * q + 1];
                }
                dc[w][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(au, bc, dc[w][t], 0, 0, 0);
                ds[w][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bs, ds[w][t], 0, 0, 0);
            }
        }
        // D rows of this lane: (lane >> 4) + 4 reg -> complex rows g, g + 4 of the tile (reg 0, 1
        // real, reg 2, 3 imaginary); their z_0
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = 8 * mt + (lane >> 4) + 4 * h;
            const double* Lr = L + (row / M1) * LS + 2 * (P + 1) * (row % M1);
            z0r[w][h] = Lr[0];
            z0i[w][h] = Lr[1];
        }
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < MTW; ++w) {
        const int mt = wave + NW * w;
        if (MT % NW != 0 && mt >= MT) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = 8 * mt + (lane >> 4) + 4 * h;
            double* Lr = L + (row / M1) * LS + 2 * (P + 1) * (row % M1);
#pragma unroll
            for (int t = 0; t < NTL; ++t) {
                const int k = 16 * t + (lane & 15);
                if (k > H) continue;
                const double Ar = z0r[w][h] + dc[w][t][h], Ai = z0i[w][h] + dc[w][t][2 + h];
                const double Br = ds[w][t][h], Bi = ds[w][t][2 + h];
                if (k == 0) {
                    Lr[0] = Ar;
                    Lr[1] = Ai;
                } else {
                    // A - i B = (Ar + Bi, Ai - Br);  A + i B = (Ar - Bi, Ai + Br)
                    const int kf = INV ? P - k : k, kb = INV ? k : P - k;
                    Lr[2 * kf] = Ar + Bi;
                    Lr[2 * kf + 1] = Ai - Br;
                    Lr[2 * kb] = Ar - Bi;
                    Lr[2 * kb + 1] = Ai + Br;
                }
            }
        }
    }
}

// the stage-2 variant for row length M2, and the LDS root table it needs (doubles)
template <int M1, int M2, bool INV, int LPB, int NTH = 256>
__device__ __forceinline__ void fft_stage2_any(double* L, const double* CS) {
    if constexpr (LdsPrime<M2>::value) fft_stage2_prime<M1, M2, INV, LPB, NTH>(L, CS);
    else fft_stage2<M1, M2, INV, LPB, NTH>(L);
}
template <int M2>
constexpr int fft_cs_len() { return LdsPrime<M2>::value ? 2 * M2 : 2; }

template <int M1, int M2>
__device__ __forceinline__ int fft_pos(int k) { return (M2 + 1) * (k % M1) + k / M1; }   // where Z_k lands

struct FftLines {   // this block's lines: CONTIG rows o0 + l, or columns (o0, i0 + l) of stride `inner`
    int o0, i0, nl;
};

// Strided lines (CONTIG = false: the y axis, element stride Nx) read LPB adjacent columns per
// block, LPB * 8 B of every row: 32 B at N = 1024 (LPB 4), a quarter of a 128-B line.  Blocks are
// dealt to the 8 XCDs round robin, so the neighbours that read the rest of each line sat on
// other XCDs and every XCD's L2 fetched the whole line (C4's y transforms ran at 1.6-1.8 TB/s).
// The swizzle gives each XCD a contiguous range of column groups: the blocks that share a
// line run on one XCD at about the same time.
template <bool CONTIG, int LPB>
__device__ __forceinline__ FftLines fft_lines(int outer, int inner) {
    FftLines f;
    if (CONTIG) {
        f.o0 = blockIdx.x * LPB;
        f.i0 = 0;
        f.nl = min(LPB, outer - f.o0);
    } else {
        int b = blockIdx.x;
        constexpr int NXCD = 8;
        const int nb = gridDim.x, per = nb / NXCD, rem = nb % NXCD, xcd = b % NXCD;
        b = xcd * per + min(xcd, rem) + b / NXCD;
        const int nib = (inner + LPB - 1) / LPB;
        f.o0 = b / nib;
        f.i0 = (b - f.o0 * nib) * LPB;
        f.nl = min(LPB, inner - f.i0);
    }
    return f;
}

// Phase loops run a compile-time number of rounds over idx = tid + 256 j (predicated), so a
// thread's global loads are all issued before the first is consumed: a tid-strided runtime
// loop compiled to load -> wait -> LDS store per element, one load in flight per thread.
template <int COUNT, int NTH = 256>
struct FftRounds {
    static constexpr int R = (COUNT + NTH - 1) / NTH;
    static __device__ __forceinline__ bool ok(int idx) { return COUNT % NTH == 0 || idx < COUNT; }
};

template <int M1, int M2, bool CONTIG, int NTH = 256>
__global__ __launch_bounds__(NTH) void k_dct_fft_fwd(int outer, int inner, const double* __restrict__ tab,
                                                     const double* __restrict__ in, double* __restrict__ out) {
    using G = FftGeom<M1, M2, CONTIG>;
    constexpr int M = G::M, N = G::N, LPB = G::LPB, LS = G::LS;
    __shared__ double L[LPB * LS];
    __shared__ double CS[fft_cs_len<M2>()];   // prime stage-2 roots (LdsPrime rows only)
    __shared__ __attribute__((aligned(16))) double PT[G::PT_LDS ? G::PTN : 2];
    const double* TW = tab;
    const int tid = threadIdx.x;
    const FftLines f = fft_lines<CONTIG, LPB>(outer, inner);
    if constexpr (LdsPrime<M2>::value)
        for (int p = tid; p < 2 * M2; p += NTH) CS[p] = tab[6 * M + 6 + p];
    fft_pt_fill<G>(PT, tab);
    const int64_t st = CONTIG ? 1 : inner;
    auto base = [&](int l) -> int64_t {
        return CONTIG ? (int64_t)(f.o0 + l) * N : (int64_t)f.o0 * N * inner + f.i0 + l;
    };
    {   // load (all rounds' loads in flight), then store in Makhoul order
        using RD = FftRounds<LPB * N, NTH>;
        // element j0 of this thread: (line l, position j); contiguous lines by line thread groups
        // (round 6: no index division per element)
        constexpr bool LT = CONTIG && NTH % LPB == 0 && N % (NTH / LPB) == 0 &&
                            N / (NTH / LPB) == RD::R;
        auto lj = [&](int j0, int& l, int& j) -> bool {
            if constexpr (LT) {
                l = tid / (NTH / LPB);
                j = tid - l * (NTH / LPB) + (NTH / LPB) * j0;
                return true;
            } else {
                const int idx = tid + NTH * j0;
                if (CONTIG) { l = idx / N; j = idx - l * N; }
                else { j = idx / LPB; l = idx - j * LPB; }
                return RD::ok(idx);
            }
        };
        double xv[RD::R];
#pragma unroll
        for (int j0 = 0; j0 < RD::R; ++j0) {
            int l, j;
            const bool ok = lj(j0, l, j);
            xv[j0] = (ok && l < f.nl) ? ld_dead(&in[base(l) + j * st]) : 0.0;
        }
#pragma unroll
        for (int j0 = 0; j0 < RD::R; ++j0) {
            int l, j;
            if (!lj(j0, l, j)) continue;
            const int p = (j & 1) ? N - 1 - (j >> 1) : (j >> 1);
            L[l * LS + 2 * fft_zpos<M2>(p >> 1) + (p & 1)] = xv[j0];
        }
    }
    __syncthreads();
    fft_stage1<M1, M2, false, LPB, NTH>(L, TW);
    __syncthreads();
    fft_stage2_any<M1, M2, false, LPB, NTH>(L, CS);
    __syncthreads();
    const double* PA = tab + 2 * M;
    const double* PB = PA + 2 * (M + 1);
    const double s0 = PB[2 * (M + 1)], s = PB[2 * (M + 1) + 1];
    auto emit = [&](int l, int k) {   // X_k and X_{N-k} of line l
        const double* Ll = L + l * LS;
        const int pa = 2 * fft_pos<M1, M2>(k == M ? 0 : k), pb = 2 * fft_pos<M1, M2>(k == 0 ? 0 : M - k);
        const double zr = Ll[pa], zi = Ll[pa + 1], cr = Ll[pb], ci = -Ll[pb + 1];
        const double er = 0.5 * (zr + cr), ei = 0.5 * (zi + ci);     // DFT of the even samples
        const double orr = 0.5 * (zi - ci), oi = 0.5 * (cr - zr);     // DFT of the odd samples
        double war, wai, wbr, wbi;
        if constexpr (G::PT_LDS) {
            const dbl2 a = *reinterpret_cast<const dbl2*>(&PT[4 * k]), b = *reinterpret_cast<const dbl2*>(&PT[4 * k + 2]);
            war = a.x; wai = a.y; wbr = b.x; wbi = b.y;
        } else {
            war = PA[2 * k]; wai = PA[2 * k + 1]; wbr = PB[2 * k]; wbi = PB[2 * k + 1];
        }
        const double vr = er + fma(war, orr, -wai * oi), vi = ei + fma(war, oi, wai * orr);
        const double yr = fma(wbr, vr, -wbi * vi), yi = fma(wbr, vi, wbi * vr);
        const int64_t b = base(l);
        out[b + k * st] = (k == 0 ? s0 : s) * yr;
        if (k > 0 && k < M) out[b + (N - k) * st] = -s * yi;
    };
    if constexpr (CONTIG && NTH % LPB == 0) {
        // (round 6) a fixed line per thread group of NTH / LPB threads, k = t, t + TPL, ...: no
        // index division per element, and the line test hoisted out of the rounds
        constexpr int TPL = NTH / LPB, RK = (M + 1 + TPL - 1) / TPL;
        const int l = tid / TPL, t = tid - l * TPL;
        if (l < f.nl) {
#pragma unroll
            for (int r = 0; r < RK; ++r) {
                const int k = t + TPL * r;
                if ((M + 1) % TPL != 0 && r == RK - 1 && k > M) break;
                emit(l, k);
            }
        }
    } else {
        using RO = FftRounds<LPB * (M + 1), NTH>;
#pragma unroll
        for (int j0 = 0; j0 < RO::R; ++j0) {
            const int idx = tid + NTH * j0;
            if (!RO::ok(idx)) continue;
            int l, k;
            if (CONTIG) { l = idx / (M + 1); k = idx - l * (M + 1); }
            else { k = idx / LPB; l = idx - k * LPB; }
            if (l >= f.nl) continue;
            emit(l, k);
        }
    }
}

template <int M1, int M2, bool CONTIG, int NTH = 256>
__global__ __launch_bounds__(NTH) void k_dct_fft_inv(int outer, int inner, const double* __restrict__ tab,
                                                     const double* __restrict__ in, double* __restrict__ out) {
    using G = FftGeom<M1, M2, CONTIG>;
    constexpr int M = G::M, N = G::N, LPB = G::LPB, LS = G::LS;
    __shared__ double L[LPB * LS];
    __shared__ double CS[fft_cs_len<M2>()];   // prime stage-2 roots (LdsPrime rows only)
    __shared__ __attribute__((aligned(16))) double PT[G::PT_LDS ? G::PTN : 2];
    const double* TW = tab;
    const int tid = threadIdx.x;
    const FftLines f = fft_lines<CONTIG, LPB>(outer, inner);
    if constexpr (LdsPrime<M2>::value)
        for (int p = tid; p < 2 * M2; p += NTH) CS[p] = tab[6 * M + 6 + p];
    fft_pt_fill<G>(PT, tab);
    const int64_t st = CONTIG ? 1 : inner;
    auto base = [&](int l) -> int64_t {
        return CONTIG ? (int64_t)(f.o0 + l) * N : (int64_t)f.o0 * N * inner + f.i0 + l;
    };
    const double* PA = tab + 2 * M;
    const double* PB = PA + 2 * (M + 1);
    const double is0 = 1.0 / PB[2 * (M + 1)], is = 1.0 / PB[2 * (M + 1) + 1];
    // Z_k and Z_{M-k} need the same four inputs X_k, X_{N-k}, X_{M-k}, X_{M+k} (V_k and V_{M-k},
    // conjugated in the other's formula), so one thread makes both: k in [0, M/2], half the
    // global reads of one Z per thread (L2-resident lines, read straight from global; no LDS
    // image of X, so Z is written once and nothing is held in registers across a barrier)
    constexpr int MH = M / 2 + 1;
    using RP = FftRounds<LPB * MH, NTH>;
    // element j0 of this thread: (line l, k); contiguous lines by line thread groups (round 6)
    constexpr bool LT = CONTIG && NTH % LPB == 0 &&
                        (MH + NTH / LPB - 1) / (NTH / LPB) == RP::R;
    auto lk = [&](int j0, int& l, int& k) -> bool {
        if constexpr (LT) {
            l = tid / (NTH / LPB);
            k = tid - l * (NTH / LPB) + (NTH / LPB) * j0;
            return k < MH;
        } else {
            const int idx = tid + NTH * j0;
            if (CONTIG) { l = idx / MH; k = idx - l * MH; }
            else { k = idx / LPB; l = idx - k * LPB; }
            return RP::ok(idx);
        }
    };
    double xk[RP::R], xnk[RP::R], xmk[RP::R], xpk[RP::R];   // X_k, X_{N-k}, X_{M-k}, X_{N-M+k}
#pragma unroll
    for (int j0 = 0; j0 < RP::R; ++j0) {   // all rounds' loads first
        int l, k;
        const bool ok = lk(j0, l, k);
        xk[j0] = xnk[j0] = xmk[j0] = xpk[j0] = 0.0;
        if (ok && l < f.nl) {
            const double* X = in + base(l);
            xk[j0] = ld_dead(&X[k * st]);
            if (k != 0) xnk[j0] = ld_dead(&X[(N - k) * st]);
            xmk[j0] = ld_dead(&X[(M - k) * st]);
            if (M - k != 0) xpk[j0] = ld_dead(&X[(N - (M - k)) * st]);
        }
    }
    if constexpr (G::PT_LDS) __syncthreads();   // (PT; the X loads stay in flight across it)
#pragma unroll
    for (int j0 = 0; j0 < RP::R; ++j0) {
        int l, k;
        if (!lk(j0, l, k)) continue;
        // V_j = e^{+i pi j/(2N)} Y_j, Y_j = (X_j / s_j, -X_{N-j} / s_{N-j}), j in {k, M - k}
        auto V = [&](int j, double xj, double xnj, double& vr, double& vi) {
            const double yr = xj * (j == 0 ? is0 : is), yi = (j == 0) ? 0.0 : -xnj * is;
            double wbr, wbi;
            if constexpr (G::PT_LDS) {
                const dbl2 b = *reinterpret_cast<const dbl2*>(&PT[4 * j + 2]);
                wbr = b.x;
                wbi = -b.y;
            } else {
                wbr = PB[2 * j];
                wbi = -PB[2 * j + 1];
            }
            vr = fma(wbr, yr, -wbi * yi);
            vi = fma(wbr, yi, wbi * yr);
        };
        // Z_q from V_q = (ar, ai) and V_{M-q} = (br, bi)
        auto Zq = [&](int q, double ar, double ai, double br, double bi, double& zr, double& zi) {
            bi = -bi;                                                  // conj V_{M-q} = V_{q+M}
            const double er = 0.5 * (ar + br), ei = 0.5 * (ai + bi);   // Ve_q
            const double dr = 0.5 * (ar - br), di = 0.5 * (ai - bi);
            double war, wai;                                           // e^{+2 pi i q/N}
            if constexpr (G::PT_LDS) {
                const dbl2 a = *reinterpret_cast<const dbl2*>(&PT[4 * q]);
                war = a.x;
                wai = -a.y;
            } else {
                war = PA[2 * q];
                wai = -PA[2 * q + 1];
            }
            const double orr = fma(war, dr, -wai * di), oi = fma(war, di, wai * dr);   // Vo_q
            zr = er - oi;                                              // Z = Ve + i Vo
            zi = ei + orr;
        };
        double z1r = 0.0, z1i = 0.0, z2r = 0.0, z2i = 0.0;
        if (l < f.nl) {
            double ar, ai, br, bi;
            V(k, xk[j0], xnk[j0], ar, ai);
            V(M - k, xmk[j0], xpk[j0], br, bi);
            Zq(k, ar, ai, br, bi, z1r, z1i);
            Zq(M - k, br, bi, ar, ai, z2r, z2i);
        }
        L[l * LS + 2 * fft_zpos<M2>(k)] = z1r;
        L[l * LS + 2 * fft_zpos<M2>(k) + 1] = z1i;
        if (k != 0 && 2 * k != M) {   // Z_{M-k} (k = 0: M - k = M is no Z index; 2k = M: the same Z)
            L[l * LS + 2 * fft_zpos<M2>(M - k)] = z2r;
            L[l * LS + 2 * fft_zpos<M2>(M - k) + 1] = z2i;
        }
    }
    __syncthreads();
    fft_stage1<M1, M2, true, LPB, NTH>(L, TW);
    __syncthreads();
    fft_stage2_any<M1, M2, true, LPB, NTH>(L, CS);
    __syncthreads();
    constexpr double iM = 1.0 / M;
    if constexpr (CONTIG && NTH % LPB == 0 && N % (NTH / LPB) == 0) {
        constexpr int TPL = NTH / LPB, RI = N / TPL;   // (round 6) a fixed line per thread group
        const int l = tid / TPL, t = tid - l * TPL;
        if (l < f.nl) {
            const double* Ll = L + l * LS;
            double* o = out + base(l);
#pragma unroll
            for (int r = 0; r < RI; ++r) {   // x_i = v_p, p = Makhoul position of i
                const int i = t + TPL * r;
                const int p = (i & 1) ? N - 1 - (i >> 1) : (i >> 1);
                o[i] = Ll[2 * fft_pos<M1, M2>(p >> 1) + (p & 1)] * iM;
            }
        }
    } else {
        using RS = FftRounds<LPB * N, NTH>;
#pragma unroll
        for (int j0 = 0; j0 < RS::R; ++j0) {   // x_i = v_p, p = Makhoul position of i
            const int idx = tid + NTH * j0;
            if (!RS::ok(idx)) continue;
            int l, i;
            if (CONTIG) { l = idx / N; i = idx - l * N; }
            else { i = idx / LPB; l = idx - i * LPB; }
            if (l >= f.nl) continue;
            const int p = (i & 1) ? N - 1 - (i >> 1) : (i >> 1);
            out[base(l) + i * st] = L[l * LS + 2 * fft_pos<M1, M2>(p >> 1) + (p & 1)] * iM;
        }
    }
}

// supported line lengths N = 2 M1 M2 (others use the GEMM kernels)
#define FOTO_FFT_SIZES(X) X(8, 2, 2) X(16, 2, 4) X(32, 4, 4) X(64, 4, 8) X(128, 8, 8) X(256, 8, 16) \
    X(146, 1, 73) X(194, 1, 97) X(380, 10, 19) X(388, 2, 97) X(420, 14, 15) X(480, 15, 16) X(512, 16, 16) X(584, 4, 73) X(640, 16, 20)    \
    X(1024, 16, 32)

bool fft_factors(int n, int* m1, int* m2) {
#define FOTO_FFT_CASE(NN, A, B) if (n == NN) { *m1 = A; *m2 = B; return true; }
    FOTO_FFT_SIZES(FOTO_FFT_CASE)
#undef FOTO_FFT_CASE
    return false;
}

// per-axis table (host, long double): see the layout above
std::vector<double> fft_table(int n) {
    const int M = n / 2;
    std::vector<double> t;
    const long double pi = 3.141592653589793238462643383279502884L;
    for (int p = 0; p < M; ++p) {
        t.push_back((double)cosl(2.0L * pi * p / M));
        t.push_back((double)-sinl(2.0L * pi * p / M));
    }
    for (int k = 0; k <= M; ++k) {
        t.push_back((double)cosl(2.0L * pi * k / n));
        t.push_back((double)-sinl(2.0L * pi * k / n));
    }
    for (int k = 0; k <= M; ++k) {
        t.push_back((double)cosl(pi * k / (2.0L * n)));
        t.push_back((double)-sinl(pi * k / (2.0L * n)));
    }
    t.push_back((double)sqrtl(1.0L / n));
    t.push_back((double)sqrtl(2.0L / n));
    int m1 = 0, m2 = 0;
    if (fft_factors(n, &m1, &m2) && m2 > 32)   // LdsPrime rows: cos, sin of 2 pi q / m2 (at 6 M + 6)
        for (int q = 0; q < m2; ++q) {
            t.push_back((double)cosl(2.0L * pi * q / m2));
            t.push_back((double)sinl(2.0L * pi * q / m2));
        }
    return t;
}

// threads per block of the contiguous (x) and strided (y, t) axis passes
constexpr int FFT_NTH_C = 256, FFT_NTH_S = 256;

// FFT path along one axis of [outer][n][inner]; hipErrorNotSupported if n has no instantiation
// or the caller holds no table (tab == nullptr: Tuning::dct_fft off, the GEMM kernels on every axis)
hipError_t dct_fft_axis(int outer, int n, int inner, bool inv, const double* tab, const double* in,
                               double* out, hipStream_t s) {
    int m1, m2;
    // n < 64: the GEMM kernel is as fast (t axis at 32: 49 vs 54 us)
    if (!tab || n < 64 || !fft_factors(n, &m1, &m2)) return hipErrorNotSupported;
#define FOTO_FFT_LAUNCH(NN, A, B)                                                                  \
    if (n == NN) {                                                                                 \
        const bool contig = (inner == 1);                                                          \
        const int LPB = contig ? FftGeom<A, B, true>::LPB : FftGeom<A, B, false>::LPB;             \
        const int nb = contig ? (outer + LPB - 1) / LPB : outer * ((inner + LPB - 1) / LPB);       \
        if (contig) {                                                                              \
            if (inv) k_dct_fft_inv<A, B, true, FFT_NTH_C><<<nb, FFT_NTH_C, 0, s>>>(outer, inner, tab, in, out); \
            else k_dct_fft_fwd<A, B, true, FFT_NTH_C><<<nb, FFT_NTH_C, 0, s>>>(outer, inner, tab, in, out);     \
        } else {                                                                                   \
            if (inv) k_dct_fft_inv<A, B, false, FFT_NTH_S><<<nb, FFT_NTH_S, 0, s>>>(outer, inner, tab, in, out); \
            else k_dct_fft_fwd<A, B, false, FFT_NTH_S><<<nb, FFT_NTH_S, 0, s>>>(outer, inner, tab, in, out);     \
        }                                                                                          \
        return hipGetLastError();                                                                  \
    }
    FOTO_FFT_SIZES(FOTO_FFT_LAUNCH)
#undef FOTO_FFT_LAUNCH
    return hipErrorNotSupported;
}

// orthonormal DCT-II matrix C[k][j] = s_k cos(pi k (2j+1) / (2n)) (long double on the host)
// eigenvalues 2 - 2 cos(pi k / n) of the Neumann second difference (the same values dct_matrix gives)
void dct_eigen(int n, std::vector<double>& mu) {
    mu.assign(n, 0.0);
    const long double pi = 3.141592653589793238462643383279502884L;
    for (int k = 0; k < n; ++k) mu[k] = (double)(2.0L - 2.0L * cosl(pi * k / n));
}

void dct_matrix(int n, std::vector<double>& C, std::vector<double>& CT, std::vector<double>& mu) {
    C.assign((size_t)n * n, 0.0);
    CT.assign((size_t)n * n, 0.0);
    mu.assign(n, 0.0);
    const long double pi = 3.141592653589793238462643383279502884L;
    for (int k = 0; k < n; ++k) {
        const long double s = (k == 0) ? sqrtl(1.0L / n) : sqrtl(2.0L / n);
        for (int j = 0; j < n; ++j) {
            const double v = (double)(s * cosl(pi * k * (2.0L * j + 1.0L) / (2.0L * n)));
            C[(size_t)k * n + j] = v;
            CT[(size_t)j * n + k] = v;
        }
        mu[k] = (double)(2.0L - 2.0L * cosl(pi * k / n));
    }
}

}  // namespace foto

// ============================================================================ C ABI: one DCT axis (test entry)

extern "C" int foto_dct(const double* in, int outer, int n, int inner, int inverse, int path, double* out) {
    using namespace foto;
    const Tuning tn = tuning_from_env();   // (a context-free entry: read here, once per call)
    if (!in || !out || outer < 1 || n < 2 || inner < 1 || path < 0 || path > 2) {
        set_error("foto_dct: bad arguments");
        return FOTO_ERR_ARG;
    }
    const size_t tot = (size_t)outer * n * inner;
    CallScope S;
    FOTO_TRY(S.init());
    double *din, *dout, *dtab = nullptr, *dC;
    FOTO_TRY(S.up(in, tot, &din));
    FOTO_TRY(S.dev(tot, &dout));
    int m1, m2;
    hipError_t e = hipErrorNotSupported;
    if (path != 2 && tn.dct_fft && fft_factors(n, &m1, &m2)) {
        const std::vector<double> t = fft_table(n);   // (host table: the sync below ends the copy from it)
        FOTO_TRY(S.up(t.data(), t.size(), &dtab));
        FOTO_TRY(S.sync());
        e = dct_fft_axis(outer, n, inner, inverse != 0, dtab, din, dout, S.s);
    }
    if (e == hipErrorNotSupported) {
        if (path == 1) { set_error("foto_dct: no FFT plan for n = %d", n); return FOTO_ERR_ARG; }
        std::vector<double> C, CT, mu;
        dct_matrix(n, C, CT, mu);
        FOTO_TRY(S.up(inverse ? CT.data() : C.data(), C.size(), &dC));
        FOTO_TRY(S.sync());
        e = dct_axis(outer, n, inner, dC, din, dout, S.s);
    }
    FOTO_HIP_CHECK(e);
    FOTO_TRY(S.down(out, dout, tot));
    return S.sync();
}
