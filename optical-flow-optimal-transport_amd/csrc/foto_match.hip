// libfoto: feature matching on gfx950 -- 256-bit binary descriptors at points (BRIEF, Calonder et
// al. 2010; the intensity-centroid orientation of Rublee et al. 2011), the nearest and
// second-nearest descriptor under the Hamming distance, and the mutual check.  include/foto.h has
// the arithmetic; tests/match_ref.py restates it in numpy and the device is held to it bit for bit
// (-ffp-contract=off, the two moment sums in one fixed order; everything else is integer).
//
//   launch_ingest      the frame widened to [h][w]
//   k_box_h, k_box_v   the smoothed plane: horizontal then vertical box sums, a thread per pixel
//   k_describe         one wavefront per point, four per block: the moments lane-serial then
//                      wave_sum's tree, the bin in every lane, the 256 tests as four ballots
//   k_match            the hot kernel, N0 x N1 distances: block (x, y) holds FOTO_MATCH_QUERIES
//                      query descriptors in registers (two per lane, 16 VGPRs) and walks split y of
//                      the train set in LDS tiles of FOTO_MATCH_TILE descriptors, read at one
//                      address by the whole wave (a broadcast); XOR, popcount with its accumulate
//                      operand, and a branch-free update of (d1, j1, d2) per pair.  A train entry
//                      that is no candidate carries a penalty above every distance instead of a
//                      branch: its state's part is in the LDS tile, the gate's is a select
//   k_match_finish     the splits' partial (d1, j1, d2) merged in split order; status, idx, dist, disp
//   k_match_cross      the mutual check
// Bound by integer VALU issue.  No atomics; nothing waits for the host.
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "foto_devmem.h"
#include "foto_devutil.h"
#include "foto_reduce.h"

namespace foto {
namespace {

constexpr int MA_Q = 2;                       // queries per lane
constexpr int MA_QB = MA_Q * NT;              // queries per block
constexpr int MA_T = FOTO_MATCH_TILE;         // train descriptors per LDS tile: one per thread
constexpr int MA_PEN = 512;                   // a non-candidate's distance starts here: above 256, below MA_FAR
constexpr int MA_FAR = 4096;                  // "nothing seen yet"; and the padding of a partial tile
constexpr int MA_U = 4;                       // train entries per round of the unrolled loop
constexpr int MA_NONE = 257;
static_assert(MA_QB == FOTO_MATCH_QUERIES && MA_T == NT && MA_T % MA_U == 0, "the sizes of include/foto.h");

// ----------------------------------------------------------------------------- the smoothed plane

__global__ __launch_bounds__(NT) void k_box_h(int w, int64_t n, int c, const double* __restrict__ f,
                                              double* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (t >= n) return;
    const int64_t j = t / w;
    const int i = (int)(t - j * w);
    const double* row = f + j * w;
    double s = i - c >= 0 ? row[i - c] : 0.0;
    for (int dx = -c + 1; dx <= c; ++dx) {
        const int x = i + dx;
        s += (x >= 0 && x < w) ? row[x] : 0.0;
    }
    out[t] = s;
}

__global__ __launch_bounds__(NT) void k_box_v(int w, int h, int64_t n, int c, const double* __restrict__ f,
                                              double* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (t >= n) return;
    const int j = (int)(t / w);
    const int i = (int)(t - (int64_t)j * w);
    double s = j - c >= 0 ? f[(int64_t)(j - c) * w + i] : 0.0;
    for (int dy = -c + 1; dy <= c; ++dy) {
        const int y = j + dy;
        s += (y >= 0 && y < h) ? f[(int64_t)y * w + i] : 0.0;
    }
    out[t] = s;
}

// ----------------------------------------------------------------------------- descriptors

struct DescPar {
    int w, h, patch, K;
};

template <class TP>
__global__ __launch_bounds__(NT) void k_describe(DescPar P, const double* __restrict__ F, const double* __restrict__ B,
                                                 const TP* __restrict__ pts, int64_t M,
                                                 const int* __restrict__ pattern, const double* __restrict__ dirs,
                                                 unsigned long long* __restrict__ desc,
                                                 unsigned char* __restrict__ state, int* __restrict__ bin_out) {
    const int lane = threadIdx.x & 63;
    const int64_t pt = (int64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (pt >= M) return;   // (a whole wave)
    const double x = (double)pts[2 * pt], y = (double)pts[2 * pt + 1];
    const double fi = floor(x + 0.5), fj = floor(y + 0.5);
    const int R = P.patch;
    unsigned st = 0;
    if (!(isfinite(x) && isfinite(y))) st = FOTO_MATCH_NONFINITE | FOTO_MATCH_OUT;
    else if (!(fi >= (double)R && fi <= (double)(P.w - 1 - R) && fj >= (double)R && fj <= (double)(P.h - 1 - R)))
        st = FOTO_MATCH_OUT;
    if (st) {   // (the same in every lane of the wave, like every branch below)
        if (lane < 4) desc[4 * pt + lane] = 0ULL;
        if (lane == 0) {
            state[pt] = (unsigned char)st;
            if (bin_out) bin_out[pt] = -1;
        }
        return;
    }
    const int i = (int)fi, j = (int)fj;
    int bin = 0;
    if (P.K > 1) {
        const int side = 2 * R + 1, n = side * side, slots = (n + 63) / 64;
        double s10 = 0.0, s01 = 0.0;
        for (int q = 0; q < slots; ++q) {
            const int e = lane + 64 * q;
            double t10 = 0.0, t01 = 0.0;
            if (e < n) {
                const int r = e / side, ay = r - R, ax = e - r * side - R;
                if (ax * ax + ay * ay <= R * R) {
                    const double v = F[(int64_t)(j + ay) * P.w + (i + ax)];
                    t10 = (double)ax * v;
                    t01 = (double)ay * v;
                }
            }
            s10 = q == 0 ? t10 : s10 + t10;
            s01 = q == 0 ? t01 : s01 + t01;
        }
        const double m10 = dbl_readlane(wave_sum(s10), 0), m01 = dbl_readlane(wave_sum(s01), 0);
        double held = m10 * dirs[0] + m01 * dirs[1];
        for (int k = 1; k < P.K; ++k) {
            const double v = m10 * dirs[2 * k] + m01 * dirs[2 * k + 1];
            if (v > held) {
                held = v;
                bin = k;
            }
        }
    }
    const int* row = pattern + bin * 256;
#pragma unroll
    for (int nw = 0; nw < 4; ++nw) {
        const int pk = row[64 * nw + lane];   // (ax, ay, bx, by) as four signed bytes
        const int ax = (signed char)(pk & 0xff), ay = (signed char)((pk >> 8) & 0xff);
        const int bx = (signed char)((pk >> 16) & 0xff), by = (signed char)((pk >> 24) & 0xff);
        const double a = B[(int64_t)(j + ay) * P.w + (i + ax)], b = B[(int64_t)(j + by) * P.w + (i + bx)];
        const unsigned long long word = __ballot(a < b);
        if (lane == 0) desc[4 * pt + nw] = word;
    }
    if (lane == 0) {
        state[pt] = 0;
        if (bin_out) bin_out[pt] = bin;
    }
}

// ----------------------------------------------------------------------------- the matcher

// acc + the set bits of x in one instruction: v_bcnt_u32_b32 adds its second operand.  Written out
// because hipcc turns `acc + __popc(x)` chains into bcnt-with-zero and a tree of v_add3 (four more
// instructions per pair in this VALU-bound loop); a register-only VALU statement, so the compiler
// still orders it after the LDS reads that feed it.
__device__ __forceinline__ int popc_acc(unsigned x, int acc) {
    int r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}

// part[(s * 3 + c) * N0 + q]: split s's d1, j1, d2 of query q (a non-candidate's d >= MA_PEN)
template <bool GATE, class TP0, class TP1>
__global__ __launch_bounds__(NT) void k_match(const uint4* __restrict__ desc0, const TP0* __restrict__ pts0, int N0,
                                              const uint4* __restrict__ desc1,
                                              const unsigned char* __restrict__ state1,
                                              const TP1* __restrict__ pts1, int N1, int chunk, double r,
                                              int* __restrict__ part) {
    __shared__ uint4 sd[2 * MA_T];
    __shared__ int spen[MA_T];
    __shared__ double sx[GATE ? MA_T : 1], sy[GATE ? MA_T : 1];
    unsigned q[MA_Q][8];
    double x0[MA_Q], y0[MA_Q];
    int d1[MA_Q], d2[MA_Q], j1[MA_Q];
#pragma unroll
    for (int k = 0; k < MA_Q; ++k) {
        const int64_t qi = (int64_t)blockIdx.x * MA_QB + k * NT + threadIdx.x;
        const int64_t qq = qi < N0 ? qi : 0;   // (a lane past N0 works on query 0 and stores nothing)
        const uint4 a = desc0[2 * qq], b = desc0[2 * qq + 1];
        q[k][0] = a.x; q[k][1] = a.y; q[k][2] = a.z; q[k][3] = a.w;
        q[k][4] = b.x; q[k][5] = b.y; q[k][6] = b.z; q[k][7] = b.w;
        x0[k] = GATE ? (double)pts0[2 * qq] : 0.0;
        y0[k] = GATE ? (double)pts0[2 * qq + 1] : 0.0;
        d1[k] = d2[k] = MA_FAR;
        j1[k] = -1;
    }
    const int64_t t0 = (int64_t)blockIdx.y * chunk;
    const int64_t t1 = min(t0 + (int64_t)chunk, (int64_t)N1);
    for (int64_t base64 = t0; base64 < t1; base64 += MA_T) {
        const int base = (int)base64, m = (int)min((int64_t)MA_T, t1 - base64);
        const int m4 = (m + MA_U - 1) & ~(MA_U - 1);   // (the tile is walked in groups of MA_U entries)
        __syncthreads();   // (the previous tile has been read)
        if ((int)threadIdx.x < m) {
            const int64_t j = (int64_t)base + threadIdx.x;
            sd[2 * threadIdx.x] = desc1[2 * j];
            sd[2 * threadIdx.x + 1] = desc1[2 * j + 1];
            spen[threadIdx.x] = state1[j] != 0 ? MA_PEN : 0;
            if constexpr (GATE) {
                sx[threadIdx.x] = (double)pts1[2 * j];
                sy[threadIdx.x] = (double)pts1[2 * j + 1];
            }
        } else if ((int)threadIdx.x < m4) {   // past the end: an entry that changes nothing, d >= MA_FAR
            sd[2 * threadIdx.x] = sd[2 * threadIdx.x + 1] = make_uint4(0, 0, 0, 0);
            spen[threadIdx.x] = MA_FAR;
            if constexpr (GATE) sx[threadIdx.x] = sy[threadIdx.x] = 0.0;
        }
        __syncthreads();
        for (int t0u = 0; t0u < m4; t0u += MA_U) {
#pragma unroll
            for (int u = 0; u < MA_U; ++u) {
                const int t = t0u + u;
                const uint4 a = sd[2 * t], b = sd[2 * t + 1];
                const int pen = spen[t];
                const int j = base + t;
                const double x1 = GATE ? sx[t] : 0.0, y1 = GATE ? sy[t] : 0.0;
#pragma unroll
                for (int k = 0; k < MA_Q; ++k) {
                    int d = pen;
                    d = popc_acc(q[k][0] ^ a.x, d);
                    d = popc_acc(q[k][1] ^ a.y, d);
                    d = popc_acc(q[k][2] ^ a.z, d);
                    d = popc_acc(q[k][3] ^ a.w, d);
                    d = popc_acc(q[k][4] ^ b.x, d);
                    d = popc_acc(q[k][5] ^ b.y, d);
                    d = popc_acc(q[k][6] ^ b.z, d);
                    d = popc_acc(q[k][7] ^ b.w, d);
                    if constexpr (GATE) {
                        // (`&`, not `&&`: both compares always, one select, no branch in the loop)
                        const int near = (int)(fabs(x1 - x0[k]) <= r) & (int)(fabs(y1 - y0[k]) <= r);
                        d = near ? d : d | MA_PEN;
                    }
                    d2[k] = min(d2[k], max(d1[k], d));
                    j1[k] = d < d1[k] ? j : j1[k];   // (j rises: the first of equal distances stays)
                    d1[k] = min(d1[k], d);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < MA_Q; ++k) {
        const int64_t qi = (int64_t)blockIdx.x * MA_QB + k * NT + threadIdx.x;
        if (qi >= N0) continue;
        int* p = part + (int64_t)blockIdx.y * 3 * N0 + qi;
        p[0] = d1[k];
        p[(int64_t)N0] = j1[k];
        p[2 * (int64_t)N0] = d2[k];
    }
}

struct MatchPar {
    int max_dist, ratio;
};

template <class TP0, class TP1, class TO>
__global__ __launch_bounds__(NT) void k_match_finish(int N0, int S, const int* __restrict__ part,
                                                     const unsigned char* __restrict__ state0,
                                                     const TP0* __restrict__ pts0, const TP1* __restrict__ pts1,
                                                     MatchPar P, int* __restrict__ idx, int* __restrict__ dist,
                                                     unsigned char* __restrict__ status, TO* __restrict__ disp) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= N0) return;
    int d1 = MA_FAR, d2 = MA_FAR, j1 = -1;
    for (int s = 0; s < S; ++s) {   // (split s holds lower j than split s + 1: `<` keeps the lower j)
        const int* p = part + (int64_t)s * 3 * N0 + i;
        const int e1 = p[0], ej = p[(int64_t)N0], e2 = p[2 * (int64_t)N0];
        d2 = min(min(d2, e2), max(d1, e1));
        j1 = e1 < d1 ? ej : j1;
        d1 = min(d1, e1);
    }
    if (d1 >= MA_PEN) {
        d1 = MA_NONE;
        j1 = -1;
    }
    if (d2 >= MA_PEN) d2 = MA_NONE;
    unsigned st = state0[i];
    if (st) {
        d1 = d2 = MA_NONE;
        j1 = -1;
    } else {
        if (j1 < 0 || d1 > P.max_dist) {
            st |= FOTO_MATCH_NONE;
            j1 = -1;
        }
        if (!(P.ratio == 0 || d1 * 256 < P.ratio * d2)) st |= FOTO_MATCH_AMBIGUOUS;
    }
    idx[i] = j1;
    dist[2 * i] = d1;
    dist[2 * i + 1] = d2;
    status[i] = (unsigned char)st;
    if (disp) {
        double dx = NAN, dy = NAN;
        if (j1 >= 0) {
            dx = (double)pts1[2 * (int64_t)j1] - (double)pts0[2 * i];
            dy = (double)pts1[2 * (int64_t)j1 + 1] - (double)pts0[2 * i + 1];
        }
        disp[2 * i] = (TO)dx;
        disp[2 * i + 1] = (TO)dy;
    }
}

__global__ __launch_bounds__(NT) void k_match_cross(const int* __restrict__ idx01, int N0,
                                                    const int* __restrict__ idx10, int N1, unsigned char* status) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= N0) return;
    const int j = idx01[i];
    if (j < 0) return;
    if (j >= N1 || idx10[j] != (int)i) status[i] = (unsigned char)(status[i] | FOTO_MATCH_NOT_MUTUAL);
}

// ----------------------------------------------------------------------------- per-device state

// One stream, link, grow-only scratch and table pair per device, kept for the process like
// foto_motion.hip's.  The calls only enqueue on the stream.
struct MatchDev {
    hipStream_t s = nullptr;
    StreamLink link;
    DevScratch tmp, table;
    std::vector<int8_t> pattern;   // the host copies of what `table` holds
    std::vector<double> dirs;
};
std::mutex ma_mu;
std::vector<MatchDev*> ma_dev;

int match_dev(int* device, MatchDev** out) {   // (ma_mu held by the caller)
    int dev = 0;
    FOTO_HIP_CHECK(hipGetDevice(&dev));
    if ((int)ma_dev.size() <= dev) ma_dev.resize(dev + 1, nullptr);
    if (!ma_dev[dev]) {
        hipStream_t s = nullptr;
        FOTO_TRY(stream_acquire(&s));
        ma_dev[dev] = new MatchDev();
        ma_dev[dev]->s = s;
    }
    *device = dev;
    *out = ma_dev[dev];
    return 0;
}

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

struct Buf {
    const void* p;
    size_t bytes;
    const char* what;
};

// every buffer is device memory of `device`; no output overlaps an input or another output
int bufs_check(const Buf* in, int n_in, const Buf* out, int n_out, int device, const char* who) {
    for (int i = 0; i < n_in; ++i) FOTO_TRY(dev_ptr_check(in[i].p, in[i].bytes, device, who, in[i].what));
    for (int a = 0; a < n_out; ++a) FOTO_TRY(dev_ptr_check(out[a].p, out[a].bytes, device, who, out[a].what));
    for (int a = 0; a < n_out; ++a) {
        for (int i = 0; i < n_in; ++i)
            if (overlaps(out[a].p, out[a].bytes, in[i].p, in[i].bytes)) {
                set_error("%s: %s may not overlap %s", who, out[a].what, in[i].what);
                return FOTO_ERR_ARG;
            }
        for (int b = a + 1; b < n_out; ++b)
            if (overlaps(out[a].p, out[a].bytes, out[b].p, out[b].bytes)) {
                set_error("%s: %s may not overlap %s", who, out[a].what, out[b].what);
                return FOTO_ERR_ARG;
            }
    }
    return 0;
}

int count_check(int64_t M, const char* who, const char* what) {
    if (M < 1 || M > (int64_t)INT32_MAX) {
        set_error("%s: %s = %lld must be in [1, 2^31 - 1]", who, what, (long long)M);
        return FOTO_ERR_ARG;
    }
    return 0;
}

int aligned_check(const void* p, size_t a, const char* who, const char* what) {
    if ((uintptr_t)p % a != 0) {
        set_error("%s: %s %p is not aligned to %d bytes", who, what, p, (int)a);
        return FOTO_ERR_ARG;
    }
    return 0;
}

template <class TP0, class TP1>
void match_launch(bool gate, dim3 grid, const void* desc0, const void* pts0, int N0, const void* desc1,
                  const unsigned char* state1, const void* pts1, int N1, int chunk, double r, int* part,
                  hipStream_t s) {
    if (gate)
        k_match<true, TP0, TP1><<<grid, NT, 0, s>>>((const uint4*)desc0, (const TP0*)pts0, N0, (const uint4*)desc1,
                                                     state1, (const TP1*)pts1, N1, chunk, r, part);
    else
        k_match<false, TP0, TP1><<<grid, NT, 0, s>>>((const uint4*)desc0, (const TP0*)pts0, N0, (const uint4*)desc1,
                                                      state1, (const TP1*)pts1, N1, chunk, r, part);
}

template <class TP0, class TP1>
void finish_launch(int N0, int S, const int* part, const unsigned char* state0, const void* pts0, const void* pts1,
                   MatchPar P, int* idx, int* dist, unsigned char* status, void* disp, int disp_dtype,
                   hipStream_t s) {
    const unsigned grid = (unsigned)(((int64_t)N0 + NT - 1) / NT);
    if (disp_dtype == FOTO_F32)
        k_match_finish<TP0, TP1, float><<<grid, NT, 0, s>>>(N0, S, part, state0, (const TP0*)pts0, (const TP1*)pts1, P,
                                                             idx, dist, status, (float*)disp);
    else
        k_match_finish<TP0, TP1, double><<<grid, NT, 0, s>>>(N0, S, part, state0, (const TP0*)pts0, (const TP1*)pts1,
                                                              P, idx, dist, status, (double*)disp);
}

}  // namespace
}  // namespace foto

using namespace foto;

extern "C" {

int foto_describe_opts_default(foto_describe_opts* o) {
    if (!o) { set_error("foto_describe_opts_default: null argument"); return FOTO_ERR_ARG; }
    o->blur = 2;
    o->patch = 15;
    o->orientations = 1;
    o->reserved = 0;
    return 0;
}

int foto_match_opts_default(foto_match_opts* o) {
    if (!o) { set_error("foto_match_opts_default: null argument"); return FOTO_ERR_ARG; }
    o->max_disp = 0.0;
    o->max_dist = 64;
    o->ratio = 205;
    o->reserved[0] = o->reserved[1] = 0;
    return 0;
}

int foto_describe_dev(const foto_image* frame, int w, int h, const void* pts, int pts_dtype, int64_t M,
                      const foto_describe_opts* opts, const int8_t* pattern, const double* directions,
                      uint64_t* desc, unsigned char* state, int32_t* bin_or_null, void* stream) {
    static const char* const who = "foto_describe_dev";
    if (!frame || !pts || !pattern || !directions || !desc || !state) {
        set_error("%s: null argument", who);
        return FOTO_ERR_ARG;
    }
    foto_describe_opts o;
    (void)foto_describe_opts_default(&o);
    if (opts) o = *opts;
    if (o.blur < 0 || o.blur > FOTO_MATCH_MAX_BLUR) {
        set_error("%s: blur = %d: the box radius is 0 .. %d", who, o.blur, FOTO_MATCH_MAX_BLUR);
        return FOTO_ERR_ARG;
    }
    if (o.patch < 2 || o.patch > FOTO_MATCH_MAX_PATCH) {
        set_error("%s: patch = %d: the disc's radius is 2 .. %d", who, o.patch, FOTO_MATCH_MAX_PATCH);
        return FOTO_ERR_ARG;
    }
    if (o.orientations < 1 || o.orientations > FOTO_MATCH_MAX_ORIENT) {
        set_error("%s: orientations = %d: 1 .. %d bins", who, o.orientations, FOTO_MATCH_MAX_ORIENT);
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(image_size_check(w, h, 2 * o.patch + 1, who));
    FOTO_TRY(image_check(frame, w, h, who));
    FOTO_TRY(count_check(M, who, "M"));
    FOTO_TRY(track_dtype_check(pts, pts_dtype, who, "pts"));
    FOTO_TRY(aligned_check(desc, 8, who, "desc"));
    FOTO_TRY(aligned_check(bin_or_null, 4, who, "bin"));
    FOTO_TRY(aligned_check(directions, 8, who, "directions"));
    const size_t pn = (size_t)o.orientations * 256 * 4;
    for (size_t e = 0; e < pn; e += 2) {
        const int ax = pattern[e], ay = pattern[e + 1];
        if (ax * ax + ay * ay > o.patch * o.patch) {
            set_error("%s: pattern entry %d of bin %d, (%d, %d), is outside the disc of radius %d", who,
                      (int)(e / 4 % 256), (int)(e / 1024), ax, ay, o.patch);
            return FOTO_ERR_ARG;
        }
    }
    std::lock_guard<std::mutex> lk(ma_mu);
    int device = 0;
    MatchDev* md = nullptr;
    FOTO_TRY(match_dev(&device, &md));
    FOTO_TRY(image_dev_check(frame, w, h, device, who));
    const int64_t n = (int64_t)w * h;
    const Buf in[1] = {{pts, (size_t)M * 2 * dtype_bytes(pts_dtype), "pts"}};
    const Buf outs[3] = {{desc, (size_t)M * 32, "desc"}, {state, (size_t)M, "state"},
                         {bin_or_null, (size_t)M * 4, "bin"}};
    FOTO_TRY(bufs_check(in, 1, outs, bin_or_null ? 3 : 2, device, who));
    hipStream_t s = md->s;
    // the tables: uploaded when they differ from the previous call's
    const size_t dn = (size_t)o.orientations * 2, doff = align_up(pn);
    if (md->pattern.size() != pn || std::memcmp(md->pattern.data(), pattern, pn) != 0 || md->dirs.size() != dn ||
        std::memcmp(md->dirs.data(), directions, dn * sizeof(double)) != 0) {
        FOTO_HIP_CHECK(hipStreamSynchronize(s));   // (an earlier call may still read the old tables)
        FOTO_TRY(md->table.reserve(align_up((size_t)FOTO_MATCH_MAX_ORIENT * 1024) + FOTO_MATCH_MAX_ORIENT * 16, s));
        md->pattern.assign(pattern, pattern + pn);
        md->dirs.assign(directions, directions + dn);
        FOTO_HIP_CHECK(hipMemcpyAsync(md->table.p, md->pattern.data(), pn, hipMemcpyHostToDevice, s));
        FOTO_HIP_CHECK(hipMemcpyAsync((char*)md->table.p + doff, md->dirs.data(), dn * sizeof(double),
                                      hipMemcpyHostToDevice, s));
    }
    FOTO_TRY(md->tmp.reserve((o.blur > 0 ? 3 : 1) * align_up((size_t)n * 8), s));
    double* F = (double*)md->tmp.p;
    double* Hh = (double*)((char*)md->tmp.p + align_up((size_t)n * 8));
    double* B = o.blur > 0 ? (double*)((char*)md->tmp.p + 2 * align_up((size_t)n * 8)) : F;
    const int* dpat = (const int*)md->table.p;
    const double* ddir = (const double*)((const char*)md->table.p + doff);
    const DescPar P{w, h, o.patch, o.orientations};
    FOTO_TRY(md->link.enter((hipStream_t)stream, s));
    auto run = [&]() -> int {
        FOTO_HIP_CHECK(launch_ingest(*frame, w, h, F, s));
        if (o.blur > 0) {
            const unsigned g = (unsigned)((n + NT - 1) / NT);
            k_box_h<<<g, NT, 0, s>>>(w, n, o.blur, F, Hh);
            k_box_v<<<g, NT, 0, s>>>(w, h, n, o.blur, Hh, B);
            FOTO_HIP_CHECK(hipGetLastError());
        }
        const unsigned grid = (unsigned)((M + NT / 64 - 1) / (NT / 64));
        if (pts_dtype == FOTO_F32)
            k_describe<float><<<grid, NT, 0, s>>>(P, F, B, (const float*)pts, M, dpat, ddir, (unsigned long long*)desc,
                                                  state, bin_or_null);
        else
            k_describe<double><<<grid, NT, 0, s>>>(P, F, B, (const double*)pts, M, dpat, ddir,
                                                   (unsigned long long*)desc, state, bin_or_null);
        FOTO_HIP_CHECK(hipGetLastError());
        return 0;
    };
    const int rc = run();
    const int rl = md->link.leave(s, (hipStream_t)stream);
    return rc < 0 ? rc : rl;
}

int foto_match_dev(const uint64_t* desc0, const unsigned char* state0, const void* pts0, int pts0_dtype, int64_t N0,
                   const uint64_t* desc1, const unsigned char* state1, const void* pts1, int pts1_dtype, int64_t N1,
                   const foto_match_opts* opts, int32_t* idx, int32_t* dist, unsigned char* status,
                   void* disp_or_null, int disp_dtype, void* stream) {
    static const char* const who = "foto_match_dev";
    if (!desc0 || !state0 || !pts0 || !desc1 || !state1 || !pts1 || !idx || !dist || !status) {
        set_error("%s: null argument", who);
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(count_check(N0, who, "N0"));
    FOTO_TRY(count_check(N1, who, "N1"));
    foto_match_opts o;
    (void)foto_match_opts_default(&o);
    if (opts) o = *opts;
    if (!std::isfinite(o.max_disp) || o.max_disp < 0) {
        set_error("%s: max_disp = %g must be finite and >= 0", who, o.max_disp);
        return FOTO_ERR_ARG;
    }
    if (o.max_dist < 0 || o.max_dist > 256 || o.ratio < 0 || o.ratio > 256) {
        set_error("%s: max_dist = %d and ratio = %d must be in 0 .. 256", who, o.max_dist, o.ratio);
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(track_dtype_check(pts0, pts0_dtype, who, "pts0"));
    FOTO_TRY(track_dtype_check(pts1, pts1_dtype, who, "pts1"));
    if (disp_or_null) FOTO_TRY(track_dtype_check(disp_or_null, disp_dtype, who, "disp"));
    FOTO_TRY(aligned_check(desc0, 16, who, "desc0"));
    FOTO_TRY(aligned_check(desc1, 16, who, "desc1"));
    FOTO_TRY(aligned_check(idx, 4, who, "idx"));
    FOTO_TRY(aligned_check(dist, 4, who, "dist"));
    std::lock_guard<std::mutex> lk(ma_mu);
    int device = 0;
    MatchDev* md = nullptr;
    FOTO_TRY(match_dev(&device, &md));
    const Buf in[6] = {{desc0, (size_t)N0 * 32, "desc0"}, {state0, (size_t)N0, "state0"},
                       {pts0, (size_t)N0 * 2 * dtype_bytes(pts0_dtype), "pts0"},
                       {desc1, (size_t)N1 * 32, "desc1"}, {state1, (size_t)N1, "state1"},
                       {pts1, (size_t)N1 * 2 * dtype_bytes(pts1_dtype), "pts1"}};
    const Buf outs[4] = {{idx, (size_t)N0 * 4, "idx"}, {dist, (size_t)N0 * 8, "dist"}, {status, (size_t)N0, "status"},
                         {disp_or_null, (size_t)N0 * 2 * dtype_bytes(disp_dtype), "disp"}};
    FOTO_TRY(bufs_check(in, 6, outs, disp_or_null ? 4 : 3, device, who));
    // the shape: query blocks x splits of the train set, about FOTO_MATCH_BLOCKS blocks in all; a
    // split is a whole number of LDS tiles
    const int64_t qb = (N0 + MA_QB - 1) / MA_QB, tiles = (N1 + MA_T - 1) / MA_T;
    const int64_t want = std::min<int64_t>(tiles, std::max<int64_t>(1, FOTO_MATCH_BLOCKS / qb));
    const int64_t per = (tiles + want - 1) / want;   // tiles per split
    const int S = (int)((tiles + per - 1) / per);
    const int chunk = (int)std::min<int64_t>(per * MA_T, (int64_t)INT32_MAX);
    hipStream_t s = md->s;
    FOTO_TRY(md->tmp.reserve((size_t)S * 3 * (size_t)N0 * 4, s));
    int* part = (int*)md->tmp.p;
    const bool gate = o.max_disp != 0.0;
    const dim3 grid((unsigned)qb, (unsigned)S);
    const MatchPar P{o.max_dist, o.ratio};
    FOTO_TRY(md->link.enter((hipStream_t)stream, s));
    const bool a32 = pts0_dtype == FOTO_F32, b32 = pts1_dtype == FOTO_F32;
    if (a32 && b32) {
        match_launch<float, float>(gate, grid, desc0, pts0, (int)N0, desc1, state1, pts1, (int)N1, chunk, o.max_disp, part, s);
        finish_launch<float, float>((int)N0, S, part, state0, pts0, pts1, P, idx, dist, status, disp_or_null, disp_dtype, s);
    } else if (a32) {
        match_launch<float, double>(gate, grid, desc0, pts0, (int)N0, desc1, state1, pts1, (int)N1, chunk, o.max_disp, part, s);
        finish_launch<float, double>((int)N0, S, part, state0, pts0, pts1, P, idx, dist, status, disp_or_null, disp_dtype, s);
    } else if (b32) {
        match_launch<double, float>(gate, grid, desc0, pts0, (int)N0, desc1, state1, pts1, (int)N1, chunk, o.max_disp, part, s);
        finish_launch<double, float>((int)N0, S, part, state0, pts0, pts1, P, idx, dist, status, disp_or_null, disp_dtype, s);
    } else {
        match_launch<double, double>(gate, grid, desc0, pts0, (int)N0, desc1, state1, pts1, (int)N1, chunk, o.max_disp, part, s);
        finish_launch<double, double>((int)N0, S, part, state0, pts0, pts1, P, idx, dist, status, disp_or_null, disp_dtype, s);
    }
    const hipError_t e = hipGetLastError();
    const int rl = md->link.leave(s, (hipStream_t)stream);
    FOTO_HIP_CHECK(e);
    return rl;
}

int foto_match_cross_dev(const int32_t* idx01, int64_t N0, const int32_t* idx10, int64_t N1, unsigned char* status,
                         void* stream) {
    static const char* const who = "foto_match_cross_dev";
    if (!idx01 || !idx10 || !status) { set_error("%s: null argument", who); return FOTO_ERR_ARG; }
    FOTO_TRY(count_check(N0, who, "N0"));
    FOTO_TRY(count_check(N1, who, "N1"));
    FOTO_TRY(aligned_check(idx01, 4, who, "idx01"));
    FOTO_TRY(aligned_check(idx10, 4, who, "idx10"));
    std::lock_guard<std::mutex> lk(ma_mu);
    int device = 0;
    MatchDev* md = nullptr;
    FOTO_TRY(match_dev(&device, &md));
    const Buf in[2] = {{idx01, (size_t)N0 * 4, "idx01"}, {idx10, (size_t)N1 * 4, "idx10"}};
    const Buf outs[1] = {{status, (size_t)N0, "status"}};
    FOTO_TRY(bufs_check(in, 2, outs, 1, device, who));
    hipStream_t s = md->s;
    FOTO_TRY(md->link.enter((hipStream_t)stream, s));
    k_match_cross<<<(unsigned)((N0 + NT - 1) / NT), NT, 0, s>>>(idx01, (int)N0, idx10, (int)N1, status);
    const hipError_t e = hipGetLastError();
    const int rl = md->link.leave(s, (hipStream_t)stream);
    FOTO_HIP_CHECK(e);
    return rl;
}

}  // extern "C"

static_assert(sizeof(foto_describe_opts) == 16, "foto_describe_opts layout");
static_assert(sizeof(foto_match_opts) == 24, "foto_match_opts layout");
