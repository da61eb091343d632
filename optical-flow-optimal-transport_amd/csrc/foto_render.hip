// Rendering (include/foto.h, "rendering"): the last stage of a device pipeline.  A flow buffer as
// foto_bb_flow_dev / foto_bb_flow_path_dev / foto_gn_plan_solve_dev write it -- float32 or
// float64, planar [records][3][h][w] or .flo-interleaved [records][h][w][2] -- becomes images
// without leaving HBM:
//   k_render_warp   the clipped reconstruction of main.py:109-110,142 (utils.apply_opticalflow,
//                   utils.py:186-248) of a strided uint8 / float32 / float64 frame with any number
//                   of channels, all records and channels in one launch;
//   k_render_lum    the 8-bit luminosity map of main.py:146;
//   k_flow_maxrad + k_maxrad_final + k_render_color
//                   the Middlebury colour code of run.sh:104,115 (bin/color_flow.py:23-63) in
//                   float64, the per-record maximum radius by a block reduction and one vector
//                   atomic max per block on the bit pattern of the non-negative double.
//
// The warp arithmetic is k_warp's (foto_eval.hip): both call warp_taps and warp_sum of
// foto_devutil.h, here on flow values widened exactly to double and on (double)pixel / divisor;
// built with -ffp-contract=off like every other unit.  A thread owns one output pixel of one record and loops over the channels: the
// weights and the four clamped taps are computed once per pixel and record.  Flow loads are
// coalesced along x, the source taps are gathers, a wave's stores cover one contiguous span.  (Two
// forms of a packed uint8 store, 4 pixels per thread into 32-bit words, measured slower than this
// one at 640 x 480 x 31: DESIGN.md 3.9.)  A uint8 frame is looked up in a 256-entry table of
// (double)pixel / divisor that each block fills with that same IEEE division (12 float64
// divisions per RGB pixel otherwise).  All index arithmetic is int64_t; the two divisions per
// pixel that split the flat index run in 32 bits when records * h * w fits.  The luminosity, one
// byte per pixel and little else, takes 4 pixels per thread and one 32-bit store when `out` is
// 4-byte aligned.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "foto_devutil.h"
#include "foto_internal.h"

namespace foto {

namespace {

// a / b for 0 <= a, 0 < b; small (uniform): both fit 32 bits, where the division is a fraction
// of the 64-bit one
__device__ __forceinline__ int64_t idiv(int64_t a, int64_t b, bool small) {
    return small ? (int64_t)((unsigned)a / (unsigned)b) : a / b;
}

// np.uint8(255 * x) for x in [0, 1]: truncating (main.py:142,146).  NaN -> 0 (np.uint8(nan) is
// platform-defined).
__device__ __forceinline__ unsigned u8_trunc(double x) { return x == x ? (unsigned)(int)(255.0 * x) : 0u; }

__device__ __forceinline__ double clip01(double x) {   // np.clip(x, 0, 1): NaN stays
    if (x < 0.0) x = 0.0;
    if (x > 1.0) x = 1.0;
    return x;
}

template <class T> __device__ __forceinline__ T out_cast(double x) { return (T)x; }
template <> __device__ __forceinline__ unsigned char out_cast<unsigned char>(double x) {
    return (unsigned char)u8_trunc(x);
}

// The bytes of a thread's 4 pixels in output order (luminosity): four into one 32-bit store.
struct Pack4 {
    unsigned acc = 0;
    int b = 0;
    __device__ __forceinline__ void put(unsigned* __restrict__ o32, unsigned v) {
        acc |= v << (8 * (b & 3));
        if ((b & 3) == 3) {
            o32[b >> 2] = acc;
            acc = 0;
        }
        ++b;
    }
};

// (u, v) of pixel p of one record; LAYOUT 0: planes u, v(, m) of n values; 1: (u, v) pairs
template <class Tf, int LAYOUT>
__device__ __forceinline__ void load_uv(const Tf* __restrict__ rec, int64_t n, int64_t p, double& u, double& v) {
    if (LAYOUT == 0) {
        u = (double)rec[p];
        v = (double)rec[n + p];
    } else {
        u = (double)rec[2 * p];
        v = (double)rec[2 * p + 1];
    }
}

// value = (double)pixel / divisor.  uint8: the block's table of that division for the 256 pixel
// values (NT = 256 threads, one entry each); float32 / float64: the division itself, skipped for
// divisor 1.
template <class Ts> struct SrcValue {
    double divisor;
    bool unit;   // divisor == 1 (the float frames' default): x / 1.0 is x, bit for bit
    __device__ __forceinline__ void init(double d, double*) { divisor = d; unit = d == 1.0; }
    __device__ __forceinline__ double operator()(Ts x) const { return unit ? (double)x : (double)x / divisor; }
};
template <> struct SrcValue<unsigned char> {
    const double* lut;
    __device__ __forceinline__ void init(double d, double* sh) {
        sh[threadIdx.x] = (double)threadIdx.x / d;
        __syncthreads();
        lut = sh;
    }
    __device__ __forceinline__ double operator()(unsigned char x) const { return lut[x]; }
};
static_assert(NT == 256, "the uint8 table has one entry per thread");

// One output pixel's share of the warp that does not depend on the channel: the shared weights
// and clamped taps (warp_taps, foto_devutil.h: k_warp's), the taps as element offsets into a
// channel, and 1 + m at the taps.
struct PixelTaps {
    WarpTaps T;
    int64_t q1, q2, q3, q4;
    double g1, g2, g3, g4;
};

template <class Tf, int LAYOUT>
__device__ __forceinline__ PixelTaps pixel_taps(const Tf* __restrict__ flow, int64_t n, int w, int h, int64_t t,
                                                bool small, int64_t sy, int64_t sx, bool scale) {
    const int64_t k = idiv(t, n, small), p = t - k * n;
    const Tf* __restrict__ rec = flow + k * (LAYOUT == 0 ? 3 : 2) * n;
    double u, v;
    load_uv<Tf, LAYOUT>(rec, n, p, u, v);
    const int64_t row = idiv(p, w, small);
    PixelTaps P;
    P.T = warp_taps((int)row, (int)(p - row * w), u, v, w, h);
    const int64_t a = P.T.a, b = P.T.b, a1 = P.T.a1, b1 = P.T.b1;
    P.q1 = a * sy + b * sx;
    P.q2 = a * sy + b1 * sx;
    P.q3 = a1 * sy + b1 * sx;
    P.q4 = a1 * sy + b * sx;
    P.g1 = P.g2 = P.g3 = P.g4 = 1;
    if (LAYOUT == 0 && scale) {
        const Tf* __restrict__ m = rec + 2 * n;
        P.g1 = 1 + (double)m[a * w + b];
        P.g2 = 1 + (double)m[a * w + b1];
        P.g3 = 1 + (double)m[a1 * w + b1];
        P.g4 = 1 + (double)m[a1 * w + b];
    }
    return P;
}

// out[records][h][w][C] = cast(clip(apply_opticalflow(src_c / divisor, u_k, v_k, w, h, m_k), 0, 1))
template <class Ts, class Tf, class To, int LAYOUT>
__global__ __launch_bounds__(NT) void k_render_warp(const Ts* __restrict__ src, int64_t sy, int64_t sx, int64_t sc,
                                                    double divisor, int C, const Tf* __restrict__ flow, int64_t R,
                                                    int w, int h, int use_m, To* __restrict__ out) {
    __shared__ double sh[sizeof(Ts) == 1 ? NT : 1];
    SrcValue<Ts> val;
    val.init(divisor, sh);
    const int64_t n = (int64_t)w * h, T = R * n;
    const bool small = T <= 0xffffffffLL, scale = LAYOUT == 0 && use_m;
    for (int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x; t < T; t += (int64_t)gridDim.x * NT) {
        const PixelTaps tp = pixel_taps<Tf, LAYOUT>(flow, n, w, h, t, small, sy, sx, scale);
        for (int c = 0; c < C; ++c) {
            const Ts* __restrict__ sp = src + (int64_t)c * sc;
            const double s1 = val(sp[tp.q1]), s2 = val(sp[tp.q2]), s3 = val(sp[tp.q3]), s4 = val(sp[tp.q4]);
            const double x = scale ? warp_sum(tp.T, tp.g1, tp.g2, tp.g3, tp.g4, s1, s2, s3, s4)
                                   : warp_sum(tp.T, s1, s2, s3, s4);
            out[t * C + c] = out_cast<To>(clip01(x));
        }
    }
}

// out[records][h][w] = np.uint8(255 * np.clip((m + 1) / 2, 0, 1)) (main.py:146), NaN -> 0
template <class Tf, int PX>
__global__ __launch_bounds__(NT) void k_render_lum(const Tf* __restrict__ flow, int64_t R, int64_t n,
                                                   unsigned char* __restrict__ out) {
    const int64_t T = R * n, items = (T + PX - 1) / PX;
    const bool small = T <= 0xffffffffLL;
    for (int64_t it = (int64_t)blockIdx.x * NT + threadIdx.x; it < items; it += (int64_t)gridDim.x * NT) {
        const int64_t t0 = it * PX;
        const bool full = PX > 1 && t0 + PX <= T;
        Pack4 pk;
        unsigned* o32 = (unsigned*)(void*)out + (PX > 1 ? it : 0);
#pragma unroll
        for (int px = 0; px < PX; ++px) {
            const int64_t t = t0 + px;
            if (t >= T) break;
            const int64_t k = idiv(t, n, small), p = t - k * n;
            const double m = (double)flow[(k * 3 + 2) * n + p];
            const unsigned y = u8_trunc(clip01((m + 1) / 2));
            if (full) pk.put(o32, y);
            else out[t] = (unsigned char)y;
        }
    }
}

// ----------------------------------------------------------------------------- colour code
// bin/color_flow.py:23-63 (the Middlebury colorcode.cpp / color_flow.cpp) in float64.

constexpr int NCOLS = 55;
// colorwheel() / 255.0 (bin/color_flow.py:23-32, 58-59): the division done once, at compile time
// (IEEE, to nearest: the quotient flow_to_color computes per pixel)
struct Wheel { double c[NCOLS][3]; };
constexpr Wheel make_wheel() {
    Wheel W{};
    const int RY = 15, YG = 6, GC = 4, CB = 11, BM = 13, MR = 6;
    int k = 0;
    for (int i = 0; i < RY; ++i, ++k) { W.c[k][0] = 255; W.c[k][1] = 255 * i / RY; W.c[k][2] = 0; }
    for (int i = 0; i < YG; ++i, ++k) { W.c[k][0] = 255 - 255 * i / YG; W.c[k][1] = 255; W.c[k][2] = 0; }
    for (int i = 0; i < GC; ++i, ++k) { W.c[k][0] = 0; W.c[k][1] = 255; W.c[k][2] = 255 * i / GC; }
    for (int i = 0; i < CB; ++i, ++k) { W.c[k][0] = 0; W.c[k][1] = 255 - 255 * i / CB; W.c[k][2] = 255; }
    for (int i = 0; i < BM; ++i, ++k) { W.c[k][0] = 255 * i / BM; W.c[k][1] = 0; W.c[k][2] = 255; }
    for (int i = 0; i < MR; ++i, ++k) { W.c[k][0] = 255; W.c[k][1] = 0; W.c[k][2] = 255 - 255 * i / MR; }
    for (k = 0; k < NCOLS; ++k)
        for (int b = 0; b < 3; ++b) W.c[k][b] = W.c[k][b] / 255.0;
    return W;
}
__constant__ Wheel WHEEL = make_wheel();

// mr[k] = max over the known pixels of record k = blockIdx.y of sqrt(u u + v v), mr zeroed before
// the launch.  The maximum does not depend on the order, and a non-negative double orders like
// its bit pattern: a block tree, then one 64-bit unsigned atomic max per block.
constexpr int MAXRAD_PER_THREAD = 8;
template <class Tf, int LAYOUT>
__global__ __launch_bounds__(NT) void k_flow_maxrad(const Tf* __restrict__ flow, int64_t n, double* __restrict__ mr) {
    __shared__ double sh[NT];
    const int64_t k = blockIdx.y;
    const Tf* __restrict__ rec = flow + k * (LAYOUT == 0 ? 3 : 2) * n;
    double best = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < n; p += (int64_t)gridDim.x * NT) {
        double u, v;
        load_uv<Tf, LAYOUT>(rec, n, p, u, v);
        const double rad = sqrt(u * u + v * v);
        if (!flow_unknown(u, v) && rad > best) best = rad;
    }
    sh[threadIdx.x] = best;
    __syncthreads();
    for (int st = NT / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st && sh[threadIdx.x + st] > sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0 && sh[0] > 0.0)
        atomicMax((unsigned long long*)(void*)(mr + k), (unsigned long long)__double_as_longlong(sh[0]));
}

// the value actually used: maxmotion > 0 replaces the maximum, a value <= 0 becomes 1
__global__ __launch_bounds__(NT) void k_maxrad_final(int64_t R, double maxmotion, double* __restrict__ mr) {
    const int64_t k = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (k >= R) return;
    double x = maxmotion > 0 ? maxmotion : mr[k];
    if (x <= 0) x = 1.0;
    mr[k] = x;
}

// out[records][h][w][3] = flow_to_color (RGB), float64 in flow_to_color's order of operations; one
// pixel per thread (bound by the float64 arithmetic: packed stores measured no faster)
template <class Tf, int LAYOUT>
__global__ __launch_bounds__(NT) void k_render_color(const Tf* __restrict__ flow, int64_t R, int64_t n,
                                                     const double* __restrict__ mr, unsigned char* __restrict__ out) {
    const int64_t T = R * n;
    const bool small = T <= 0xffffffffLL;
    for (int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x; t < T; t += (int64_t)gridDim.x * NT) {
        const int64_t k = idiv(t, n, small), p = t - k * n;
        double u, v;
        load_uv<Tf, LAYOUT>(flow + k * (LAYOUT == 0 ? 3 : 2) * n, n, p, u, v);
        unsigned rgb[3] = {0, 0, 0};   // unknown flow is black
        if (!flow_unknown(u, v)) {
            const double maxrad = mr[k];
            const double fx = u / maxrad, fy = v / maxrad;
            const double r = sqrt(fx * fx + fy * fy);
            const double a = atan2(-fy, -fx) / M_PI;
            const double fk = (a + 1.0) / 2.0 * (double)(NCOLS - 1);
            int k0 = (int)fk;
            k0 = k0 < 0 ? 0 : k0 > NCOLS - 1 ? NCOLS - 1 : k0;   // (fk is in [0, 54]: the table read stays inside)
            const int k1 = (k0 + 1) % NCOLS;
            const double f = fk - (double)k0;
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const double col0 = WHEEL.c[k0][b], col1 = WHEEL.c[k1][b];
                double col = (1 - f) * col0 + f * col1;
                col = r <= 1 ? 1 - r * (1 - col) : col * 0.75;
                rgb[b] = (unsigned)(int)(255.0 * col) & 0xffu;
            }
        }
#pragma unroll
        for (int b = 0; b < 3; ++b) out[t * 3 + b] = (unsigned char)rgb[b];
    }
}

// ----------------------------------------------------------------------------- host side

}  // namespace

// (foto_internal.h: the scorer, foto_score.hip, reads the same descriptors)
int flow_check(const foto_flow* fl, int w, int h, const char* who) {
    if (!fl) { set_error("%s: null flow descriptor", who); return FOTO_ERR_ARG; }
    if (w < 1 || h < 1) { set_error("%s: w = %d, h = %d: both must be >= 1", who, w, h); return FOTO_ERR_ARG; }
    if (!fl->data) { set_error("%s: flow data is null", who); return FOTO_ERR_ARG; }
    if (fl->dtype != FOTO_F32 && fl->dtype != FOTO_F64) {
        set_error("%s: flow dtype %d is not FOTO_F32 / FOTO_F64", who, fl->dtype);
        return FOTO_ERR_ARG;
    }
    if (fl->layout != 0 && fl->layout != 1) {
        set_error("%s: flow layout %d is not 0 (planar u, v, m) / 1 (interleaved (u, v))", who, fl->layout);
        return FOTO_ERR_ARG;
    }
    if (fl->records < 1) { set_error("%s: flow records = %d must be >= 1", who, fl->records); return FOTO_ERR_ARG; }
    if ((uintptr_t)fl->data % dtype_bytes(fl->dtype) != 0) {
        set_error("%s: flow data %p is not aligned to its %zu-byte element", who, fl->data, dtype_bytes(fl->dtype));
        return FOTO_ERR_ARG;
    }
    return 0;
}

size_t flow_bytes(const foto_flow* fl, int w, int h) {
    return (size_t)fl->records * (fl->layout == 0 ? 3 : 2) * (size_t)w * (size_t)h * dtype_bytes(fl->dtype);
}

namespace {

// One stream, link and maxrad scratch per device, kept for the process like the EvSlots of
// foto_eval.hip.  The calls only enqueue: the stream is never handed back to the pool, so nothing
// waits on the host (but a scratch that has to grow).
struct RenderDev {
    hipStream_t s = nullptr;
    StreamLink link;
    DevScratch mr;   // one double per record
};
std::mutex rd_mu;
std::vector<RenderDev*> rd_dev;

// the current device and its RenderDev (rd_mu held by the caller)
int render_dev(int* device, RenderDev** out) {
    int dev = 0;
    FOTO_HIP_CHECK(hipGetDevice(&dev));
    if ((int)rd_dev.size() <= dev) rd_dev.resize(dev + 1, nullptr);
    if (!rd_dev[dev]) {
        hipStream_t s = nullptr;
        FOTO_TRY(stream_acquire(&s));
        rd_dev[dev] = new RenderDev();
        rd_dev[dev]->s = s;
    }
    *device = dev;
    *out = rd_dev[dev];
    return 0;
}

struct WarpArgs {
    const foto_image* src;
    int C;
    int64_t sc;
    const foto_flow* fl;
    int use_m, w, h;
    void* out;
    int out_dtype;
    hipStream_t s;
};

template <class Ts, class Tf, class To, int LAYOUT>
void warp1_launch(const WarpArgs& a, int64_t T) {
    k_render_warp<Ts, Tf, To, LAYOUT><<<capped_blocks(T, STREAM_MAX_BLOCKS), NT, 0, a.s>>>(
        (const Ts*)a.src->data, a.src->stride_y, a.src->stride_x, a.sc, a.src->divisor, a.C, (const Tf*)a.fl->data,
        a.fl->records, a.w, a.h, a.use_m, (To*)a.out);
}

template <class Ts, class Tf, int LAYOUT>
void warp_launch_l(const WarpArgs& a) {
    const int64_t T = (int64_t)a.fl->records * a.w * a.h;
    switch (a.out_dtype) {
        case FOTO_U8: return warp1_launch<Ts, Tf, unsigned char, LAYOUT>(a, T);
        case FOTO_F32: return warp1_launch<Ts, Tf, float, LAYOUT>(a, T);
        default: return warp1_launch<Ts, Tf, double, LAYOUT>(a, T);
    }
}

template <class Ts>
void warp_launch(const WarpArgs& a) {
    if (a.fl->dtype == FOTO_F32) {
        if (a.fl->layout == 0) warp_launch_l<Ts, float, 0>(a);
        else warp_launch_l<Ts, float, 1>(a);
    } else {
        if (a.fl->layout == 0) warp_launch_l<Ts, double, 0>(a);
        else warp_launch_l<Ts, double, 1>(a);
    }
}

template <class Tf>
void lum_launch(const foto_flow* fl, int64_t n, void* out, hipStream_t s) {
    const int64_t T = (int64_t)fl->records * n;
    const Tf* f = (const Tf*)fl->data;
    unsigned char* o = (unsigned char*)out;
    if ((uintptr_t)out % 4 == 0)
        k_render_lum<Tf, 4><<<capped_blocks((T + 3) / 4, STREAM_MAX_BLOCKS), NT, 0, s>>>(f, fl->records, n, o);
    else
        k_render_lum<Tf, 1><<<capped_blocks(T, STREAM_MAX_BLOCKS), NT, 0, s>>>(f, fl->records, n, o);
}

template <class Tf, int LAYOUT>
void color_launch(const foto_flow* fl, int64_t n, double maxmotion, double* mr, void* out, hipStream_t s) {
    const int64_t R = fl->records, T = R * n;
    if (!(maxmotion > 0)) {
        const int64_t per_block = (int64_t)NT * MAXRAD_PER_THREAD;
        const unsigned bx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per_block - 1) / per_block, 1024));
        for (int64_t k0 = 0; k0 < R; k0 += 65535) {   // (the records of one launch ride on gridDim.y)
            const unsigned by = (unsigned)std::min<int64_t>(R - k0, 65535);
            k_flow_maxrad<Tf, LAYOUT><<<dim3(bx, by), NT, 0, s>>>(
                (const Tf*)fl->data + k0 * (LAYOUT == 0 ? 3 : 2) * n, n, mr + k0);
        }
    }
    k_maxrad_final<<<(unsigned)((R + NT - 1) / NT), NT, 0, s>>>(R, maxmotion, mr);
    k_render_color<Tf, LAYOUT><<<capped_blocks(T, STREAM_MAX_BLOCKS), NT, 0, s>>>((const Tf*)fl->data, R, n, mr,
                                                                                  (unsigned char*)out);
}

}  // namespace
}  // namespace foto

using namespace foto;

extern "C" {

int foto_flow_check(const foto_flow* fl, int w, int h) { return flow_check(fl, w, h, "foto_flow_check"); }

int foto_render_warp_dev(const foto_image* src, int channels, int64_t stride_c, const foto_flow* fl, int use_m, int w,
                         int h, void* out, int out_dtype, void* stream) {
    static const char* const who = "foto_render_warp_dev";
    // ---- host-only checks, before any device call
    if (!src || !fl || !out) { set_error("%s: null pointer", who); return FOTO_ERR_ARG; }
    if (channels < 1) { set_error("%s: channels = %d must be >= 1", who, channels); return FOTO_ERR_ARG; }
    if (stride_c <= 0) {
        set_error("%s: stride_c = %lld must be > 0 (in elements)", who, (long long)stride_c);
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(image_check(src, w, h, who));
    const size_t es = dtype_bytes(src->dtype);
    for (int c = 1; c < channels; ++c) {   // (the alignment and the strides are those of channel 0)
        foto_image ch = *src;
        ch.data = (const char*)src->data + (size_t)c * (size_t)stride_c * es;
        FOTO_TRY(image_check(&ch, w, h, who));
    }
    FOTO_TRY(flow_check(fl, w, h, who));
    if (use_m != 0 && use_m != 1) { set_error("%s: use_m = %d is not 0 / 1", who, use_m); return FOTO_ERR_ARG; }
    if (use_m && fl->layout != 0) {
        set_error("%s: use_m = 1 needs layout 0: the interleaved (u, v) layout carries no m", who);
        return FOTO_ERR_ARG;
    }
    if (out_dtype < FOTO_U8 || out_dtype > FOTO_F64) {
        set_error("%s: out_dtype %d is not FOTO_U8 / FOTO_F32 / FOTO_F64", who, out_dtype);
        return FOTO_ERR_ARG;
    }
    if ((uintptr_t)out % dtype_bytes(out_dtype) != 0) {
        set_error("%s: out %p is not aligned to its %zu-byte element", who, out, dtype_bytes(out_dtype));
        return FOTO_ERR_ARG;
    }
    // ---- the pointer queries, before anything is enqueued
    std::lock_guard<std::mutex> lk(rd_mu);
    int device = 0;
    RenderDev* rd = nullptr;
    FOTO_TRY(render_dev(&device, &rd));
    const size_t last = (size_t)(h - 1) * (size_t)src->stride_y + (size_t)(w - 1) * (size_t)src->stride_x +
                        (size_t)(channels - 1) * (size_t)stride_c;
    const size_t src_bytes = (last + 1) * es, fl_bytes = flow_bytes(fl, w, h);
    const size_t out_bytes = (size_t)fl->records * (size_t)w * (size_t)h * (size_t)channels * dtype_bytes(out_dtype);
    FOTO_TRY(image_dev_check(src, w, h, device, who));
    FOTO_TRY(dev_ptr_check(src->data, src_bytes, device, who, "image data (all channels)"));
    FOTO_TRY(dev_ptr_check(fl->data, fl_bytes, device, who, "flow data"));
    FOTO_TRY(dev_ptr_check(out, out_bytes, device, who, "out"));
    if (overlaps(out, out_bytes, src->data, src_bytes) || overlaps(out, out_bytes, fl->data, fl_bytes)) {
        set_error("%s: out may not overlap the frame or the flow (the warp gathers)", who);
        return FOTO_ERR_ARG;
    }
    // ---- one launch
    FOTO_TRY(rd->link.enter((hipStream_t)stream, rd->s));
    const WarpArgs a{src, channels, stride_c, fl, use_m, w, h, out, out_dtype, rd->s};
    switch (src->dtype) {
        case FOTO_U8: warp_launch<unsigned char>(a); break;
        case FOTO_F32: warp_launch<float>(a); break;
        default: warp_launch<double>(a); break;
    }
    FOTO_HIP_CHECK(hipGetLastError());
    return rd->link.leave(rd->s, (hipStream_t)stream);
}

int foto_render_lum_dev(const foto_flow* fl, int w, int h, void* out, void* stream) {
    static const char* const who = "foto_render_lum_dev";
    if (!fl || !out) { set_error("%s: null pointer", who); return FOTO_ERR_ARG; }
    FOTO_TRY(flow_check(fl, w, h, who));
    if (fl->layout != 0) {
        set_error("%s: needs layout 0: the interleaved (u, v) layout carries no m", who);
        return FOTO_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(rd_mu);
    int device = 0;
    RenderDev* rd = nullptr;
    FOTO_TRY(render_dev(&device, &rd));
    const size_t fl_bytes = flow_bytes(fl, w, h), out_bytes = (size_t)fl->records * (size_t)w * (size_t)h;
    FOTO_TRY(dev_ptr_check(fl->data, fl_bytes, device, who, "flow data"));
    FOTO_TRY(dev_ptr_check(out, out_bytes, device, who, "out"));
    if (overlaps(out, out_bytes, fl->data, fl_bytes)) {
        set_error("%s: out may not overlap the flow", who);
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(rd->link.enter((hipStream_t)stream, rd->s));
    if (fl->dtype == FOTO_F32) lum_launch<float>(fl, (int64_t)w * h, out, rd->s);
    else lum_launch<double>(fl, (int64_t)w * h, out, rd->s);
    FOTO_HIP_CHECK(hipGetLastError());
    return rd->link.leave(rd->s, (hipStream_t)stream);
}

int foto_render_color_dev(const foto_flow* fl, int w, int h, double maxmotion, void* out, double* maxrad_or_null,
                          void* stream) {
    static const char* const who = "foto_render_color_dev";
    if (!fl || !out) { set_error("%s: null pointer", who); return FOTO_ERR_ARG; }
    FOTO_TRY(flow_check(fl, w, h, who));
    if (!std::isfinite(maxmotion)) { set_error("%s: maxmotion %g is not finite", who, maxmotion); return FOTO_ERR_ARG; }
    if ((uintptr_t)maxrad_or_null % sizeof(double) != 0) {
        set_error("%s: maxrad %p is not aligned to 8 bytes", who, (void*)maxrad_or_null);
        return FOTO_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(rd_mu);
    int device = 0;
    RenderDev* rd = nullptr;
    FOTO_TRY(render_dev(&device, &rd));
    const size_t fl_bytes = flow_bytes(fl, w, h), out_bytes = (size_t)fl->records * (size_t)w * (size_t)h * 3;
    const size_t mr_bytes = (size_t)fl->records * sizeof(double);
    FOTO_TRY(dev_ptr_check(fl->data, fl_bytes, device, who, "flow data"));
    FOTO_TRY(dev_ptr_check(out, out_bytes, device, who, "out"));
    if (maxrad_or_null) FOTO_TRY(dev_ptr_check(maxrad_or_null, mr_bytes, device, who, "maxrad"));
    if (overlaps(out, out_bytes, fl->data, fl_bytes) ||
        (maxrad_or_null && (overlaps(maxrad_or_null, mr_bytes, fl->data, fl_bytes) ||
                            overlaps(maxrad_or_null, mr_bytes, out, out_bytes)))) {
        set_error("%s: out and maxrad may not overlap the flow or each other", who);
        return FOTO_ERR_ARG;
    }
    double* mr = maxrad_or_null;
    if (!mr) {
        FOTO_TRY(rd->mr.reserve(mr_bytes, rd->s));
        mr = (double*)rd->mr.p;
    }
    FOTO_TRY(rd->link.enter((hipStream_t)stream, rd->s));
    FOTO_HIP_CHECK(hipMemsetAsync(mr, 0, mr_bytes, rd->s));
    const int64_t n = (int64_t)w * h;
    if (fl->dtype == FOTO_F32) {
        if (fl->layout == 0) color_launch<float, 0>(fl, n, maxmotion, mr, out, rd->s);
        else color_launch<float, 1>(fl, n, maxmotion, mr, out, rd->s);
    } else {
        if (fl->layout == 0) color_launch<double, 0>(fl, n, maxmotion, mr, out, rd->s);
        else color_launch<double, 1>(fl, n, maxmotion, mr, out, rd->s);
    }
    FOTO_HIP_CHECK(hipGetLastError());
    return rd->link.leave(rd->s, (hipStream_t)stream);
}

}  // extern "C"

static_assert(sizeof(foto_flow) == 24, "foto_flow layout");
