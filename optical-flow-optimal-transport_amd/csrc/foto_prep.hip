// Frame preparation (include/foto.h, "frame preparation"): what the reference does to a frame
// before main.py sees it -- utils.openGrayscaleImage's convert('L'), run.sh:18-30's resize,
// bin/create_lum_dataset.py, bin/normalize_image.py, bin/data_diff.py -- on device frames, and the
// way back: a flow buffer resized to the size of the caller's frames.
//   k_gray            PIL's convert('L') of a strided 3 / 4 channel frame;
//   k_resize_h / _v   Pillow's separable Image.resize (Resample.c: precompute_coeffs,
//                     normalize_coeffs_8bpc, ImagingResampleHorizontal/Vertical_8bpc / _32bpc), bit
//                     for bit, from coefficient tables the host code below computes as Pillow does;
//   k_illuminate      the rectangles and discs of bin/create_lum_dataset.py:8-21;
//   k_minmax_*        the minimum and maximum of a frame (order-independent);
//   k_normalize_out   bin/normalize_image.py:20-26 from the fixed-order sums of launch_sum;
//   k_diff_out        bin/data_diff.py:35-39.
//
// The resize.  An output pixel is a dot product of its taps with its own coefficients, in tap
// order: int32 from 2^21 with 22-bit coefficients for uint8, a double from 0 for float32 /
// float64.  The horizontal pass works on tiles of TILE_X outputs by H_ROWS rows of one channel; the
// taps of neighbouring outputs overlap almost completely, so a block stages the input span of its
// tile in LDS (one coalesced read) and every thread takes its taps from there.  The spans of a
// tile grow with the reduction ratio; where the widest one exceeds SPAN_CAP elements the launch
// reads its taps from global memory instead (the same arithmetic, the same bits).  Its coefficient
// table is stored transposed, [tap][output], so that a wave's loads are contiguous.  The vertical
// pass reads whole rows, coalesced along x, with coefficients that are uniform over a wave.
// Between the passes the image lives in the input dtype (PIL's 'L' / 'F' intermediate), planar,
// in a grow-only scratch of the plan.  Built with -ffp-contract=off like every other unit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "foto_devmem.h"
#include "foto_internal.h"

namespace foto {

namespace {

constexpr int TILE_X = FOTO_PREP_TILE_X;   // outputs of a horizontal tile: one wave
constexpr int H_ROWS = NT / TILE_X;        // rows of a horizontal tile: one per wave
constexpr int SPAN_CAP = 512;              // elements of one staged row: 4 rows of doubles are 16 KiB
constexpr int PRECISION_BITS = 22;         // Resample.c: 32 - 8 - 2
static_assert(TILE_X == 64 && H_ROWS * TILE_X == NT, "one wave per tile row");

// np.uint8(255 * np.clip(x, 0, 1)): truncating; NaN -> 0 (foto_render_warp_dev's rule)
template <class T> __device__ __forceinline__ T prep_cast(double x) { return (T)x; }
template <> __device__ __forceinline__ unsigned char prep_cast<unsigned char>(double x) {
    if (x < 0.0) x = 0.0;
    if (x > 1.0) x = 1.0;
    return x == x ? (unsigned char)(int)(255.0 * x) : (unsigned char)0;
}

// ----------------------------------------------------------------------------- grey

template <class T> __device__ __forceinline__ T gray_value(T r, T g, T b) {
    const double x = ((19595.0 / 65536.0) * (double)r + (38470.0 / 65536.0) * (double)g) + (7471.0 / 65536.0) * (double)b;
    return (T)x;
}
template <> __device__ __forceinline__ unsigned char gray_value<unsigned char>(unsigned char r, unsigned char g,
                                                                              unsigned char b) {
    return (unsigned char)((19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16);
}

template <class T>
__global__ __launch_bounds__(NT) void k_gray(const T* __restrict__ src, int64_t sy, int64_t sx, int64_t sc, int w,
                                             int64_t n, T* __restrict__ out) {
    for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < n; p += (int64_t)gridDim.x * NT) {
        const int64_t row = (int64_t)((unsigned)p / (unsigned)w), col = p - row * w;   // (n < 2^31)
        const T* __restrict__ q = src + row * sy + col * sx;
        out[p] = gray_value<T>(q[0], q[sc], q[2 * sc]);
    }
}

// ----------------------------------------------------------------------------- resize

// element (plane p, channel c, row y, column x) of an image is at p sp + c sc + y sy + x sx
struct View {
    int64_t sp, sc, sy, sx;
};
// the factor of (plane, channel): s[(p C + c) % mod]; frames: mod = 1, s = {1}
struct Scales {
    double s[3];
    int mod;
};

template <class T> struct Acc {   // float32 / float64: a double from zero, coefficients double
    typedef double K;
    double a = 0.0;
    __device__ __forceinline__ void tap(T x, double k) { a += (double)x * k; }
    __device__ __forceinline__ T done(double scale) const { return (T)(a * scale); }
};
template <> struct Acc<unsigned char> {   // uint8: int32 from 2^21, coefficients 22-bit fixed point
    typedef int K;
    int a = 1 << (PRECISION_BITS - 1);
    __device__ __forceinline__ void tap(unsigned char x, int k) { a += (int)x * k; }
    __device__ __forceinline__ unsigned char done(double) const {
        const int v = a >> PRECISION_BITS;
        return (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : v);
    }
};

// Horizontal pass: block = (tile of TILE_X outputs) x (H_ROWS rows) of one (plane, channel);
// blockIdx.x = (pc * row_groups + rg) * tiles + tile.  kT: [ksize][n_out].
template <class T, bool LDS>
__global__ __launch_bounds__(NT) void k_resize_h(const T* __restrict__ src, View sv, T* __restrict__ dst, View dv,
                                                 int C, int rows, int n_out, int tiles, int row_groups,
                                                 const int2* __restrict__ bounds,
                                                 const typename Acc<T>::K* __restrict__ kT, Scales sa) {
    __shared__ T sh[LDS ? H_ROWS : 1][LDS ? SPAN_CAP : 1];
    const int tx = threadIdx.x & (TILE_X - 1), ty = threadIdx.x / TILE_X;
    const int64_t b = blockIdx.x;
    const int tile = (int)(b % tiles);
    const int64_t br = b / tiles;
    const int rg = (int)(br % row_groups);
    const int64_t pc = br / row_groups;
    const int64_t p = pc / C;
    const int c = (int)(pc - p * C);
    const int row = rg * H_ROWS + ty, x0 = tile * TILE_X, xx = x0 + tx;
    const T* __restrict__ srow = src + p * sv.sp + c * sv.sc + (int64_t)row * sv.sy;
    int s0 = 0;
    if (LDS) {
        const int xl = min(x0 + TILE_X - 1, n_out - 1);
        const int2 bl = bounds[xl];
        s0 = bounds[x0].x;
        const int span = min(bl.x + bl.y - s0, SPAN_CAP);   // (the host checked it: never clipped)
        if (row < rows)
            for (int i = tx; i < span; i += TILE_X) sh[ty][i] = srow[(int64_t)(s0 + i) * sv.sx];
        __syncthreads();
    }
    if (row >= rows || xx >= n_out) return;
    const int2 bx = bounds[xx];
    Acc<T> acc;
    for (int t = 0; t < bx.y; ++t) {
        const T v = LDS ? sh[ty][bx.x - s0 + t] : srow[(int64_t)(bx.x + t) * sv.sx];
        acc.tap(v, kT[(int64_t)t * n_out + xx]);
    }
    dst[p * dv.sp + c * dv.sc + (int64_t)row * dv.sy + (int64_t)xx * dv.sx] = acc.done(sa.s[(int)((p * C + c) % sa.mod)]);
}

// Vertical pass: one thread per output element, x fastest.  k: [n_out][ksize].
template <class T>
__global__ __launch_bounds__(NT) void k_resize_v(const T* __restrict__ src, View sv, T* __restrict__ dst, View dv,
                                                 int C, int width, int n_out, int ksize, int64_t total,
                                                 const int2* __restrict__ bounds,
                                                 const typename Acc<T>::K* __restrict__ k, Scales sa) {
    for (int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x; t < total; t += (int64_t)gridDim.x * NT) {
        const int64_t r = t / width, pc = r / n_out;
        const int x = (int)(t - r * width), yy = (int)(r - pc * n_out);
        const int64_t p = pc / C;
        const int c = (int)(pc - p * C);
        const int2 by = bounds[yy];
        const T* __restrict__ col = src + p * sv.sp + c * sv.sc + (int64_t)x * sv.sx;
        const typename Acc<T>::K* __restrict__ kr = k + (int64_t)yy * ksize;
        Acc<T> acc;
        for (int j = 0; j < by.y; ++j) acc.tap(col[(int64_t)(by.x + j) * sv.sy], kr[j]);
        dst[p * dv.sp + c * dv.sc + (int64_t)yy * dv.sy + (int64_t)x * dv.sx] = acc.done(sa.s[(int)((p * C + c) % sa.mod)]);
    }
}

// equal sizes: the input's bits
template <class T>
__global__ __launch_bounds__(NT) void k_resize_copy(const T* __restrict__ src, View sv, T* __restrict__ dst, View dv,
                                                    int C, int w, int h, int64_t total) {
    for (int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x; t < total; t += (int64_t)gridDim.x * NT) {
        const int64_t r = t / w, pc = r / h;
        const int x = (int)(t - r * w), y = (int)(r - pc * h);
        const int64_t p = pc / C;
        const int c = (int)(pc - p * C);
        dst[p * dv.sp + c * dv.sc + (int64_t)y * dv.sy + (int64_t)x * dv.sx] =
            src[p * sv.sp + c * sv.sc + (int64_t)y * sv.sy + (int64_t)x * sv.sx];
    }
}

// ----------------------------------------------------------------------------- illumination

struct LumArgs {
    int n;
    int kind[FOTO_PREP_MAX_SHAPES];                       // 0 rectangle, 1 disc
    int x0[FOTO_PREP_MAX_SHAPES], x1[FOTO_PREP_MAX_SHAPES], y0[FOTO_PREP_MAX_SHAPES], y1[FOTO_PREP_MAX_SHAPES];
    double R[FOTO_PREP_MAX_SHAPES], cx[FOTO_PREP_MAX_SHAPES], cy[FOTO_PREP_MAX_SHAPES], v[FOTO_PREP_MAX_SHAPES];
};

template <class Ts, class To>
__global__ __launch_bounds__(NT) void k_illuminate(const Ts* __restrict__ src, int64_t sy, int64_t sx, double divisor,
                                                   int w, int64_t n, LumArgs L, To* __restrict__ out) {
    for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < n; p += (int64_t)gridDim.x * NT) {
        const int j = (int)((unsigned)p / (unsigned)w), i = (int)(p - (int64_t)j * w);
        double x = (double)src[(int64_t)j * sy + (int64_t)i * sx] / divisor;
        for (int k = 0; k < L.n; ++k) {
            bool in;
            if (L.kind[k] == 0) {
                in = i >= L.x0[k] && i < L.x1[k] && j >= L.y0[k] && j < L.y1[k];
            } else {
                const double dx = (double)i - L.cx[k], dy = (double)j - L.cy[k];
                in = dx * dx + dy * dy < L.R[k] * L.R[k];
            }
            if (in) x += L.v[k];
        }
        out[p] = prep_cast<To>(x);
    }
}

// ----------------------------------------------------------------------------- min / max, normalise, diff

// The minimum and maximum do not depend on the order; a NaN never wins a comparison.
__device__ __forceinline__ void block_minmax(double& mn, double& mx, double* sh /* 2 * NT / 64 */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double a = __shfl_down(mn, o, 64), b = __shfl_down(mx, o, 64);
        if (a < mn) mn = a;
        if (b > mx) mx = b;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { sh[wv] = mn; sh[NT / 64 + wv] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int j = 1; j < NT / 64; ++j) {
            if (sh[j] < mn) mn = sh[j];
            if (sh[NT / 64 + j] > mx) mx = sh[NT / 64 + j];
        }
    }
}

// part[b] = min, part[nb + b] = max of block b's share of x; with `sub`, x <- x - sub first (in place)
__global__ __launch_bounds__(NT) void k_minmax_partial(int64_t n, const double* __restrict__ sub, double* __restrict__ x,
                                                       double* __restrict__ part) {
    __shared__ double sh[2 * NT / 64];
    double mn = INFINITY, mx = -INFINITY;
    for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < n; p += (int64_t)gridDim.x * NT) {
        double v = x[p];
        if (sub) {
            v = v - sub[p];
            x[p] = v;
        }
        if (v < mn) mn = v;
        if (v > mx) mx = v;
    }
    block_minmax(mn, mx, sh);
    if (threadIdx.x == 0) { part[blockIdx.x] = mn; part[gridDim.x + blockIdx.x] = mx; }
}

__global__ __launch_bounds__(NT) void k_minmax_final(int nb, const double* __restrict__ part, double* __restrict__ out2) {
    __shared__ double sh[2 * NT / 64];
    double mn = INFINITY, mx = -INFINITY;
    for (int b = threadIdx.x; b < nb; b += NT) {
        if (part[b] < mn) mn = part[b];
        if (part[nb + b] > mx) mx = part[nb + b];
    }
    block_minmax(mn, mx, sh);
    if (threadIdx.x == 0) { out2[0] = mn; out2[1] = mx; }
}

// scal = {S0, S1, min0, max0, min1, max1}; out_k = (v_k / S_k) / max(max0 / S0, max1 / S1)
template <class To>
__global__ __launch_bounds__(NT) void k_normalize_out(int64_t n, const double* __restrict__ v0,
                                                      const double* __restrict__ v1, const double* __restrict__ scal,
                                                      To* __restrict__ out0, To* __restrict__ out1) {
    const double S0 = scal[0], S1 = scal[1];
    const double a = scal[3] / S0, b = scal[5] / S1;
    const double scale = a > b ? a : b;   // Python's max(a, b): b unless a > b
    for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < n; p += (int64_t)gridDim.x * NT) {
        out0[p] = prep_cast<To>((v0[p] / S0) / scale);
        out1[p] = prep_cast<To>((v1[p] / S1) / scale);
    }
}

// mm = {min, max} of d; out = (d - min) / (max - min)
template <class To>
__global__ __launch_bounds__(NT) void k_diff_out(int64_t n, const double* __restrict__ d, const double* __restrict__ mm,
                                                 To* __restrict__ out) {
    const double mn = mm[0], den = mm[1] - mm[0];
    for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < n; p += (int64_t)gridDim.x * NT)
        out[p] = prep_cast<To>((d[p] - mn) / den);
}

// ----------------------------------------------------------------------------- Pillow's coefficients (host)

double filter_value(int filter, double x) {
    switch (filter) {
        case FOTO_FILTER_BOX: return x > -0.5 && x <= 0.5 ? 1.0 : 0.0;
        case FOTO_FILTER_BILINEAR:
            if (x < 0.0) x = -x;
            return x < 1.0 ? 1.0 - x : 0.0;
        case FOTO_FILTER_BICUBIC: {
            const double a = -0.5;
            if (x < 0.0) x = -x;
            if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
            if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
            return 0.0;
        }
        default: {   // Lanczos: the truncated sinc
            if (!(-3.0 <= x && x < 3.0)) return 0.0;
            auto sinc = [](double t) {
                if (t == 0.0) return 1.0;
                t = t * M_PI;
                return std::sin(t) / t;
            };
            return sinc(x) * sinc(x / 3);
        }
    }
}

constexpr double FILTER_SUPPORT[4] = {0.5, 1.0, 2.0, 3.0};

struct AxisTable {
    int n_in = 0, n_out = 0, ksize = 0;
    std::vector<int> bounds;   // [n_out][2] = first tap, count
    std::vector<double> kk;    // [n_out][ksize]
    std::vector<int> kki;      // the same in 22-bit fixed point
};

// Resample.c precompute_coeffs (in0 = 0, in1 = inSize) and normalize_coeffs_8bpc
void axis_table(int n_in, int n_out, int filter, AxisTable* T) {
    const float in0 = 0.0f, in1 = (float)n_in;
    double filterscale, scale;
    filterscale = scale = (double)(in1 - in0) / n_out;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = FILTER_SUPPORT[filter] * filterscale;
    const int ksize = (int)std::ceil(support) * 2 + 1;
    T->n_in = n_in;
    T->n_out = n_out;
    T->ksize = ksize;
    T->bounds.assign((size_t)n_out * 2, 0);
    T->kk.assign((size_t)n_out * ksize, 0.0);
    T->kki.assign((size_t)n_out * ksize, 0);
    for (int xx = 0; xx < n_out; ++xx) {
        const double center = in0 + (xx + 0.5) * scale;
        double ww = 0.0;
        const double ss = 1.0 / filterscale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > n_in) xmax = n_in;
        xmax -= xmin;
        double* k = &T->kk[(size_t)xx * ksize];
        for (int x = 0; x < xmax; ++x) {
            const double w = filter_value(filter, (x + xmin - center + 0.5) * ss);
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < xmax; ++x)
            if (ww != 0.0) k[x] /= ww;
        T->bounds[(size_t)xx * 2] = xmin;
        T->bounds[(size_t)xx * 2 + 1] = xmax;
    }
    for (size_t i = 0; i < T->kk.size(); ++i)
        T->kki[i] = T->kk[i] < 0 ? (int)(-0.5 + T->kk[i] * (1 << PRECISION_BITS))
                                 : (int)(0.5 + T->kk[i] * (1 << PRECISION_BITS));
}

// the widest input span of a tile of TILE_X outputs
int max_tile_span(const AxisTable& T) {
    int best = 0;
    for (int x0 = 0; x0 < T.n_out; x0 += TILE_X) {
        const int xl = std::min(x0 + TILE_X - 1, T.n_out - 1);
        best = std::max(best, T.bounds[(size_t)xl * 2] + T.bounds[(size_t)xl * 2 + 1] - T.bounds[(size_t)x0 * 2]);
    }
    return best;
}

// n_out * ksize of one axis, in double (axis_table's int arithmetic would overflow first), against
// FOTO_RESIZE_MAX_TABLE: the tables live on the host and the device
int axis_table_check(int n_in, int n_out, int filter, const char* who) {
    const double fs = std::max(1.0, (double)n_in / n_out);
    const double entries = (double)n_out * (std::ceil(FILTER_SUPPORT[filter] * fs) * 2 + 1);
    if (entries > (double)FOTO_RESIZE_MAX_TABLE) {
        set_error("%s: %d -> %d needs a table of %.0f coefficients; at most %d (FOTO_RESIZE_MAX_TABLE)", who, n_in, n_out,
                  entries, FOTO_RESIZE_MAX_TABLE);
        return FOTO_ERR_ARG;
    }
    return 0;
}

int size_pair_check(int w, int h, int ow, int oh, int filter, const char* who) {
    FOTO_TRY(image_size_check(w, h, 1, who));
    FOTO_TRY(image_size_check(ow, oh, 1, who));
    if (filter < FOTO_FILTER_BOX || filter > FOTO_FILTER_LANCZOS) {
        set_error("%s: filter %d is not FOTO_FILTER_BOX / BILINEAR / BICUBIC / LANCZOS (0..3)", who, filter);
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(axis_table_check(w, ow, filter, who));
    FOTO_TRY(axis_table_check(h, oh, filter, who));
    return 0;
}

// ----------------------------------------------------------------------------- per-device state

// One stream and link per device for the entries without a plan, kept for the process like
// foto_render.hip's.  The pointwise entries only enqueue on it.
struct PrepDev {
    hipStream_t s = nullptr;
    StreamLink link;
};
std::mutex pd_mu;
std::vector<PrepDev*> pd_dev;

int prep_dev(int* device, PrepDev** out) {   // (pd_mu held by the caller)
    int dev = 0;
    FOTO_HIP_CHECK(hipGetDevice(&dev));
    if ((int)pd_dev.size() <= dev) pd_dev.resize(dev + 1, nullptr);
    if (!pd_dev[dev]) {
        hipStream_t s = nullptr;
        FOTO_TRY(stream_acquire(&s));
        pd_dev[dev] = new PrepDev();
        pd_dev[dev]->s = s;
    }
    *device = dev;
    *out = pd_dev[dev];
    return 0;
}

int out_check(const void* out, int out_dtype, const char* who, const char* what) {
    if (!out) { set_error("%s: %s is null", who, what); return FOTO_ERR_ARG; }
    if (out_dtype < FOTO_U8 || out_dtype > FOTO_F64) {
        set_error("%s: out_dtype %d is not FOTO_U8 / FOTO_F32 / FOTO_F64", who, out_dtype);
        return FOTO_ERR_ARG;
    }
    if ((uintptr_t)out % dtype_bytes(out_dtype) != 0) {
        set_error("%s: %s %p is not aligned to its %zu-byte element", who, what, out, dtype_bytes(out_dtype));
        return FOTO_ERR_ARG;
    }
    return 0;
}

size_t image_bytes(const foto_image* im, int w, int h, int channels = 1, int64_t stride_c = 0) {
    const size_t last = (size_t)(h - 1) * (size_t)im->stride_y + (size_t)(w - 1) * (size_t)im->stride_x +
                        (size_t)(channels - 1) * (size_t)stride_c;
    return (last + 1) * dtype_bytes(im->dtype);
}

// The end of a call that has entered its link: `own` is handed back to `user` whether or not the
// launches in between succeeded, so what was enqueued before a failure is still ordered before the
// caller's next work.  rc: the launches' result, returned unless it was fine and the hand-back failed.
int leave_with(StreamLink& link, hipStream_t own, void* user, int rc) {
    const int rl = link.leave(own, (hipStream_t)user);
    return rc < 0 ? rc : rl;
}

int last_launch() {
    FOTO_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace
}  // namespace foto

using namespace foto;

// ----------------------------------------------------------------------------- the resize plan

struct foto_resize_plan {
    int w = 0, h = 0, ow = 0, oh = 0, filter = 0, device = 0;
    AxisTable X, Y;
    int span_x = 0;            // the widest tile span of the horizontal pass
    hipStream_t s = nullptr;
    StreamLink link;
    DevArena mem;              // the tables, uploaded once
    DevScratch tmp;            // the image between the passes, grow-only
    int2 *bx = nullptr, *by = nullptr;
    double *kxT = nullptr, *ky = nullptr;   // horizontal: [ksize][ow]; vertical: [oh][ksize]
    int *kxTi = nullptr, *kyi = nullptr;
    std::mutex mu;
    ~foto_resize_plan() {
        if (s) {
            (void)hipStreamSynchronize(s);
            stream_release(s);
        }
        if (tmp.p) (void)hipFree(tmp.p);
    }
};

namespace foto {
namespace {

template <class T> const typename Acc<T>::K* table_h(const foto_resize_plan* p);
template <> const double* table_h<float>(const foto_resize_plan* p) { return p->kxT; }
template <> const double* table_h<double>(const foto_resize_plan* p) { return p->kxT; }
template <> const int* table_h<unsigned char>(const foto_resize_plan* p) { return p->kxTi; }
template <class T> const typename Acc<T>::K* table_v(const foto_resize_plan* p);
template <> const double* table_v<float>(const foto_resize_plan* p) { return p->ky; }
template <> const double* table_v<double>(const foto_resize_plan* p) { return p->ky; }
template <> const int* table_v<unsigned char>(const foto_resize_plan* p) { return p->kyi; }

// P planes of C channels through the plan: horizontal, then vertical; a pass whose size does not
// change is skipped; the scales apply in the last pass that runs.  use_lds: the horizontal route.
template <class T>
int resize_run(foto_resize_plan* p, const void* src, View sv, void* dst, View dv, int64_t P, int C, Scales sa,
               bool use_lds) {
    static const char* const who = "foto_resize_dev";
    const bool need_h = p->ow != p->w, need_v = p->oh != p->h;
    const int64_t PC = P * C;
    Scales one;
    one.s[0] = one.s[1] = one.s[2] = 1.0;
    one.mod = 1;
    if (!need_h && !need_v) {
        const int64_t total = PC * p->h * p->w;
        k_resize_copy<T><<<capped_blocks(total, STREAM_MAX_BLOCKS), NT, 0, p->s>>>((const T*)src, sv, (T*)dst, dv, C,
                                                                                  p->w, p->h, total);
        FOTO_HIP_CHECK(hipGetLastError());
        return 0;
    }
    const View iv{(int64_t)C * p->h * p->ow, (int64_t)p->h * p->ow, p->ow, 1};   // between the passes: planar
    const T* vsrc = (const T*)src;
    View vsv = sv;
    if (need_h) {
        T* hdst = (T*)dst;
        View hdv = dv;
        if (need_v) {
            FOTO_TRY(p->tmp.reserve((size_t)PC * p->h * p->ow * sizeof(T), p->s));
            hdst = (T*)p->tmp.p;
            hdv = iv;
        }
        const int tiles = (p->ow + TILE_X - 1) / TILE_X, row_groups = (p->h + H_ROWS - 1) / H_ROWS;
        const int64_t nb = PC * row_groups * tiles;
        if (nb > (int64_t)INT32_MAX) {
            set_error("%s: %lld horizontal tiles exceed one launch", who, (long long)nb);
            return FOTO_ERR_ARG;
        }
        const Scales& hs = need_v ? one : sa;
        if (use_lds)
            k_resize_h<T, true><<<(unsigned)nb, NT, 0, p->s>>>((const T*)src, sv, hdst, hdv, C, p->h, p->ow, tiles,
                                                              row_groups, p->bx, table_h<T>(p), hs);
        else
            k_resize_h<T, false><<<(unsigned)nb, NT, 0, p->s>>>((const T*)src, sv, hdst, hdv, C, p->h, p->ow, tiles,
                                                               row_groups, p->bx, table_h<T>(p), hs);
        FOTO_HIP_CHECK(hipGetLastError());
        vsrc = hdst;
        vsv = hdv;
    }
    if (need_v) {
        const int64_t total = PC * p->oh * p->ow;
        k_resize_v<T><<<capped_blocks(total, STREAM_MAX_BLOCKS), NT, 0, p->s>>>(vsrc, vsv, (T*)dst, dv, C, p->ow, p->oh,
                                                                               p->Y.ksize, total, p->by, table_v<T>(p),
                                                                               sa);
        FOTO_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

int resize_dispatch(foto_resize_plan* p, int dtype, const void* src, View sv, void* dst, View dv, int64_t P, int C,
                    Scales sa, bool use_lds) {
    switch (dtype) {
        case FOTO_U8: return resize_run<unsigned char>(p, src, sv, dst, dv, P, C, sa, use_lds);
        case FOTO_F32: return resize_run<float>(p, src, sv, dst, dv, P, C, sa, use_lds);
        default: return resize_run<double>(p, src, sv, dst, dv, P, C, sa, use_lds);
    }
}

// route -> the horizontal pass stages in LDS (1) or not (0); FOTO_ERR_ARG for a forced LDS route
// whose widest span does not fit
int route_pick(const foto_resize_plan* p, int route, const char* who, bool* use_lds) {
    if (route < FOTO_RESIZE_ROUTE_AUTO || route > FOTO_RESIZE_ROUTE_DIRECT) {
        set_error("%s: route %d is not FOTO_RESIZE_ROUTE_AUTO / LDS / DIRECT (0..2)", who, route);
        return FOTO_ERR_ARG;
    }
    const bool fits = p->span_x <= SPAN_CAP;
    if (route == FOTO_RESIZE_ROUTE_LDS && !fits) {
        set_error("%s: FOTO_RESIZE_ROUTE_LDS: a tile of %d outputs spans %d inputs, the staging holds %d", who, TILE_X,
                  p->span_x, SPAN_CAP);
        return FOTO_ERR_ARG;
    }
    *use_lds = route == FOTO_RESIZE_ROUTE_DIRECT ? false : fits;
    return 0;
}

template <class T>
int upload(foto_resize_plan* p, const std::vector<T>& h, T** out) {
    FOTO_TRY(p->mem.alloc_n(h.size(), out));
    FOTO_HIP_CHECK(hipMemcpyAsync(*out, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, p->s));
    return 0;
}

template <class T>
std::vector<T> transposed(const std::vector<T>& k, int n_out, int ksize) {
    std::vector<T> t(k.size());
    for (int x = 0; x < n_out; ++x)
        for (int j = 0; j < ksize; ++j) t[(size_t)j * n_out + x] = k[(size_t)x * ksize + j];
    return t;
}

int plan_upload(foto_resize_plan* p) {
    const std::vector<double> kxT = transposed(p->X.kk, p->ow, p->X.ksize);
    const std::vector<int> kxTi = transposed(p->X.kki, p->ow, p->X.ksize);
    FOTO_TRY(upload(p, p->X.bounds, (int**)&p->bx));
    FOTO_TRY(upload(p, p->Y.bounds, (int**)&p->by));
    FOTO_TRY(upload(p, kxT, &p->kxT));
    FOTO_TRY(upload(p, kxTi, &p->kxTi));
    FOTO_TRY(upload(p, p->Y.kk, &p->ky));
    FOTO_TRY(upload(p, p->Y.kki, &p->kyi));
    FOTO_HIP_CHECK(hipStreamSynchronize(p->s));   // (the host vectors above go out of scope)
    return 0;
}

template <class T>
void gray_launch(const foto_image* src, int64_t sc, int w, int h, void* out, hipStream_t s) {
    const int64_t n = (int64_t)w * h;
    k_gray<T><<<capped_blocks(n, STREAM_MAX_BLOCKS), NT, 0, s>>>((const T*)src->data, src->stride_y, src->stride_x, sc,
                                                                 w, n, (T*)out);
}

template <class Ts>
void illuminate_launch(const foto_image* src, int w, int h, const LumArgs& L, void* out, int out_dtype, hipStream_t s) {
    const int64_t n = (int64_t)w * h;
    const int nb = capped_blocks(n, STREAM_MAX_BLOCKS);
    const Ts* q = (const Ts*)src->data;
    switch (out_dtype) {
        case FOTO_U8:
            k_illuminate<Ts, unsigned char><<<nb, NT, 0, s>>>(q, src->stride_y, src->stride_x, src->divisor, w, n, L,
                                                              (unsigned char*)out);
            break;
        case FOTO_F32:
            k_illuminate<Ts, float><<<nb, NT, 0, s>>>(q, src->stride_y, src->stride_x, src->divisor, w, n, L, (float*)out);
            break;
        default:
            k_illuminate<Ts, double><<<nb, NT, 0, s>>>(q, src->stride_y, src->stride_x, src->divisor, w, n, L,
                                                       (double*)out);
            break;
    }
}

// int(x) of a shape bound: finite and well inside int
int shape_int(double x, const char* who, int k, int* out) {
    if (!(std::fabs(x) < 1e9)) {
        set_error("%s: shape %d: bound %g is not finite or beyond 1e9", who, k, x);
        return FOTO_ERR_ARG;
    }
    *out = (int)x;
    return 0;
}

int lum_args(const foto_lum_shape* shapes, int count, int w, int h, const char* who, LumArgs* L) {
    if (count < 0 || count > FOTO_PREP_MAX_SHAPES) {
        set_error("%s: %d shapes; 0..%d are allowed", who, count, FOTO_PREP_MAX_SHAPES);
        return FOTO_ERR_ARG;
    }
    if (count > 0 && !shapes) { set_error("%s: shapes is null", who); return FOTO_ERR_ARG; }
    memset(L, 0, sizeof(*L));
    L->n = count;
    for (int k = 0; k < count; ++k) {
        const foto_lum_shape& s = shapes[k];
        if (s.kind != FOTO_LUM_RECT && s.kind != FOTO_LUM_CIRCLE) {
            set_error("%s: shape %d: kind %d is not FOTO_LUM_RECT / FOTO_LUM_CIRCLE", who, k, s.kind);
            return FOTO_ERR_ARG;
        }
        if (!std::isfinite(s.v)) { set_error("%s: shape %d: value %g is not finite", who, k, s.v); return FOTO_ERR_ARG; }
        L->kind[k] = s.kind;
        L->v[k] = s.v;
        if (s.kind == FOTO_LUM_RECT) {   // p = L_x, L_y, r_x, r_y: range(int(r - L / 2), int(r + L / 2))
            FOTO_TRY(shape_int(s.p[2] - s.p[0] / 2, who, k, &L->x0[k]));
            FOTO_TRY(shape_int(s.p[2] + s.p[0] / 2, who, k, &L->x1[k]));
            FOTO_TRY(shape_int(s.p[3] - s.p[1] / 2, who, k, &L->y0[k]));
            FOTO_TRY(shape_int(s.p[3] + s.p[1] / 2, who, k, &L->y1[k]));
            L->x0[k] = std::max(L->x0[k], 0);
            L->y0[k] = std::max(L->y0[k], 0);
            L->x1[k] = std::min(L->x1[k], w);
            L->y1[k] = std::min(L->y1[k], h);
        } else {                         // p = R, c_x, c_y
            for (int j = 0; j < 3; ++j)
                if (!std::isfinite(s.p[j])) {
                    set_error("%s: shape %d: parameter %g is not finite", who, k, s.p[j]);
                    return FOTO_ERR_ARG;
                }
            L->R[k] = s.p[0];
            L->cx[k] = s.p[1];
            L->cy[k] = s.p[2];
        }
    }
    return 0;
}

// the checks the two pair entries share; host-only
int pair_check(const foto_image* f0, const foto_image* f1, int w, int h, const char* who) {
    if (!f0 || !f1) { set_error("%s: null image descriptor", who); return FOTO_ERR_ARG; }
    FOTO_TRY(image_size_check(w, h, 1, who));
    FOTO_TRY(image_check(f0, w, h, who));
    FOTO_TRY(image_check(f1, w, h, who));
    return 0;
}

hipError_t launch_minmax(int64_t n, const double* sub, double* x, double* part, double* out2, hipStream_t s) {
    const int nb = capped_blocks(n, SUM_MAX_BLOCKS);
    k_minmax_partial<<<nb, NT, 0, s>>>(n, sub, x, part);
    k_minmax_final<<<1, NT, 0, s>>>(nb, part, out2);
    return hipGetLastError();
}

}  // namespace
}  // namespace foto

extern "C" {

int foto_resize_coeffs(int n_in, int n_out, int filter, int* ksize, int* bounds, double* kk, int32_t* kk_int, int cap) {
    static const char* const who = "foto_resize_coeffs";
    if (!ksize) { set_error("%s: ksize is null", who); return FOTO_ERR_ARG; }
    FOTO_TRY(size_pair_check(n_in, 1, n_out, 1, filter, who));
    AxisTable T;
    axis_table(n_in, n_out, filter, &T);
    *ksize = T.ksize;
    if ((kk || kk_int) && (int64_t)cap < (int64_t)n_out * T.ksize) {
        set_error("%s: cap = %d; the tables hold n_out * ksize = %lld entries", who, cap, (long long)n_out * T.ksize);
        return FOTO_ERR_ARG;
    }
    if (bounds) memcpy(bounds, T.bounds.data(), T.bounds.size() * sizeof(int));
    if (kk) memcpy(kk, T.kk.data(), T.kk.size() * sizeof(double));
    if (kk_int) memcpy(kk_int, T.kki.data(), T.kki.size() * sizeof(int));
    return 0;
}

int foto_resize_plan_create(int w, int h, int ow, int oh, int filter, foto_resize_plan** out) {
    static const char* const who = "foto_resize_plan_create";
    if (!out) { set_error("%s: null pointer", who); return FOTO_ERR_ARG; }
    *out = nullptr;
    FOTO_TRY(size_pair_check(w, h, ow, oh, filter, who));
    foto_resize_plan* p = new foto_resize_plan();
    p->w = w; p->h = h; p->ow = ow; p->oh = oh; p->filter = filter;
    axis_table(w, ow, filter, &p->X);
    axis_table(h, oh, filter, &p->Y);
    p->span_x = max_tile_span(p->X);
    int rc = hipGetDevice(&p->device) == hipSuccess ? 0 : FOTO_ERR_HIP;
    if (rc < 0) set_error("%s: hipGetDevice failed", who);
    if (rc == 0) rc = stream_acquire(&p->s);
    if (rc == 0) rc = plan_upload(p);
    if (rc < 0) { delete p; return rc; }
    *out = p;
    return 0;
}

void foto_resize_plan_destroy(foto_resize_plan* p) { delete p; }

int foto_resize_plan_device(const foto_resize_plan* p) { return p ? p->device : -1; }

int foto_resize_plan_info(const foto_resize_plan* p, int* info8) {
    if (!p || !info8) { set_error("foto_resize_plan_info: null pointer"); return FOTO_ERR_ARG; }
    const int v[8] = {p->w, p->h, p->ow, p->oh, p->filter, p->X.ksize, p->Y.ksize, p->span_x};
    memcpy(info8, v, sizeof(v));
    return 0;
}

int foto_resize_dev(foto_resize_plan* p, const foto_image* src, int channels, int64_t stride_c, void* out,
                    int out_planar, int route, void* stream) {
    static const char* const who = "foto_resize_dev";
    if (!p || !src || !out) { set_error("%s: null pointer", who); return FOTO_ERR_ARG; }
    FOTO_TRY(interp_frame_check(src, channels, stride_c, p->w, p->h, who));
    if ((uintptr_t)out % dtype_bytes(src->dtype) != 0) {
        set_error("%s: out %p is not aligned to its %zu-byte element", who, out, dtype_bytes(src->dtype));
        return FOTO_ERR_ARG;
    }
    if (out_planar != 0 && out_planar != 1) {
        set_error("%s: out_planar = %d is not 0 ([oh][ow][channels]) / 1 ([channels][oh][ow])", who, out_planar);
        return FOTO_ERR_ARG;
    }
    bool use_lds = false;
    FOTO_TRY(route_pick(p, route, who, &use_lds));
    std::lock_guard<std::mutex> lk(p->mu);
    const size_t src_bytes = interp_frame_bytes(src, channels, stride_c, p->w, p->h);
    const size_t out_bytes = (size_t)p->ow * (size_t)p->oh * (size_t)channels * dtype_bytes(src->dtype);
    FOTO_TRY(dev_ptr_check(src->data, src_bytes, p->device, who, "image data (all channels)"));
    FOTO_TRY(dev_ptr_check(out, out_bytes, p->device, who, "out"));
    if (overlaps(out, out_bytes, src->data, src_bytes)) {
        set_error("%s: out may not overlap the frame", who);
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(p->link.enter((hipStream_t)stream, p->s));
    const View sv{0, stride_c, src->stride_y, src->stride_x};
    const View dv = out_planar ? View{0, (int64_t)p->ow * p->oh, p->ow, 1}              // [channels][oh][ow]
                               : View{0, 1, (int64_t)p->ow * channels, channels};   // [oh][ow][channels]
    Scales one;
    one.s[0] = one.s[1] = one.s[2] = 1.0;
    one.mod = 1;
    return leave_with(p->link, p->s, stream,
                      resize_dispatch(p, src->dtype, src->data, sv, out, dv, 1, channels, one, use_lds));
}

int foto_flow_resize_dev(foto_resize_plan* p, const foto_flow* fl, void* out, int route, void* stream) {
    static const char* const who = "foto_flow_resize_dev";
    if (!p || !fl || !out) { set_error("%s: null pointer", who); return FOTO_ERR_ARG; }
    FOTO_TRY(flow_check(fl, p->w, p->h, who));
    if ((uintptr_t)out % dtype_bytes(fl->dtype) != 0) {
        set_error("%s: out %p is not aligned to its %zu-byte element", who, out, dtype_bytes(fl->dtype));
        return FOTO_ERR_ARG;
    }
    bool use_lds = false;
    FOTO_TRY(route_pick(p, route, who, &use_lds));
    std::lock_guard<std::mutex> lk(p->mu);
    foto_flow ofl = *fl;
    ofl.data = out;
    const size_t in_bytes = flow_bytes(fl, p->w, p->h), out_bytes = flow_bytes(&ofl, p->ow, p->oh);
    FOTO_TRY(dev_ptr_check(fl->data, in_bytes, p->device, who, "flow data"));
    FOTO_TRY(dev_ptr_check(out, out_bytes, p->device, who, "out"));
    if (overlaps(out, out_bytes, fl->data, in_bytes)) {
        set_error("%s: out may not overlap the flow", who);
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(p->link.enter((hipStream_t)stream, p->s));
    const int64_t n = (int64_t)p->w * p->h, on = (int64_t)p->ow * p->oh;
    Scales sa;
    sa.s[0] = (double)p->ow / p->w;
    sa.s[1] = (double)p->oh / p->h;
    sa.s[2] = 1.0;
    View sv, dv;
    int64_t P;
    int C;
    if (fl->layout == 0) {   // [records][3][h][w]: 3 records planes, u, v, m
        P = (int64_t)fl->records * 3;
        C = 1;
        sa.mod = 3;
        sv = View{n, 0, p->w, 1};
        dv = View{on, 0, p->ow, 1};
    } else {                 // [records][h][w][2]: two interleaved channels, u, v
        P = fl->records;
        C = 2;
        sa.mod = 2;
        sv = View{2 * n, 1, 2 * (int64_t)p->w, 2};
        dv = View{2 * on, 1, 2 * (int64_t)p->ow, 2};
    }
    return leave_with(p->link, p->s, stream, resize_dispatch(p, fl->dtype, fl->data, sv, out, dv, P, C, sa, use_lds));
}

int foto_prep_gray_dev(const foto_image* src, int channels, int64_t stride_c, int w, int h, void* out, void* stream) {
    static const char* const who = "foto_prep_gray_dev";
    if (!src || !out) { set_error("%s: null pointer", who); return FOTO_ERR_ARG; }
    if (channels != 3 && channels != 4) {
        set_error("%s: channels = %d; a colour frame has 3 (RGB) or 4 (RGBA, alpha ignored)", who, channels);
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(image_size_check(w, h, 1, who));
    FOTO_TRY(interp_frame_check(src, channels, stride_c, w, h, who));
    FOTO_TRY(out_check(out, src->dtype, who, "out"));
    std::lock_guard<std::mutex> lk(pd_mu);
    int device = 0;
    PrepDev* pd = nullptr;
    FOTO_TRY(prep_dev(&device, &pd));
    const size_t src_bytes = interp_frame_bytes(src, channels, stride_c, w, h);
    const size_t out_bytes = (size_t)w * (size_t)h * dtype_bytes(src->dtype);
    FOTO_TRY(dev_ptr_check(src->data, src_bytes, device, who, "image data (all channels)"));
    FOTO_TRY(dev_ptr_check(out, out_bytes, device, who, "out"));
    if (overlaps(out, out_bytes, src->data, src_bytes)) {
        set_error("%s: out may not overlap the frame", who);
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(pd->link.enter((hipStream_t)stream, pd->s));
    switch (src->dtype) {
        case FOTO_U8: gray_launch<unsigned char>(src, stride_c, w, h, out, pd->s); break;
        case FOTO_F32: gray_launch<float>(src, stride_c, w, h, out, pd->s); break;
        default: gray_launch<double>(src, stride_c, w, h, out, pd->s); break;
    }
    return leave_with(pd->link, pd->s, stream, last_launch());
}

int foto_prep_illuminate_dev(const foto_image* src, int w, int h, const foto_lum_shape* shapes, int count, void* out,
                             int out_dtype, void* stream) {
    static const char* const who = "foto_prep_illuminate_dev";
    if (!src) { set_error("%s: null image descriptor", who); return FOTO_ERR_ARG; }
    FOTO_TRY(image_size_check(w, h, 1, who));
    FOTO_TRY(image_check(src, w, h, who));
    FOTO_TRY(out_check(out, out_dtype, who, "out"));
    LumArgs L;
    FOTO_TRY(lum_args(shapes, count, w, h, who, &L));
    std::lock_guard<std::mutex> lk(pd_mu);
    int device = 0;
    PrepDev* pd = nullptr;
    FOTO_TRY(prep_dev(&device, &pd));
    const size_t src_bytes = image_bytes(src, w, h), out_bytes = (size_t)w * (size_t)h * dtype_bytes(out_dtype);
    FOTO_TRY(image_dev_check(src, w, h, device, who));
    FOTO_TRY(dev_ptr_check(out, out_bytes, device, who, "out"));
    if (overlaps(out, out_bytes, src->data, src_bytes)) {
        set_error("%s: out may not overlap the frame", who);
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(pd->link.enter((hipStream_t)stream, pd->s));
    switch (src->dtype) {
        case FOTO_U8: illuminate_launch<unsigned char>(src, w, h, L, out, out_dtype, pd->s); break;
        case FOTO_F32: illuminate_launch<float>(src, w, h, L, out, out_dtype, pd->s); break;
        default: illuminate_launch<double>(src, w, h, L, out, out_dtype, pd->s); break;
    }
    return leave_with(pd->link, pd->s, stream, last_launch());
}

int foto_prep_normalize_pair_dev(const foto_image* f0, const foto_image* f1, int w, int h, void* out0, void* out1,
                                 int out_dtype, double* stats4, void* stream) {
    static const char* const who = "foto_prep_normalize_pair_dev";
    FOTO_TRY(pair_check(f0, f1, w, h, who));
    FOTO_TRY(out_check(out0, out_dtype, who, "out0"));
    FOTO_TRY(out_check(out1, out_dtype, who, "out1"));
    if (!stats4) { set_error("%s: stats4 is null", who); return FOTO_ERR_ARG; }
    int device = 0;
    FOTO_HIP_CHECK(hipGetDevice(&device));
    const int64_t n = (int64_t)w * h;
    const size_t out_bytes = (size_t)n * dtype_bytes(out_dtype);
    FOTO_TRY(image_dev_check(f0, w, h, device, who));
    FOTO_TRY(image_dev_check(f1, w, h, device, who));
    FOTO_TRY(dev_ptr_check(out0, out_bytes, device, who, "out0"));
    FOTO_TRY(dev_ptr_check(out1, out_bytes, device, who, "out1"));
    if (overlaps(out0, out_bytes, out1, out_bytes) || overlaps(out0, out_bytes, f0->data, image_bytes(f0, w, h)) ||
        overlaps(out0, out_bytes, f1->data, image_bytes(f1, w, h)) ||
        overlaps(out1, out_bytes, f0->data, image_bytes(f0, w, h)) ||
        overlaps(out1, out_bytes, f1->data, image_bytes(f1, w, h))) {
        set_error("%s: the outputs may not overlap each other or a frame", who);
        return FOTO_ERR_ARG;
    }
    // the call's stream and temporaries: both frames as float64, the partials, six scalars
    StreamLink link;
    CallScope S;
    FOTO_TRY(S.init());
    const int nb = capped_blocks(n, SUM_MAX_BLOCKS);
    double* buf = nullptr;
    FOTO_TRY(S.dev(2 * (size_t)n + 2 * (size_t)nb + 6, &buf));
    double *v0 = buf, *v1 = buf + n, *part = buf + 2 * n, *scal = part + 2 * nb;
    FOTO_TRY(link.enter((hipStream_t)stream, S.s));
    FOTO_HIP_CHECK(launch_ingest(*f0, w, h, v0, S.s));
    FOTO_HIP_CHECK(launch_ingest(*f1, w, h, v1, S.s));
    FOTO_HIP_CHECK(launch_sum(n, v0, part, scal + 0, S.s));   // (the order of normalize = 1)
    FOTO_HIP_CHECK(launch_sum(n, v1, part, scal + 1, S.s));
    FOTO_HIP_CHECK(launch_minmax(n, nullptr, v0, part, scal + 2, S.s));
    FOTO_HIP_CHECK(launch_minmax(n, nullptr, v1, part, scal + 4, S.s));
    const int ob = capped_blocks(n, STREAM_MAX_BLOCKS);
    switch (out_dtype) {
        case FOTO_U8:
            k_normalize_out<unsigned char><<<ob, NT, 0, S.s>>>(n, v0, v1, scal, (unsigned char*)out0, (unsigned char*)out1);
            break;
        case FOTO_F32: k_normalize_out<float><<<ob, NT, 0, S.s>>>(n, v0, v1, scal, (float*)out0, (float*)out1); break;
        default: k_normalize_out<double><<<ob, NT, 0, S.s>>>(n, v0, v1, scal, (double*)out0, (double*)out1); break;
    }
    FOTO_HIP_CHECK(hipGetLastError());
    double hs[6];
    FOTO_HIP_CHECK(hipMemcpyAsync(hs, scal, sizeof(hs), hipMemcpyDeviceToHost, S.s));
    FOTO_TRY(link.leave(S.s, (hipStream_t)stream));
    FOTO_TRY(S.sync());
    stats4[0] = hs[0]; stats4[1] = hs[1]; stats4[2] = hs[3]; stats4[3] = hs[5];
    return 0;
}

int foto_prep_diff_dev(const foto_image* f0, const foto_image* f1, int w, int h, void* out, int out_dtype,
                       double* minmax2_or_null, void* stream) {
    static const char* const who = "foto_prep_diff_dev";
    FOTO_TRY(pair_check(f0, f1, w, h, who));
    FOTO_TRY(out_check(out, out_dtype, who, "out"));
    int device = 0;
    FOTO_HIP_CHECK(hipGetDevice(&device));
    const int64_t n = (int64_t)w * h;
    const size_t out_bytes = (size_t)n * dtype_bytes(out_dtype);
    FOTO_TRY(image_dev_check(f0, w, h, device, who));
    FOTO_TRY(image_dev_check(f1, w, h, device, who));
    FOTO_TRY(dev_ptr_check(out, out_bytes, device, who, "out"));
    if (overlaps(out, out_bytes, f0->data, image_bytes(f0, w, h)) ||
        overlaps(out, out_bytes, f1->data, image_bytes(f1, w, h))) {
        set_error("%s: out may not overlap a frame", who);
        return FOTO_ERR_ARG;
    }
    StreamLink link;
    CallScope S;
    FOTO_TRY(S.init());
    const int nb = capped_blocks(n, SUM_MAX_BLOCKS);
    double* buf = nullptr;
    FOTO_TRY(S.dev(2 * (size_t)n + 2 * (size_t)nb + 2, &buf));
    double *v0 = buf, *d = buf + n, *part = buf + 2 * n, *mm = part + 2 * nb;
    FOTO_TRY(link.enter((hipStream_t)stream, S.s));
    FOTO_HIP_CHECK(launch_ingest(*f0, w, h, v0, S.s));
    FOTO_HIP_CHECK(launch_ingest(*f1, w, h, d, S.s));
    FOTO_HIP_CHECK(launch_minmax(n, v0, d, part, mm, S.s));   // d <- f1 - f0, its minimum and maximum
    const int ob = capped_blocks(n, STREAM_MAX_BLOCKS);
    switch (out_dtype) {
        case FOTO_U8: k_diff_out<unsigned char><<<ob, NT, 0, S.s>>>(n, d, mm, (unsigned char*)out); break;
        case FOTO_F32: k_diff_out<float><<<ob, NT, 0, S.s>>>(n, d, mm, (float*)out); break;
        default: k_diff_out<double><<<ob, NT, 0, S.s>>>(n, d, mm, (double*)out); break;
    }
    FOTO_HIP_CHECK(hipGetLastError());
    double hm[2] = {0, 0};
    if (minmax2_or_null) FOTO_HIP_CHECK(hipMemcpyAsync(hm, mm, sizeof(hm), hipMemcpyDeviceToHost, S.s));
    FOTO_TRY(link.leave(S.s, (hipStream_t)stream));
    FOTO_TRY(S.sync());
    if (minmax2_or_null) { minmax2_or_null[0] = hm[0]; minmax2_or_null[1] = hm[1]; }
    return 0;
}

}  // extern "C"

static_assert(sizeof(foto_lum_shape) == 48, "foto_lum_shape layout");
