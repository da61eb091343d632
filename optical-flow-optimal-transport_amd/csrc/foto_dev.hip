// Device-buffer interface (include/foto.h, "device buffers"): the strided image descriptor's
// validation, the ingest kernels (uint8 / float32 / float64 strided image -> the solvers'
// contiguous float64 frame), the export kernels (float64 fields -> float32 / float64, planar or
// interleaved), the fixed-order frame sum of normalize = 1, and the small device-memory
// utilities.  The entries that need a context's or plan's internals (foto_bb_*_dev,
// foto_gn_plan_solve_dev, the evaluation *_dev calls) live next to their host twins and call the
// launchers below.
//
// Built with -ffp-contract=off like every other unit: value = (double)pixel / divisor is one
// IEEE division (numpy's img.astype(np.float64) / 255), never a multiply by a reciprocal, and
// (float)x rounds to nearest even as np.float32(x) does.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "foto_devutil.h"
#include "foto_internal.h"

namespace foto {

namespace {

template <class T> struct Vec16;   // the 16-byte load of the vector path
template <> struct Vec16<unsigned char> { typedef unsigned int type __attribute__((ext_vector_type(4))); };
template <> struct Vec16<float> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct Vec16<double> { typedef double type __attribute__((ext_vector_type(2))); };

// One work item = one chunk of VE = 16 / sizeof(T) pixels of a row (cpr chunks per row).  VEC: the
// rows are unit-stride and every row start is 16-byte aligned -- a full chunk is one 16-byte
// load (read once: non-temporal); the row tail, and every chunk of the scalar kernel, go pixel
// by pixel through the strides.  Consecutive lanes take consecutive chunks of a row, so both
// the loads and the float64 stores of a wave cover one contiguous span.
template <class T, bool VEC>
__global__ __launch_bounds__(NT) void k_ingest(const T* __restrict__ src, int64_t sy, int64_t sx, int w, int h,
                                               int cpr, double divisor, double* __restrict__ dst) {
    constexpr int VE = 16 / (int)sizeof(T);
    const int64_t nchunk = (int64_t)h * cpr;
    for (int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x; t < nchunk; t += (int64_t)gridDim.x * NT) {
        const int row = (int)(t / cpr);
        const int c0 = (int)(t - (int64_t)row * cpr) * VE;
        const T* rp = src + (int64_t)row * sy;
        double* out = dst + (int64_t)row * w + c0;
        if (VEC && c0 + VE <= w) {
            typedef typename Vec16<T>::type V;
            const V q = __builtin_nontemporal_load((const V*)(rp + c0));
            T e[VE];
            __builtin_memcpy(e, &q, 16);
#pragma unroll
            for (int k = 0; k < VE; ++k) out[k] = (double)e[k] / divisor;
        } else {
            const int ce = c0 + VE < w ? c0 + VE : w;
            for (int c = c0; c < ce; ++c) out[c - c0] = (double)rp[(int64_t)c * sx] / divisor;
        }
    }
}

// fixed-order sum: a grid that depends on n only, per-thread strided partial sums, the block
// tree (block_tree_sum), then one block over the block partials
__global__ __launch_bounds__(NT) void k_sum_partial(int64_t n, const double* __restrict__ x,
                                                    double* __restrict__ part) {
    __shared__ double sh[NT];
    double acc[1] = {0.0};
    for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < n; p += (int64_t)gridDim.x * NT) acc[0] += x[p];
    block_tree_sum<NT>(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(NT) void k_sum_final(int nb, const double* __restrict__ part, double* __restrict__ tot) {
    __shared__ double sh[NT];
    double acc[1] = {0.0};
    for (int b = threadIdx.x; b < nb; b += NT) acc[0] += part[b];
    block_tree_sum<NT>(acc, sh);
    if (threadIdx.x == 0) tot[0] = sh[0];
}

__global__ __launch_bounds__(NT) void k_div_scalar(int64_t n, double* __restrict__ x, const double* __restrict__ S) {
    const double d = S[0];
    for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < n; p += (int64_t)gridDim.x * NT) x[p] = x[p] / d;
}

// LAYOUT 0: planar [3][n] = a, b, c; 1: interleaved [n][2] = (a, b)
template <class T, int LAYOUT>
__global__ __launch_bounds__(NT) void k_export(int64_t n, const double* __restrict__ a, const double* __restrict__ b,
                                               const double* __restrict__ c, T* __restrict__ out) {
    for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < n; p += (int64_t)gridDim.x * NT) {
        if (LAYOUT == 0) {
            out[p] = (T)a[p];
            out[n + p] = (T)b[p];
            out[2 * n + p] = (T)c[p];
        } else {
            out[2 * p] = (T)a[p];
            out[2 * p + 1] = (T)b[p];
        }
    }
}

// (float)x rounds to nearest even; uint8 is (uint8)(255 * clip(x, 0, 1) + 0.5), NaN -> 0: to
// nearest, so a u8 frame ingested with divisor 255 comes back (255 * (49 / 255.0) is 48.99...)
template <class T> __device__ __forceinline__ T frame_cast(double x) { return (T)x; }
template <> __device__ __forceinline__ unsigned char frame_cast<unsigned char>(double x) {
    if (!(x >= 0.0)) x = 0.0;
    if (x > 1.0) x = 1.0;
    return (unsigned char)(255.0 * x + 0.5);
}

// The multiply by scale comes last: an integer position with scale == 1 gives the plane's bits.
__device__ __forceinline__ double frame_value(const double* __restrict__ a, const double* __restrict__ b, double w,
                                              double scale, int64_t p) {
    if (w == 0.0) return scale * a[p];
    if (w == 1.0) return scale * b[p];
    return scale * ((1.0 - w) * a[p] + w * b[p]);
}

// Frame k = blockIdx.y: out[k][0..n) from one or two density planes.  One work item = one
// 16-byte store of VE = 16 / sizeof(T) pixels; a frame starts at any element-aligned address
// (n * sizeof(T) need not be a multiple of 16), so item 0 takes the pixels before the frame's
// first 16-byte boundary, the last item the tail, one by one.
template <class T>
__global__ __launch_bounds__(NT) void k_frames(FrameArgs fa, int64_t n, double scale, T* __restrict__ out) {
    constexpr int VE = 16 / (int)sizeof(T);
    const int k = blockIdx.y;
    const double* __restrict__ a = fa.a[k];
    const double* __restrict__ b = fa.b[k];
    const double w = fa.w[k];
    T* __restrict__ o = out + (int64_t)k * n;
    int64_t head = (int64_t)(((16 - ((uintptr_t)o & 15)) & 15) / sizeof(T));
    if (head > n) head = n;
    const int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (t == 0) {
        for (int64_t p = 0; p < head; ++p) o[p] = frame_cast<T>(frame_value(a, b, w, scale, p));
        return;
    }
    const int64_t p0 = head + (t - 1) * VE;
    if (p0 >= n) return;
    if (p0 + VE <= n) {
        typedef typename Vec16<T>::type V;
        T e[VE];
#pragma unroll
        for (int j = 0; j < VE; ++j) e[j] = frame_cast<T>(frame_value(a, b, w, scale, p0 + j));
        V q;
        __builtin_memcpy(&q, e, 16);
        *(V*)(o + p0) = q;
    } else {
        for (int64_t p = p0; p < n; ++p) o[p] = frame_cast<T>(frame_value(a, b, w, scale, p));
    }
}

template <class T>
hipError_t frames_t(const FrameArgs& fa, int count, int64_t n, double scale, void* out, hipStream_t s) {
    constexpr int VE = 16 / (int)sizeof(T);
    const int64_t items = (n + VE - 1) / VE + 2;   // the head item, the chunks, a tail behind a head
    k_frames<T><<<dim3((unsigned)flat_blocks(items), (unsigned)count), NT, 0, s>>>(fa, n, scale, (T*)out);
    return hipGetLastError();
}

template <class T>
hipError_t ingest_t(const foto_image& im, int w, int h, double* dst, hipStream_t s) {
    constexpr int VE = 16 / (int)sizeof(T);
    const int cpr = (w + VE - 1) / VE;
    const T* src = (const T*)im.data;
    const bool vec = im.stride_x == 1 && ((uintptr_t)im.data % 16) == 0 &&
                     (((uint64_t)im.stride_y * sizeof(T)) % 16) == 0;
    const int nb = capped_blocks((int64_t)h * cpr, STREAM_MAX_BLOCKS);
    if (vec) k_ingest<T, true><<<nb, NT, 0, s>>>(src, im.stride_y, im.stride_x, w, h, cpr, im.divisor, dst);
    else k_ingest<T, false><<<nb, NT, 0, s>>>(src, im.stride_y, im.stride_x, w, h, cpr, im.divisor, dst);
    return hipGetLastError();
}

template <class T>
hipError_t export_t(int64_t n, const double* a, const double* b, const double* c, void* out, int layout,
                    hipStream_t s) {
    const int nb = capped_blocks(n, STREAM_MAX_BLOCKS);
    if (layout == 0) k_export<T, 0><<<nb, NT, 0, s>>>(n, a, b, c, (T*)out);
    else k_export<T, 1><<<nb, NT, 0, s>>>(n, a, b, c, (T*)out);
    return hipGetLastError();
}

}  // namespace

// ----------------------------------------------------------------------------- validation

int image_check(const foto_image* im, int w, int h, const char* who) {
    if (!im) { set_error("%s: null image descriptor", who); return FOTO_ERR_ARG; }
    if (w < 1 || h < 1) { set_error("%s: w = %d, h = %d: both must be >= 1", who, w, h); return FOTO_ERR_ARG; }
    if (!im->data) { set_error("%s: image data is null", who); return FOTO_ERR_ARG; }
    if (im->dtype < FOTO_U8 || im->dtype > FOTO_F64) {
        set_error("%s: dtype %d is not FOTO_U8 / FOTO_F32 / FOTO_F64", who, im->dtype);
        return FOTO_ERR_ARG;
    }
    if (im->stride_x <= 0 || im->stride_y <= 0) {
        set_error("%s: strides (%lld, %lld) must both be > 0 (in elements)", who, (long long)im->stride_y,
                  (long long)im->stride_x);
        return FOTO_ERR_ARG;
    }
    if (!(im->divisor != 0.0) || !std::isfinite(im->divisor)) {
        set_error("%s: divisor %g must be finite and non-zero", who, im->divisor);
        return FOTO_ERR_ARG;
    }
    if ((uintptr_t)im->data % dtype_bytes(im->dtype) != 0) {
        set_error("%s: data %p is not aligned to its %zu-byte element", who, im->data, dtype_bytes(im->dtype));
        return FOTO_ERR_ARG;
    }
    // the w x h pixels must be distinct elements: the lines along the minor stride may not
    // reach into each other
    const bool x_minor = im->stride_x <= im->stride_y;
    const int64_t major = x_minor ? im->stride_y : im->stride_x, minor = x_minor ? im->stride_x : im->stride_y;
    const int64_t len = x_minor ? w : h, lines = x_minor ? h : w;
    if (lines > 1 && major < (len - 1) * minor + 1) {
        set_error("%s: strides (%lld, %lld) make the %s of a %d x %d image overlap", who, (long long)im->stride_y,
                  (long long)im->stride_x, x_minor ? "rows" : "columns", w, h);
        return FOTO_ERR_ARG;
    }
    return 0;
}

// [p, p + bytes) must be device memory of `device`: hipPointerGetAttributes knows every
// allocation of the runtime, a pointer it does not know (plain host memory) is an error there
int dev_ptr_check(const void* p, size_t bytes, int device, const char* who, const char* what) {
    if (!p) { set_error("%s: %s is null", who, what); return FOTO_ERR_ARG; }
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof(at));
    const hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();   // (the lookup failure is this call's answer, not a sticky error)
        set_error("%s: %s %p is not memory of the HIP runtime (%s); a device pointer is required", who, what, p,
                  hipGetErrorString(e));
        return FOTO_ERR_ARG;
    }
    if (at.type != hipMemoryTypeDevice) {
        set_error("%s: %s %p is not device memory (memory type %d)", who, what, p, (int)at.type);
        return FOTO_ERR_ARG;
    }
    if (at.device != device) {
        set_error("%s: %s %p lives on device %d, the solver on device %d", who, what, p, at.device, device);
        return FOTO_ERR_ARG;
    }
    // the extent, where the runtime can tell the allocation's range
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) == hipSuccess && base && size) {
        const uintptr_t lo = (uintptr_t)base, hi = lo + size, a = (uintptr_t)p;
        if (a < lo || a + bytes > hi) {
            set_error("%s: %s %p + %zu bytes runs past its allocation [%p, +%zu)", who, what, p, bytes, (void*)base, size);
            return FOTO_ERR_ARG;
        }
    } else {
        (void)hipGetLastError();
    }
    return 0;
}

int image_dev_check(const foto_image* im, int w, int h, int device, const char* who) {
    FOTO_TRY(image_check(im, w, h, who));
    const size_t last = (size_t)(h - 1) * (size_t)im->stride_y + (size_t)(w - 1) * (size_t)im->stride_x;
    return dev_ptr_check(im->data, (last + 1) * dtype_bytes(im->dtype), device, who, "image data");
}

int export_check(const void* out, int dtype, int layout, int64_t n, int device, const char* who) {
    if (dtype != FOTO_F32 && dtype != FOTO_F64) {
        set_error("%s: output dtype %d is not FOTO_F32 / FOTO_F64", who, dtype);
        return FOTO_ERR_ARG;
    }
    if (layout != 0 && layout != 1) {
        set_error("%s: layout %d is not 0 (planar u, v, m) / 1 (interleaved (u, v))", who, layout);
        return FOTO_ERR_ARG;
    }
    if (out && (uintptr_t)out % dtype_bytes(dtype) != 0) {
        set_error("%s: out %p is not aligned to its %zu-byte element", who, out, dtype_bytes(dtype));
        return FOTO_ERR_ARG;
    }
    return dev_ptr_check(out, (size_t)n * (layout == 0 ? 3 : 2) * dtype_bytes(dtype), device, who, "out");
}

int track_arg_check(const void* pts, const void* out, int64_t M, int all_steps, const char* who) {
    if (!pts || !out) { set_error("%s: null pointer", who); return FOTO_ERR_ARG; }
    if (M < 1 || M > (int64_t)INT32_MAX) {
        set_error("%s: M = %lld points must be in [1, 2^31 - 1]", who, (long long)M);
        return FOTO_ERR_ARG;
    }
    if (all_steps != 0 && all_steps != 1) {
        set_error("%s: all_steps = %d is not 0 (the last record) / 1 (every record)", who, all_steps);
        return FOTO_ERR_ARG;
    }
    return 0;
}

int track_dtype_check(const void* p, int dtype, const char* who, const char* what) {
    if (dtype != FOTO_F32 && dtype != FOTO_F64) {
        set_error("%s: %s dtype %d is not FOTO_F32 / FOTO_F64", who, what, dtype);
        return FOTO_ERR_ARG;
    }
    if ((uintptr_t)p % (2 * dtype_bytes(dtype)) != 0) {   // one (x, y) pair is one vector load / store
        set_error("%s: %s %p is not aligned to its %zu-byte (x, y) pair", who, what, p, 2 * dtype_bytes(dtype));
        return FOTO_ERR_ARG;
    }
    return 0;
}

// ----------------------------------------------------------------------------- launchers

hipError_t launch_ingest(const foto_image& im, int w, int h, double* dst, hipStream_t s) {
    switch (im.dtype) {
        case FOTO_U8: return ingest_t<unsigned char>(im, w, h, dst, s);
        case FOTO_F32: return ingest_t<float>(im, w, h, dst, s);
        case FOTO_F64: return ingest_t<double>(im, w, h, dst, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_sum(int64_t n, const double* x, double* part, double* tot, hipStream_t s) {
    const int nb = capped_blocks(n, SUM_MAX_BLOCKS);
    k_sum_partial<<<nb, NT, 0, s>>>(n, x, part);
    k_sum_final<<<1, NT, 0, s>>>(nb, part, tot);
    return hipGetLastError();
}

hipError_t launch_div_scalar(int64_t n, double* x, const double* S, hipStream_t s) {
    k_div_scalar<<<capped_blocks(n, STREAM_MAX_BLOCKS), NT, 0, s>>>(n, x, S);
    return hipGetLastError();
}

hipError_t launch_export(int64_t n, const double* a, const double* b, const double* c, void* out, int dtype,
                         int layout, hipStream_t s) {
    if (dtype == FOTO_F32) return export_t<float>(n, a, b, c, out, layout, s);
    if (dtype == FOTO_F64) return export_t<double>(n, a, b, c, out, layout, s);
    return hipErrorInvalidValue;
}

hipError_t launch_frames(const FrameArgs& fa, int count, int64_t n, double scale, void* out, int dtype,
                         hipStream_t s) {
    if (count < 1 || count > FRAMES_MAX || n < 1) return hipErrorInvalidValue;
    switch (dtype) {
        case FOTO_U8: return frames_t<unsigned char>(fa, count, n, scale, out, s);
        case FOTO_F32: return frames_t<float>(fa, count, n, scale, out, s);
        case FOTO_F64: return frames_t<double>(fa, count, n, scale, out, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace foto

using namespace foto;

extern "C" {

int foto_image_check(const foto_image* im, int w, int h) { return image_check(im, w, h, "foto_image_check"); }

int foto_dev_malloc(size_t bytes, void** out) {
    if (!out) { set_error("foto_dev_malloc: null argument"); return FOTO_ERR_ARG; }
    *out = nullptr;
    FOTO_HIP_CHECK(hipMalloc(out, std::max<size_t>(bytes, 1)));
    return 0;
}

int foto_dev_free(void* p) {
    if (p) FOTO_HIP_CHECK(hipFree(p));
    return 0;
}

int foto_dev_memcpy(void* dst, const void* src, size_t bytes, int kind) {
    if (kind < 0 || kind > 2) { set_error("foto_dev_memcpy: kind %d is not 0 (H2D) / 1 (D2H) / 2 (D2D)", kind); return FOTO_ERR_ARG; }
    if (bytes == 0) return 0;
    if (!dst || !src) { set_error("foto_dev_memcpy: null pointer"); return FOTO_ERR_ARG; }
    static const hipMemcpyKind kinds[3] = {hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice};
    FOTO_HIP_CHECK(hipMemcpy(dst, src, bytes, kinds[kind]));
    return 0;
}

}  // extern "C"

static_assert(sizeof(foto_image) == 40, "foto_image layout");
