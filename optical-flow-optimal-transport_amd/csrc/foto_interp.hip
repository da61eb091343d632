// Maps and in-betweens (include/foto.h, "maps and in-betweens"): the transport read from an
// arbitrary time s, in both directions.  The trajectory through pixel p of the time-s image runs
// back to frame 0 (a) and forward to frame 1 (b):
//   n = (int)s, theta = s - n;   p_n = theta > 0 ? inv(n, theta, p) : p
//   b = p_n pushed through the steps n .. Nt-2 (traj_step, the step of the flow and the tracks)
//   a = p_n pulled back: a <- inv(m, 1, a) for m = n-1 .. 0
// with inv(m, theta, p) the fixed-count inverse step (inv_step, foto_devutil.h).
//   k_maps    the record (a - p, b - p) per pixel and time: out[count][4][Ny][Nx]
//   k_interp  the caller's own frames carried along it: per channel
//             (1 - w_t) S(I0; a) + w_t S(I1; b), w_t = s / (Nt - 1), S the clamped bilinear
//             sample of the pyramid (sample_taps / sample_sum): out[count][Ny][Nx][C]
//
// One thread per (pixel, time): times ride on the grid's second axis (<= MAPS_MAX per launch, the
// positions passed by value), pixels in 2-D tiles of MT_W x MT_H so that a wave -- two tile rows --
// gathers its twelve phi taps from a few rows of the plane, and its stores cover whole 256-byte
// row segments (float64 maps).  Plane m of phi comes from a table of Nt plane pointers (k_plane_table
// fills it from the buffers that own the planes: one per in-process shard), so the chain does not
// care where a plane lives.  The chain is serial and latency-bound: Nt - 1 - n forward steps plus
// inv_iters (n + 1) velocity samples, each twelve loads issued together ahead of their use
// (traj_vel).  Positions are float64 throughout; every load is inside its plane or frame whatever
// the position (trunc_clamp, sample_taps), so a non-finite phi makes non-finite records for the
// pixels whose chains touch it and nothing else.  Built with -ffp-contract=off like every other
// unit: the numpy restatement (tests/interp_ref.py) rounds the same way.
#include <hip/hip_runtime.h>

#include <cmath>

#include "foto_devutil.h"
#include "foto_internal.h"

namespace foto {

namespace {

static_assert(MT_W * MT_H == NT, "one thread per tile pixel");

// table[m] = plane m of phi, for the planes of up to PLANE_SEGS buffers
__global__ __launch_bounds__(NT) void k_plane_table(PlaneSegs sg, int64_t nxy, const double** __restrict__ table) {
    const int k = blockIdx.x;
    for (int l = threadIdx.x; l < sg.nloc[k]; l += NT) table[sg.t0[k] + l] = sg.base[k] + (int64_t)l * nxy;
}

// The two ends of the trajectory through (x, y) of the time-s image; (x, y) in: the pixel centre.
__device__ __forceinline__ void transport_ends(const double* const* __restrict__ table, int Nt, int Nx, int Ny,
                                               double s, int iters, double x, double y, double& ax, double& ay,
                                               double& bx, double& by) {
    int n = (int)s;
    n = n < 0 ? 0 : n > Nt - 1 ? Nt - 1 : n;   // (the host checked s: the table is never overrun)
    const double theta = s - (double)n;
    if (theta > 0.0 && n < Nt - 1) inv_step(table[n], Nx, Ny, theta, iters, x, y);
    bx = x;
    by = y;
    for (int m = n; m < Nt - 1; ++m) traj_step(table[m], Nx, Ny, bx, by);
    ax = x;
    ay = y;
    for (int m = n - 1; m >= 0; --m) inv_step(table[m], Nx, Ny, 1.0, iters, ax, ay);
}

// the tile pixel of this thread; false outside the frame
__device__ __forceinline__ bool tile_pixel(int Nx, int Ny, int& i, int& j) {
    const int tiles_x = (Nx + MT_W - 1) / MT_W;
    const int by = (int)blockIdx.x / tiles_x, bx = (int)blockIdx.x - by * tiles_x;
    i = bx * MT_W + (int)threadIdx.x % MT_W;
    j = by * MT_H + (int)threadIdx.x / MT_W;
    return i < Nx && j < Ny;
}

template <class T>
__global__ __launch_bounds__(NT) void k_maps(const double* const* __restrict__ table, int Nt, int Nx, int Ny,
                                             MapTimes tm, int iters, T* __restrict__ out) {
    int i, j;
    if (!tile_pixel(Nx, Ny, i, j)) return;
    const int k = blockIdx.y;
    double ax, ay, bx, by;
    transport_ends(table, Nt, Nx, Ny, tm.s[k], iters, (double)i, (double)j, ax, ay, bx, by);
    const int64_t nxy = (int64_t)Nx * Ny;
    T* __restrict__ o = out + (int64_t)k * 4 * nxy + (int64_t)j * Nx + i;
    o[0] = (T)(ax - (double)i);
    o[nxy] = (T)(ay - (double)j);
    o[2 * nxy] = (T)(bx - (double)i);
    o[3 * nxy] = (T)(by - (double)j);
}

// (double)pixel / divisor of element e of a frame whose dtype is a launch-wide value (a uniform
// branch); x / 1.0 is x bit for bit, so the float frames' default skips the division
__device__ __forceinline__ double frame_px(const void* __restrict__ base, int dtype, int64_t e, double divisor) {
    double v;
    if (dtype == FOTO_U8) v = (double)((const unsigned char*)base)[e];
    else if (dtype == FOTO_F32) v = (double)((const float*)base)[e];
    else v = ((const double*)base)[e];
    return divisor == 1.0 ? v : v / divisor;
}

struct FrameView {
    const void* data;
    int dtype;
    int64_t sy, sx, sc;
    double divisor;
};

// S(frame channel c; taps T): the four taps as element offsets o00 .. o11 of channel 0
__device__ __forceinline__ double frame_sample(const FrameView& f, const SampleTaps& T, int64_t o00, int c) {
    const int64_t e = o00 + (int64_t)c * f.sc;
    return sample_sum(T, frame_px(f.data, f.dtype, e, f.divisor), frame_px(f.data, f.dtype, e + f.sx, f.divisor),
                      frame_px(f.data, f.dtype, e + f.sy, f.divisor),
                      frame_px(f.data, f.dtype, e + f.sy + f.sx, f.divisor));
}

// (float)x rounds to nearest even; uint8 is foto_bb_frames' rule, (uint8)(255 clip(x, 0, 1) + 0.5),
// NaN -> 0: to nearest, so that s = 0 and s = Nt - 1 give a u8 frame back unchanged
template <class T> __device__ __forceinline__ T interp_cast(double x) { return (T)x; }
template <> __device__ __forceinline__ unsigned char interp_cast<unsigned char>(double x) {
    if (!(x >= 0.0)) x = 0.0;
    if (x > 1.0) x = 1.0;
    return (unsigned char)(255.0 * x + 0.5);
}

template <class T>
__global__ __launch_bounds__(NT) void k_interp(const double* const* __restrict__ table, int Nt, int Nx, int Ny,
                                               MapTimes tm, int iters, FrameView f0, FrameView f1, int C,
                                               T* __restrict__ out) {
    int i, j;
    if (!tile_pixel(Nx, Ny, i, j)) return;
    const int k = blockIdx.y;
    const double s = tm.s[k];
    double ax, ay, bx, by;
    transport_ends(table, Nt, Nx, Ny, s, iters, (double)i, (double)j, ax, ay, bx, by);
    // the weights and taps of both ends, once for every channel
    const SampleTaps Ta = sample_taps(Nx, Ny, ax, ay), Tb = sample_taps(Nx, Ny, bx, by);
    const int64_t oa = (int64_t)Ta.j0 * f0.sy + (int64_t)Ta.i0 * f0.sx;
    const int64_t ob = (int64_t)Tb.j0 * f1.sy + (int64_t)Tb.i0 * f1.sx;
    const double wt = s / (double)(Nt - 1);
    T* __restrict__ o = out + (((int64_t)k * Ny + j) * Nx + i) * C;
    for (int c = 0; c < C; ++c) {
        const double va = frame_sample(f0, Ta, oa, c), vb = frame_sample(f1, Tb, ob, c);
        o[c] = interp_cast<T>((1.0 - wt) * va + wt * vb);
    }
}

FrameView frame_view(const foto_image& im, int64_t sc) {
    return FrameView{im.data, im.dtype, im.stride_y, im.stride_x, sc, im.divisor};
}

dim3 maps_grid(int Nx, int Ny, int count) {
    return dim3((unsigned)(((Nx + MT_W - 1) / MT_W) * ((Ny + MT_H - 1) / MT_H)), (unsigned)count);
}

bool maps_launch_ok(int Nt, int Nx, int Ny, int count, int iters) {
    return Nt >= 2 && Nx >= 2 && Ny >= 2 && count >= 1 && count <= MAPS_MAX && iters >= 1 && iters <= FOTO_INV_ITERS_MAX;
}

}  // namespace

hipError_t launch_plane_table(const PlaneSegs& sg, int64_t nxy, const double** table, hipStream_t s) {
    if (sg.n < 1 || sg.n > PLANE_SEGS) return hipErrorInvalidValue;
    k_plane_table<<<sg.n, NT, 0, s>>>(sg, nxy, table);
    return hipGetLastError();
}

hipError_t launch_maps(const double* const* table, int Nt, int Nx, int Ny, const double* s, int count, int inv_iters,
                       void* out, int dtype, hipStream_t st) {
    if (!maps_launch_ok(Nt, Nx, Ny, count, inv_iters)) return hipErrorInvalidValue;
    MapTimes tm;
    for (int k = 0; k < count; ++k) tm.s[k] = s[k];
    const dim3 grid = maps_grid(Nx, Ny, count);
    if (dtype == FOTO_F32) k_maps<float><<<grid, NT, 0, st>>>(table, Nt, Nx, Ny, tm, inv_iters, (float*)out);
    else if (dtype == FOTO_F64) k_maps<double><<<grid, NT, 0, st>>>(table, Nt, Nx, Ny, tm, inv_iters, (double*)out);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_interp(const double* const* table, int Nt, int Nx, int Ny, const foto_image& f0, int64_t sc0,
                         const foto_image& f1, int64_t sc1, int channels, const double* s, int count, int inv_iters,
                         void* out, int out_dtype, hipStream_t st) {
    if (!maps_launch_ok(Nt, Nx, Ny, count, inv_iters) || channels < 1) return hipErrorInvalidValue;
    MapTimes tm;
    for (int k = 0; k < count; ++k) tm.s[k] = s[k];
    const dim3 grid = maps_grid(Nx, Ny, count);
    const FrameView a = frame_view(f0, sc0), b = frame_view(f1, sc1);
    switch (out_dtype) {
        case FOTO_U8:
            k_interp<unsigned char><<<grid, NT, 0, st>>>(table, Nt, Nx, Ny, tm, inv_iters, a, b, channels,
                                                         (unsigned char*)out);
            break;
        case FOTO_F32:
            k_interp<float><<<grid, NT, 0, st>>>(table, Nt, Nx, Ny, tm, inv_iters, a, b, channels, (float*)out);
            break;
        case FOTO_F64:
            k_interp<double><<<grid, NT, 0, st>>>(table, Nt, Nx, Ny, tm, inv_iters, a, b, channels, (double*)out);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ----------------------------------------------------------------------------- argument rules

int maps_arg_check(const double* s, const void* out, int count, int inv_iters, int Nt, const char* who) {
    if (!s || !out) { set_error("%s: null pointer", who); return FOTO_ERR_ARG; }
    if (count < 1) { set_error("%s: count = %d must be >= 1", who, count); return FOTO_ERR_ARG; }
    if (inv_iters < 1 || inv_iters > FOTO_INV_ITERS_MAX) {
        set_error("%s: inv_iters = %d must be in [1, %d]", who, inv_iters, FOTO_INV_ITERS_MAX);
        return FOTO_ERR_ARG;
    }
    for (int k = 0; k < count; ++k) {
        if (!std::isfinite(s[k]) || s[k] < 0.0 || s[k] > (double)(Nt - 1)) {
            set_error("%s: s[%d] = %.17g is outside [0, Nt - 1 = %d]", who, k, s[k], Nt - 1);
            return FOTO_ERR_ARG;
        }
    }
    return 0;
}

int interp_frame_check(const foto_image* f, int channels, int64_t stride_c, int w, int h, const char* who) {
    if (!f) { set_error("%s: null pointer", who); return FOTO_ERR_ARG; }
    if (channels < 1) { set_error("%s: channels = %d must be >= 1", who, channels); return FOTO_ERR_ARG; }
    if (stride_c <= 0) {
        set_error("%s: stride_c = %lld must be > 0 (in elements)", who, (long long)stride_c);
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(image_check(f, w, h, who));
    for (int c = 1; c < channels; ++c) {   // (the alignment and the strides are those of channel 0)
        foto_image ch = *f;
        ch.data = (const char*)f->data + (size_t)c * (size_t)stride_c * dtype_bytes(f->dtype);
        FOTO_TRY(image_check(&ch, w, h, who));
    }
    return 0;
}

size_t interp_frame_bytes(const foto_image* f, int channels, int64_t stride_c, int w, int h) {
    const size_t last = (size_t)(h - 1) * (size_t)f->stride_y + (size_t)(w - 1) * (size_t)f->stride_x +
                        (size_t)(channels - 1) * (size_t)stride_c;
    return (last + 1) * dtype_bytes(f->dtype);
}

}  // namespace foto
