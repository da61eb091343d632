// Flow algebra (include/foto.h, "flow algebra"): what a caller with K + 1 frames and K pair flows
// needs beyond one pair -- the composed flow frame 0 -> frame k, the backward flow of a forward
// flow, and the forward-backward cross-check with its validity mask -- on the flow buffers the
// *_dev entries leave in HBM: float32 or float64, planar or .flo-interleaved.
//
//   k_compose      one thread per pixel walks the K records in order, the running displacement
//                  (and the gain, for planar input) in registers; every record of mode `all` is
//                  stored by the same launch.
//   k_invert       one thread per (pixel, record): B <- -S(F; p + B), a fixed number of rounds.
//   k_consistency  one thread per (pixel, record): the class of the pixel, the mask, the error, and
//                  the four class counts of the record (grid_reduce_last of foto_reduce.h: integer
//                  counts in doubles, fixed order, last-block hand-off; that block writes the table).
//
// Every sample is S of foto_devutil.h (sample_taps / sample_sum): the cell and the fractions once
// per position, reused for u, v and m.  All arithmetic is float64 on values widened exactly, built
// with -ffp-contract=off like every other unit: + - * sqrt, compare, floor, min / max.  The kernels
// are gather-bound: a block is a TX x TY tile, one wave per 64-pixel row segment, so a wave's
// own-pixel loads and its stores are contiguous and its taps stay within a few rows of the segment
// (DESIGN.md 3.14 has the traffic model).  The two taps of a cell's row come with one load; a
// pixel's own interleaved (u, v) pair moves as one float2 / double2 where the buffer is aligned to
// a pair.  Every index is int64_t; every tap is inside the frame for
// every coordinate, NaN and +-inf included (sample_taps clamps), so nothing is read out of range
// whatever the flow holds.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <vector>

#include "foto_devmem.h"
#include "foto_devutil.h"
#include "foto_internal.h"
#include "foto_reduce.h"

namespace foto {

namespace {

typedef float flt2 __attribute__((ext_vector_type(2)));

struct FlowIn {
    const void* data;
    int f32, inter, vec;   // vec: interleaved and aligned to a pair
    int64_t rec;           // elements per record (0: one record, read for every record)
};
struct FlowOut {
    void* data;
    int f32, inter, vec;
    int64_t rec;
};

template <class T>
struct Pair;
template <>
struct Pair<float> { typedef flt2 type; };
template <>
struct Pair<double> { typedef dbl2 type; };

// (u, v) of element p of the record at `base`; n = w h
template <class T>
__device__ __forceinline__ void load_uv(const T* __restrict__ base, bool inter, bool vec, int64_t n, int64_t p,
                                        double& u, double& v) {
    if (!inter) {
        u = (double)base[p];
        v = (double)base[n + p];
    } else if (vec) {
        const typename Pair<T>::type q = ((const typename Pair<T>::type*)base)[p];
        u = (double)q.x;
        v = (double)q.y;
    } else {
        u = (double)base[2 * p];
        v = (double)base[2 * p + 1];
    }
}

// The two taps of a cell's row are neighbours in memory: one load for both (planar: 2 elements;
// interleaved: u0 v0 u1 v1), aligned to the element only, which gfx950's global loads take.  Half
// the load instructions of the gather (DESIGN.md 3.14 has the A/B).
template <class T>
struct Row;
template <>
struct Row<float> {
    typedef float two __attribute__((ext_vector_type(2), aligned(4)));
    typedef float four __attribute__((ext_vector_type(4), aligned(4)));
};
template <>
struct Row<double> {
    typedef double two __attribute__((ext_vector_type(2), aligned(8)));
    typedef double four __attribute__((ext_vector_type(4), aligned(8)));
};

// one plane's taps of the cell of S: f[0..3] = (j0, i0), (j0, i0 + 1), (j0 + 1, i0), (j0 + 1, i0 + 1)
template <class T>
__device__ __forceinline__ void load_plane_taps(const T* __restrict__ plane, int w, const SampleTaps& S,
                                                double (&f)[4]) {
    const T* r0 = plane + ((int64_t)S.j0 * w + S.i0);
    const typename Row<T>::two a = *(const typename Row<T>::two*)r0, b = *(const typename Row<T>::two*)(r0 + w);
    f[0] = (double)a.x;
    f[1] = (double)a.y;
    f[2] = (double)b.x;
    f[3] = (double)b.y;
}
// the (u, v) taps of the record at `base`; i0 <= w - 2 and j0 <= h - 2: every element is inside the record
template <class T>
__device__ __forceinline__ void load_taps(const T* __restrict__ base, bool inter, int64_t n, int w,
                                          const SampleTaps& S, double (&u)[4], double (&v)[4]) {
    if (!inter) {
        load_plane_taps(base, w, S, u);
        load_plane_taps(base + n, w, S, v);
    } else {
        const T* r0 = base + 2 * ((int64_t)S.j0 * w + S.i0);
        const typename Row<T>::four a = *(const typename Row<T>::four*)r0,
                                    b = *(const typename Row<T>::four*)(r0 + 2 * (int64_t)w);
        u[0] = (double)a.x, v[0] = (double)a.y, u[1] = (double)a.z, v[1] = (double)a.w;
        u[2] = (double)b.x, v[2] = (double)b.y, u[3] = (double)b.z, v[3] = (double)b.w;
    }
}
template <class T>
__device__ __forceinline__ void load_taps_m(const T* __restrict__ base, int64_t n, int w, const SampleTaps& S,
                                            double (&m)[4]) {
    load_plane_taps(base + 2 * n, w, S, m);
}

__device__ __forceinline__ double sum4(const SampleTaps& S, const double (&f)[4]) {
    return sample_sum(S, f[0], f[1], f[2], f[3]);
}

// record r of `o`, pixel p: (u, v) and, planar, m
template <class T>
__device__ __forceinline__ void store_rec_t(const FlowOut& o, int64_t r, int64_t n, int64_t p, double u, double v,
                                            double m) {
    T* base = (T*)o.data + r * o.rec;
    if (!o.inter) {
        base[p] = (T)u;
        base[n + p] = (T)v;
        base[2 * n + p] = (T)m;
    } else if (o.vec) {
        typename Pair<T>::type q;
        q.x = (T)u;
        q.y = (T)v;
        ((typename Pair<T>::type*)base)[p] = q;
    } else {
        base[2 * p] = (T)u;
        base[2 * p + 1] = (T)v;
    }
}
__device__ __forceinline__ void store_rec(const FlowOut& o, int64_t r, int64_t n, int64_t p, double u, double v,
                                          double m) {
    if (o.f32) store_rec_t<float>(o, r, n, p, u, v, m);
    else store_rec_t<double>(o, r, n, p, u, v, m);
}

// Tile t of the frame, TX x TY pixels, tiles counted along x first: this thread's pixel (i, j);
// false outside the frame.  One wave = one 64-pixel row segment.
__device__ __forceinline__ bool tile_pixel(int64_t t, int tiles_x, int w, int h, int& i, int& j) {
    const int64_t ty = t / tiles_x;
    const int tx = (int)(t - ty * tiles_x);
    i = tx * TX + (int)(threadIdx.x & (TX - 1));
    const int64_t jj = ty * TY + (int64_t)(threadIdx.x / TX);
    j = (int)jj;
    return i < w && jj < h;
}

// C_0 = F_0;  C_k = C_{k-1} + S(F_k; p + C_{k-1});  1 + M_k = (1 + M_{k-1}) (1 + S(m_k; p + C_{k-1}))
template <class T>
__global__ __launch_bounds__(NT) void k_compose(FlowIn f, int K, int w, int h, int64_t tiles, int tiles_x,
                                                int last_only, int gain, FlowOut o) {
    const int64_t n = (int64_t)w * h;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        int i, j;
        if (!tile_pixel(t, tiles_x, w, h, i, j)) continue;
        const int64_t p = (int64_t)j * w + i;
        const double x = (double)i, y = (double)j;
        const T* base = (const T*)f.data;
        double cu, cv, M = 0.0;
        load_uv(base, f.inter, f.vec, n, p, cu, cv);
        if (gain) M = (double)base[2 * n + p];
        if (!last_only || K == 1) store_rec(o, 0, n, p, cu, cv, M);
        for (int k = 1; k < K; ++k) {
            base += f.rec;
            const SampleTaps S = sample_taps(w, h, x + cu, y + cv);
            double tu[4], tv[4];
            load_taps(base, f.inter, n, w, S, tu, tv);
            if (gain) {
                double tm[4];
                load_taps_m(base, n, w, S, tm);
                M = (1.0 + M) * (1.0 + sum4(S, tm)) - 1.0;
            }
            cu = cu + sum4(S, tu);
            cv = cv + sum4(S, tv);
            if (!last_only) store_rec(o, k, n, p, cu, cv, M);
            else if (k == K - 1) store_rec(o, 0, n, p, cu, cv, M);
        }
    }
}

// B <- 0, then B <- -S(F; p + B) `iters` times; records r0 + blockIdx.y
template <class T>
__global__ __launch_bounds__(NT) void k_invert(FlowIn f, int64_t r0, int w, int h, int64_t tiles, int tiles_x,
                                               int iters, FlowOut o) {
    const int64_t n = (int64_t)w * h, r = r0 + blockIdx.y;
    const T* base = (const T*)f.data + r * f.rec;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        int i, j;
        if (!tile_pixel(t, tiles_x, w, h, i, j)) continue;
        const double x = (double)i, y = (double)j;
        double bu = 0.0, bv = 0.0;
        for (int k = 0; k < iters; ++k) {
            const SampleTaps S = sample_taps(w, h, x + bu, y + bv);
            double tu[4], tv[4];
            load_taps(base, f.inter, n, w, S, tu, tv);
            bu = -sum4(S, tu);
            bv = -sum4(S, tv);
        }
        store_rec(o, r, n, (int64_t)j * w + i, bu, bv, 0.0);
    }
}

// the class of every pixel of record r0 + blockIdx.y, valid = (class == 0), err = sqrt(e) (NaN for
// class 3), table[r][c] = the number of pixels of class c
template <class TF, class TB>
__global__ __launch_bounds__(NT) void k_consistency(FlowIn f, FlowIn b, int64_t r0, int w, int h, int64_t tiles,
                                                    int tiles_x, double alpha1, double alpha2,
                                                    unsigned char* __restrict__ valid, void* err, int err_f32,
                                                    double* partials, unsigned* tickets, double* __restrict__ table) {
    const int64_t n = (int64_t)w * h, r = r0 + blockIdx.y;
    const TF* fb = (const TF*)f.data + r * f.rec;
    const TB* bb = (const TB*)b.data + r * b.rec;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        int i, j;
        if (!tile_pixel(t, tiles_x, w, h, i, j)) continue;
        const int64_t p = (int64_t)j * w + i;
        double fu, fv;
        load_uv(fb, f.inter, f.vec, n, p, fu, fv);
        const double qx = (double)i + fu, qy = (double)j + fv;
        const SampleTaps S = sample_taps(w, h, qx, qy);
        double tu[4], tv[4];
        load_taps(bb, b.inter, n, w, S, tu, tv);
        const double bu = sum4(S, tu), bv = sum4(S, tv);
        const double du = fu + bu, dv = fv + bv;
        const double e = du * du + dv * dv;
        const double thr = alpha1 * ((fu * fu + fv * fv) + (bu * bu + bv * bv)) + alpha2;
        int c;
        if (!(isfinite(fu) && isfinite(fv) && isfinite(bu) && isfinite(bv))) c = 3;
        else if (qx < 0.0 || qx > (double)(w - 1) || qy < 0.0 || qy > (double)(h - 1)) c = 2;
        else if (e > thr) c = 1;
        else c = 0;
        valid[r * n + p] = c == 0 ? 1 : 0;
        if (err) {
            const double s = c == 3 ? qnan : sqrt(e);
            if (err_f32) ((float*)err)[r * n + p] = (float)s;
            else ((double*)err)[r * n + p] = s;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += c == q ? 1.0 : 0.0;
    }
    const RedBuf rb{partials + (int64_t)blockIdx.y * 4 * gridDim.x, tickets + blockIdx.y, 0};
    double tot[4];
    if (grid_reduce_last<4>(acc, rb, tot) && threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) table[r * 4 + q] = tot[q];
    }
}

// ----------------------------------------------------------------------------- host side

constexpr int MAX_GRID_Y = 65535;   // records per launch of k_invert / k_consistency

int chain_check(const foto_flow* a, const foto_flow* b, int w, int h, const char* who) {
    if (!a) { set_error("%s: null flow descriptor", who); return FOTO_ERR_ARG; }
    FOTO_TRY(flow_check(a, w, h, who));
    FOTO_TRY(image_size_check(w, h, 2, who));   // the bilinear cell: w, h >= 2
    if (b) {
        FOTO_TRY(flow_check(b, w, h, who));
        if (b->records != 1 && b->records != a->records) {
            set_error("%s: the backward flow has %d records: 1 (for every record) or the forward flow's %d", who,
                      b->records, a->records);
            return FOTO_ERR_ARG;
        }
    }
    return 0;
}

// a flow output: dtype F32 | F64, layout 0 | 1, non-null, aligned to its element
int flow_out_check(const void* out, int dtype, int layout, const char* who) {
    if (!out) { set_error("%s: out is null", who); return FOTO_ERR_ARG; }
    if (dtype != FOTO_F32 && dtype != FOTO_F64) {
        set_error("%s: out_dtype %d is not FOTO_F32 / FOTO_F64", who, dtype);
        return FOTO_ERR_ARG;
    }
    if (layout != 0 && layout != 1) {
        set_error("%s: out_layout %d is not 0 (planar u, v, m) / 1 (interleaved (u, v))", who, layout);
        return FOTO_ERR_ARG;
    }
    if ((uintptr_t)out % dtype_bytes(dtype) != 0) {
        set_error("%s: out %p is not aligned to its %zu-byte element", who, out, dtype_bytes(dtype));
        return FOTO_ERR_ARG;
    }
    return 0;
}

FlowIn flow_in(const foto_flow* f, int64_t n, bool broadcast) {
    const int inter = f->layout == 1;
    return FlowIn{f->data, f->dtype == FOTO_F32, inter,
                  inter && (uintptr_t)f->data % (2 * dtype_bytes(f->dtype)) == 0,
                  broadcast ? 0 : (inter ? 2 : 3) * n};
}
FlowOut flow_out(void* out, int dtype, int layout, int64_t n) {
    return FlowOut{out, dtype == FOTO_F32, layout == 1, layout == 1 && (uintptr_t)out % (2 * dtype_bytes(dtype)) == 0,
                   (layout == 1 ? 2 : 3) * n};
}

// One stream, link and scratch per device, kept for the process (ScoreDev's scheme): the calls only
// enqueue, nothing waits on the host but a scratch that has to grow.
struct ChainDev {
    hipStream_t s = nullptr;
    StreamLink link;
    DevScratch ctl;    // the tickets of k_consistency: zeroed per call
    DevScratch work;   // its partials
};
std::mutex cd_mu;
std::vector<ChainDev*> cd_dev;

int chain_dev(int* device, ChainDev** out) {
    int dev = 0;
    FOTO_HIP_CHECK(hipGetDevice(&dev));
    if ((int)cd_dev.size() <= dev) cd_dev.resize(dev + 1, nullptr);
    if (!cd_dev[dev]) {
        hipStream_t s = nullptr;
        FOTO_TRY(stream_acquire(&s));
        cd_dev[dev] = new ChainDev();
        cd_dev[dev]->s = s;
    }
    *device = dev;
    *out = cd_dev[dev];
    return 0;
}

struct Tiling {
    int tiles_x;
    int64_t tiles;
};
Tiling tiling(int w, int h) {
    const int tx = (w + TX - 1) / TX;
    return Tiling{tx, (int64_t)tx * ((h + TY - 1) / TY)};
}

}  // namespace
}  // namespace foto

using namespace foto;

extern "C" {

int foto_chain_check(const foto_flow* a, const foto_flow* b_or_null, int w, int h) {
    return chain_check(a, b_or_null, w, h, "foto_chain_check");
}

int foto_flow_compose_dev(const foto_flow* fl, int w, int h, int last_only, void* out, int out_dtype, int out_layout,
                          void* stream) {
    static const char* const who = "foto_flow_compose_dev";
    FOTO_TRY(chain_check(fl, nullptr, w, h, who));
    if (last_only != 0 && last_only != 1) { set_error("%s: last_only = %d is not 0 / 1", who, last_only); return FOTO_ERR_ARG; }
    FOTO_TRY(flow_out_check(out, out_dtype, out_layout, who));
    std::lock_guard<std::mutex> lk(cd_mu);
    int device = 0;
    ChainDev* cd = nullptr;
    FOTO_TRY(chain_dev(&device, &cd));
    const int64_t n = (int64_t)w * h;
    const size_t in_b = flow_bytes(fl, w, h);
    const size_t out_b = (size_t)(last_only ? 1 : fl->records) * (out_layout == 0 ? 3 : 2) * (size_t)n * dtype_bytes(out_dtype);
    FOTO_TRY(dev_ptr_check(fl->data, in_b, device, who, "flow data"));
    FOTO_TRY(dev_ptr_check(out, out_b, device, who, "out"));
    if (overlaps(out, out_b, fl->data, in_b)) {
        set_error("%s: out may not overlap the flow (the composition gathers)", who);
        return FOTO_ERR_ARG;
    }
    const Tiling tl = tiling(w, h);
    const unsigned bx = (unsigned)std::min<int64_t>(tl.tiles, STREAM_MAX_BLOCKS);
    const FlowIn fi = flow_in(fl, n, false);
    const FlowOut fo = flow_out(out, out_dtype, out_layout, n);
    const int gain = fl->layout == 0 && out_layout == 0;
    FOTO_TRY(cd->link.enter((hipStream_t)stream, cd->s));
    if (fi.f32) k_compose<float><<<bx, NT, 0, cd->s>>>(fi, fl->records, w, h, tl.tiles, tl.tiles_x, last_only, gain, fo);
    else k_compose<double><<<bx, NT, 0, cd->s>>>(fi, fl->records, w, h, tl.tiles, tl.tiles_x, last_only, gain, fo);
    FOTO_HIP_CHECK(hipGetLastError());
    return cd->link.leave(cd->s, (hipStream_t)stream);
}

int foto_flow_invert_dev(const foto_flow* fl, int w, int h, int iters, void* out, int out_dtype, int out_layout,
                         void* stream) {
    static const char* const who = "foto_flow_invert_dev";
    FOTO_TRY(chain_check(fl, nullptr, w, h, who));
    if (iters < 1 || iters > FOTO_INV_ITERS_MAX) {
        set_error("%s: iters = %d is outside [1, %d]", who, iters, FOTO_INV_ITERS_MAX);
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(flow_out_check(out, out_dtype, out_layout, who));
    std::lock_guard<std::mutex> lk(cd_mu);
    int device = 0;
    ChainDev* cd = nullptr;
    FOTO_TRY(chain_dev(&device, &cd));
    const int64_t n = (int64_t)w * h, R = fl->records;
    const size_t in_b = flow_bytes(fl, w, h);
    const size_t out_b = (size_t)R * (out_layout == 0 ? 3 : 2) * (size_t)n * dtype_bytes(out_dtype);
    FOTO_TRY(dev_ptr_check(fl->data, in_b, device, who, "flow data"));
    FOTO_TRY(dev_ptr_check(out, out_b, device, who, "out"));
    if (overlaps(out, out_b, fl->data, in_b)) {
        set_error("%s: out may not overlap the flow (the inversion gathers)", who);
        return FOTO_ERR_ARG;
    }
    const Tiling tl = tiling(w, h);
    const FlowIn fi = flow_in(fl, n, false);
    const FlowOut fo = flow_out(out, out_dtype, out_layout, n);
    FOTO_TRY(cd->link.enter((hipStream_t)stream, cd->s));
    for (int64_t r0 = 0; r0 < R; r0 += MAX_GRID_Y) {
        const unsigned ry = (unsigned)std::min<int64_t>(R - r0, MAX_GRID_Y);
        const unsigned bx = (unsigned)std::min<int64_t>(tl.tiles, std::max<int64_t>(64, STREAM_MAX_BLOCKS / ry));
        if (fi.f32) k_invert<float><<<dim3(bx, ry), NT, 0, cd->s>>>(fi, r0, w, h, tl.tiles, tl.tiles_x, iters, fo);
        else k_invert<double><<<dim3(bx, ry), NT, 0, cd->s>>>(fi, r0, w, h, tl.tiles, tl.tiles_x, iters, fo);
    }
    FOTO_HIP_CHECK(hipGetLastError());
    return cd->link.leave(cd->s, (hipStream_t)stream);
}

int foto_flow_consistency_dev(const foto_flow* fwd, const foto_flow* bwd, int w, int h, double alpha1, double alpha2,
                              void* valid_u8, void* err_or_null, int err_dtype, double* table, void* stream) {
    static const char* const who = "foto_flow_consistency_dev";
    if (!bwd) { set_error("%s: null flow descriptor", who); return FOTO_ERR_ARG; }
    FOTO_TRY(chain_check(fwd, bwd, w, h, who));
    if (!std::isfinite(alpha1) || alpha1 < 0.0 || !std::isfinite(alpha2) || alpha2 < 0.0) {
        set_error("%s: alpha1 = %g, alpha2 = %g: both must be finite and >= 0", who, alpha1, alpha2);
        return FOTO_ERR_ARG;
    }
    if (!valid_u8 || !table) { set_error("%s: valid and table are required", who); return FOTO_ERR_ARG; }
    if ((uintptr_t)table % sizeof(double) != 0) {
        set_error("%s: table %p is not aligned to 8 bytes", who, (const void*)table);
        return FOTO_ERR_ARG;
    }
    if (err_or_null) {
        if (err_dtype != FOTO_F32 && err_dtype != FOTO_F64) {
            set_error("%s: err_dtype %d is not FOTO_F32 / FOTO_F64", who, err_dtype);
            return FOTO_ERR_ARG;
        }
        if ((uintptr_t)err_or_null % dtype_bytes(err_dtype) != 0) {
            set_error("%s: err %p is not aligned to its %zu-byte element", who, err_or_null, dtype_bytes(err_dtype));
            return FOTO_ERR_ARG;
        }
    }
    std::lock_guard<std::mutex> lk(cd_mu);
    int device = 0;
    ChainDev* cd = nullptr;
    FOTO_TRY(chain_dev(&device, &cd));
    const int64_t n = (int64_t)w * h, R = fwd->records;
    const size_t f_b = flow_bytes(fwd, w, h), b_b = flow_bytes(bwd, w, h);
    const size_t v_b = (size_t)R * (size_t)n, t_b = (size_t)R * 4 * sizeof(double);
    const size_t e_b = err_or_null ? (size_t)R * (size_t)n * dtype_bytes(err_dtype) : 0;
    FOTO_TRY(dev_ptr_check(fwd->data, f_b, device, who, "forward flow data"));
    FOTO_TRY(dev_ptr_check(bwd->data, b_b, device, who, "backward flow data"));
    FOTO_TRY(dev_ptr_check(valid_u8, v_b, device, who, "valid"));
    if (err_or_null) FOTO_TRY(dev_ptr_check(err_or_null, e_b, device, who, "err"));
    FOTO_TRY(dev_ptr_check(table, t_b, device, who, "table"));
    const void* outs[3] = {valid_u8, table, err_or_null};
    const size_t outs_b[3] = {v_b, t_b, e_b};
    for (int k = 0; k < 3; ++k) {
        if (!outs[k]) continue;
        if (overlaps(outs[k], outs_b[k], fwd->data, f_b) || overlaps(outs[k], outs_b[k], bwd->data, b_b)) {
            set_error("%s: valid, err and table may not overlap the flows (the cross-check gathers)", who);
            return FOTO_ERR_ARG;
        }
        for (int q = 0; q < k; ++q)
            if (overlaps(outs[k], outs_b[k], outs[q], outs_b[q])) {
                set_error("%s: valid, err and table may not overlap each other", who);
                return FOTO_ERR_ARG;
            }
    }
    hipStream_t s = cd->s;
    const Tiling tl = tiling(w, h);
    const int64_t ry_max = std::min<int64_t>(R, MAX_GRID_Y);
    // blocks per record as the scorer's: every block ends with one returning atomic on its record's ticket
    const unsigned bx = (unsigned)std::min<int64_t>(tl.tiles, std::max<int64_t>(8, 2048 / ry_max));
    const size_t ctl_bytes = (size_t)ry_max * sizeof(unsigned);
    FOTO_TRY(cd->ctl.reserve(ctl_bytes, s));
    FOTO_TRY(cd->work.reserve((size_t)ry_max * 4 * bx * sizeof(double), s));
    const FlowIn ff = flow_in(fwd, n, false), fb = flow_in(bwd, n, bwd->records == 1 && R > 1);
    FOTO_TRY(cd->link.enter((hipStream_t)stream, s));
    FOTO_HIP_CHECK(hipMemsetAsync(cd->ctl.p, 0, ctl_bytes, s));
    for (int64_t r0 = 0; r0 < R; r0 += MAX_GRID_Y) {
        const dim3 g(bx, (unsigned)std::min<int64_t>(R - r0, MAX_GRID_Y));
#define FOTO_CONS(TF, TB)                                                                                         \
    k_consistency<TF, TB><<<g, NT, 0, s>>>(ff, fb, r0, w, h, tl.tiles, tl.tiles_x, alpha1, alpha2,               \
                                           (unsigned char*)valid_u8, err_or_null, err_dtype == FOTO_F32,         \
                                           (double*)cd->work.p, (unsigned*)cd->ctl.p, table)
        if (ff.f32 && fb.f32) FOTO_CONS(float, float);
        else if (ff.f32) FOTO_CONS(float, double);
        else if (fb.f32) FOTO_CONS(double, float);
        else FOTO_CONS(double, double);
#undef FOTO_CONS
    }
    FOTO_HIP_CHECK(hipGetLastError());
    return cd->link.leave(s, (hipStream_t)stream);
}

}  // extern "C"
