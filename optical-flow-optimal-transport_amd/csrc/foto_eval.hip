// Evaluation kernels: the backward warp utils.apply_opticalflow
// (utils.py:186-248) and the flow / intensity error metrics utils.EE / AE / IE
// (utils.py:294-354), behind the C ABI (include/foto.h).
//
// The warp is per pixel in the reference's operation order (built with -ffp-contract=off):
// bit-identical to the reference.  The metrics are two-pass masked sums (mean, then the
// squared deviations) with fixed-order tree reductions: deterministic, and equal to the
// reference's np.sum up to summation order (~1e-16 relative).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

#include "foto_devmem.h"
#include "foto_devutil.h"
#include "foto_internal.h"


namespace foto {

constexpr int EV_NT = 256;
constexpr int EV_Q = 6;   // quantities per block partial
constexpr int EV_MAX_BLOCKS = 2048;
static_assert(EV_NT == NT, "capped_blocks counts blocks of NT threads");

__global__ __launch_bounds__(EV_NT) void k_warp(const double* __restrict__ f1, const double* __restrict__ m,
                                                const double* __restrict__ u, const double* __restrict__ v, int w,
                                                int h, double* __restrict__ out) {
    const int64_t n = (int64_t)w * h;
    for (int64_t p = (int64_t)blockIdx.x * EV_NT + threadIdx.x; p < n; p += (int64_t)gridDim.x * EV_NT) {
        const int i = (int)(p / w), j = (int)(p - (p / w) * w);   // row, column
        const WarpTaps T = warp_taps(i, j, u[p], v[p], w, h);
        const int64_t q1 = T.a * w + T.b, q2 = T.a * w + T.b1, q3 = T.a1 * w + T.b1, q4 = T.a1 * w + T.b;
        out[p] = m ? warp_sum(T, 1 + m[q1], 1 + m[q2], 1 + m[q3], 1 + m[q4], f1[q1], f1[q2], f1[q3], f1[q4])
                   : warp_sum(T, f1[q1], f1[q2], f1[q3], f1[q4]);
    }
}

// pass 0: (sum EE | EE <= 50, count, sum AE | AE not NaN, count, sum (255 I - 255 IGT)^2, 0)
// pass 1: (sum (EE - mean_EE)^2 | kept, 0, sum (AE - mean_AE)^2 | kept, 0, 0, 0)
__global__ __launch_bounds__(EV_NT) void k_err_partial(int64_t n, const double* __restrict__ u,
                                                       const double* __restrict__ v, const double* __restrict__ uG,
                                                       const double* __restrict__ vG, const double* __restrict__ I,
                                                       const double* __restrict__ IG, int pass, double mee,
                                                       double mae, double* __restrict__ part) {
    __shared__ double sh[EV_Q * EV_NT];
    double acc[EV_Q] = {0, 0, 0, 0, 0, 0};
    for (int64_t p = (int64_t)blockIdx.x * EV_NT + threadIdx.x; p < n; p += (int64_t)gridDim.x * EV_NT) {
        if (u) {
            const double du = u[p] - uG[p], dv = v[p] - vG[p];
            const double e = sqrt(du * du + dv * dv);
            if (e <= 50) {
                if (pass == 0) { acc[0] += e; acc[1] += 1.0; }
                else acc[0] += (e - mee) * (e - mee);
            }
            const double a = acos((1.0 + u[p] * uG[p] + v[p] * vG[p]) /
                                  (sqrt(1.0 + u[p] * u[p] + v[p] * v[p]) * sqrt(1.0 + uG[p] * uG[p] + vG[p] * vG[p])));
            if (!isnan(a)) {
                if (pass == 0) { acc[2] += a; acc[3] += 1.0; }
                else acc[2] += (a - mae) * (a - mae);
            }
        }
        if (I && pass == 0) {
            const double d = 255 * I[p] - 255 * IG[p];
            acc[4] += d * d;
        }
    }
    block_tree_sum<EV_NT>(acc, sh);
    if (threadIdx.x < EV_Q) part[(int64_t)blockIdx.x * EV_Q + threadIdx.x] = sh[threadIdx.x * EV_NT];
}

// sum of nb block partials per quantity (one block, fixed tree)
__global__ __launch_bounds__(EV_NT) void k_err_final(int nb, const double* __restrict__ part,
                                                     double* __restrict__ tot) {
    __shared__ double sh[EV_Q * EV_NT];
    double acc[EV_Q] = {0, 0, 0, 0, 0, 0};
    for (int b = threadIdx.x; b < nb; b += EV_NT)
#pragma unroll
        for (int q = 0; q < EV_Q; ++q) acc[q] += part[(int64_t)b * EV_Q + q];
    block_tree_sum<EV_NT>(acc, sh);
    if (threadIdx.x < EV_Q) tot[threadIdx.x] = sh[threadIdx.x * EV_NT];
}

namespace {

// Device buffers of the evaluation calls: grow-only slots kept for the process (a batch worker
// evaluates every solve at one frame size; hipMalloc / hipFree per call synchronise the device
// and cost more than the kernels).  One call at a time holds them.
constexpr int EV_SLOTS = 8;
struct EvSlots {
    DevScratch buf[EV_SLOTS];
    StreamLink* link = nullptr;   // the *_dev entries: the caller's stream <-> the call's (kept, like the slots)
};
std::mutex ev_mu;
std::vector<EvSlots> ev_dev;   // per device (a slot is only valid on the device it was made on)

struct EvScope {
    std::unique_lock<std::mutex> lk{ev_mu};   // (first: unlocked after `call` has drained its stream)
    CallScope call;                           // the stream: acquired, synchronised on exit, released
    hipStream_t s = nullptr;
    EvSlots* sl = nullptr;
    int used = 0;
    bool dev_in = false;   // the *_dev entries: inputs are device arrays already, nothing to upload
    int device = -1;
    int init() {
        FOTO_TRY(call.init());
        s = call.s;
        const int dev = stream_device(s);
        if (dev < 0) {
            set_error("evaluation: stream without a device");
            return FOTO_ERR_STATE;
        }
        if ((int)ev_dev.size() <= dev) ev_dev.resize(dev + 1);
        sl = &ev_dev[dev];
        device = dev;
        return 0;
    }
    // a *_dev call (after init and the pointer checks): its inputs are used in place once the
    // caller's stream has produced them
    int init_dev(hipStream_t user) {
        dev_in = true;
        if (!sl->link) sl->link = new StreamLink();
        return sl->link->enter(user, s);
    }
    int leave(hipStream_t user) { return sl->link->leave(s, user); }
    // n doubles at p are device memory of this call's device (nullptr: an absent input)
    int check(const double* p, size_t n, const char* who, const char* what) {
        if (!p) return 0;
        if ((uintptr_t)p % sizeof(double) != 0) {
            set_error("%s: %s %p is not aligned to 8 bytes", who, what, (const void*)p);
            return FOTO_ERR_ARG;
        }
        return dev_ptr_check(p, n * sizeof(double), device, who, what);
    }
    int slot(size_t n, double** d) {
        if (used >= EV_SLOTS) {
            set_error("evaluation: out of scratch slots");
            return FOTO_ERR_STATE;
        }
        FOTO_TRY(sl->buf[used].reserve(std::max<size_t>(n, 1) * sizeof(double), s));
        *d = (double*)sl->buf[used++].p;
        return 0;
    }
    int up(const double* h, size_t n, double** d) {
        if (!h) { *d = nullptr; return 0; }
        if (dev_in) { *d = const_cast<double*>(h); return 0; }
        FOTO_TRY(slot(n, d));
        FOTO_HIP_CHECK(hipMemcpyAsync(*d, h, n * sizeof(double), hipMemcpyHostToDevice, s));
        return 0;
    }
    int dev(size_t n, double** d) { return slot(n, d); }
};

// the two passes; out: mean EE, std EE, mean AE, std AE, IE (any of the inputs may be absent)
// (on_dev: the six inputs are device arrays, used in place -- the *_dev entries)
int ev_errors(const double* u, const double* v, const double* uG, const double* vG, const double* I,
              const double* IG, int w, int h, double* out5, bool on_dev = false, hipStream_t user = nullptr,
              const char* who = "flow errors") {
    FOTO_TRY(image_size_check(w, h, 1, who));
    const int64_t n = (int64_t)w * h;
    EvScope S;
    if (on_dev) {
        FOTO_TRY(S.init());   // (the pointers are checked before anything is enqueued or waited on)
        const double* in[6] = {u, v, uG, vG, I, IG};
        static const char* const names[6] = {"u", "v", "uGT", "vGT", "I", "IGT"};
        for (int k = 0; k < 6; ++k) FOTO_TRY(S.check(in[k], (size_t)n, who, names[k]));
        FOTO_TRY(S.init_dev(user));
    } else {
        FOTO_TRY(S.init());
    }
    double *du, *dv, *duG, *dvG, *dI, *dIG, *part, *tot;
    FOTO_TRY(S.up(u, n, &du));
    FOTO_TRY(S.up(v, n, &dv));
    FOTO_TRY(S.up(uG, n, &duG));
    FOTO_TRY(S.up(vG, n, &dvG));
    FOTO_TRY(S.up(I, n, &dI));
    FOTO_TRY(S.up(IG, n, &dIG));
    const int nb = capped_blocks(n, EV_MAX_BLOCKS);
    FOTO_TRY(S.dev((size_t)nb * EV_Q, &part));
    FOTO_TRY(S.dev(EV_Q, &tot));
    double h0[EV_Q], h1[EV_Q];
    k_err_partial<<<nb, EV_NT, 0, S.s>>>(n, du, dv, duG, dvG, dI, dIG, 0, 0.0, 0.0, part);
    k_err_final<<<1, EV_NT, 0, S.s>>>(nb, part, tot);
    FOTO_HIP_CHECK(hipGetLastError());
    FOTO_HIP_CHECK(hipMemcpyAsync(h0, tot, sizeof(h0), hipMemcpyDeviceToHost, S.s));
    FOTO_HIP_CHECK(hipStreamSynchronize(S.s));
    const double mee = h0[0] / h0[1], mae = h0[2] / h0[3];
    if (du) {
        k_err_partial<<<nb, EV_NT, 0, S.s>>>(n, du, dv, duG, dvG, nullptr, nullptr, 1, mee, mae, part);
        k_err_final<<<1, EV_NT, 0, S.s>>>(nb, part, tot);
        FOTO_HIP_CHECK(hipGetLastError());
        FOTO_HIP_CHECK(hipMemcpyAsync(h1, tot, sizeof(h1), hipMemcpyDeviceToHost, S.s));
        FOTO_HIP_CHECK(hipStreamSynchronize(S.s));
        out5[0] = mee;
        out5[1] = sqrt(h1[0] / h0[1]);
        out5[2] = mae;
        out5[3] = sqrt(h1[2] / h0[3]);
    }
    if (dI) out5[4] = sqrt(h0[4] / ((double)w * h));
    if (on_dev) FOTO_TRY(S.leave(user));   // (the inputs may be overwritten by what the caller enqueues next)
    return 0;
}

}  // namespace
}  // namespace foto

using namespace foto;

extern "C" {

int foto_warp(const double* f1, const double* u, const double* v, const double* m, int w, int h, double* out) {
    if (!f1 || !u || !v || !out) {
        set_error("foto_warp: null buffer");
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(image_size_check(w, h, 1, "foto_warp"));
    const int64_t n = (int64_t)w * h;
    EvScope S;
    FOTO_TRY(S.init());
    double *df, *dm, *du, *dv, *dout;
    FOTO_TRY(S.up(f1, n, &df));
    FOTO_TRY(S.up(m, n, &dm));
    FOTO_TRY(S.up(u, n, &du));
    FOTO_TRY(S.up(v, n, &dv));
    FOTO_TRY(S.dev(n, &dout));
    k_warp<<<capped_blocks(n, EV_MAX_BLOCKS), EV_NT, 0, S.s>>>(df, dm, du, dv, w, h, dout);
    FOTO_HIP_CHECK(hipGetLastError());
    FOTO_HIP_CHECK(hipMemcpyAsync(out, dout, n * sizeof(double), hipMemcpyDeviceToHost, S.s));
    FOTO_HIP_CHECK(hipStreamSynchronize(S.s));
    return 0;
}

int foto_warp_dev(const double* f1, const double* u, const double* v, const double* m, int w, int h, double* out,
                  void* stream) {
    if (!f1 || !u || !v || !out) {
        set_error("foto_warp_dev: null buffer");
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(image_size_check(w, h, 1, "foto_warp_dev"));
    const size_t n = (size_t)w * h;
    EvScope S;
    FOTO_TRY(S.init());
    FOTO_TRY(S.check(f1, n, "foto_warp_dev", "f1"));
    FOTO_TRY(S.check(u, n, "foto_warp_dev", "u"));
    FOTO_TRY(S.check(v, n, "foto_warp_dev", "v"));
    FOTO_TRY(S.check(m, n, "foto_warp_dev", "m"));
    FOTO_TRY(S.check(out, n, "foto_warp_dev", "out"));
    if (out == f1 || out == u || out == v || out == m) {
        set_error("foto_warp_dev: out may not alias an input (the warp gathers)");
        return FOTO_ERR_ARG;
    }
    FOTO_TRY(S.init_dev((hipStream_t)stream));
    k_warp<<<capped_blocks((int64_t)n, EV_MAX_BLOCKS), EV_NT, 0, S.s>>>(f1, m, u, v, w, h, out);
    FOTO_HIP_CHECK(hipGetLastError());
    return S.leave((hipStream_t)stream);
}

int foto_flow_errors_dev(const double* u, const double* v, const double* uGT, const double* vGT, int w, int h,
                         double* out4, void* stream) {
    if (!u || !v || !uGT || !vGT || !out4) {
        set_error("foto_flow_errors_dev: null buffer");
        return FOTO_ERR_ARG;
    }
    double r[5];
    FOTO_TRY(ev_errors(u, v, uGT, vGT, nullptr, nullptr, w, h, r, true, (hipStream_t)stream, "foto_flow_errors_dev"));
    for (int k = 0; k < 4; ++k) out4[k] = r[k];
    return 0;
}

int foto_intensity_error_dev(const double* I, const double* IGT, int w, int h, double* ie, void* stream) {
    if (!I || !IGT || !ie) {
        set_error("foto_intensity_error_dev: null buffer");
        return FOTO_ERR_ARG;
    }
    double r[5];
    FOTO_TRY(ev_errors(nullptr, nullptr, nullptr, nullptr, I, IGT, w, h, r, true, (hipStream_t)stream,
                       "foto_intensity_error_dev"));
    *ie = r[4];
    return 0;
}

int foto_flow_errors(const double* u, const double* v, const double* uGT, const double* vGT, int w, int h,
                     double* out4) {
    if (!u || !v || !uGT || !vGT || !out4) {
        set_error("foto_flow_errors: null buffer");
        return FOTO_ERR_ARG;
    }
    double r[5];
    FOTO_TRY(ev_errors(u, v, uGT, vGT, nullptr, nullptr, w, h, r));
    for (int k = 0; k < 4; ++k) out4[k] = r[k];
    return 0;
}

int foto_intensity_error(const double* I, const double* IGT, int w, int h, double* ie) {
    if (!I || !IGT || !ie) {
        set_error("foto_intensity_error: null buffer");
        return FOTO_ERR_ARG;
    }
    double r[5];
    FOTO_TRY(ev_errors(nullptr, nullptr, nullptr, nullptr, I, IGT, w, h, r));
    *ie = r[4];
    return 0;
}

}  // extern "C"
