// Stream ceiling probes (foto_stream_probe, foto_stream_probe4): memory traffic of the dominant
// kernels alone, for bench.py's roofline figures.  Not part of the solver.
#include <algorithm>

#include "foto_devmem.h"
#include "foto_devutil.h"
#include "foto_internal.h"

// ============================================================================ C ABI: stream ceiling probe
// The s-step pass's memory traffic alone -- read r, q (16 B per lane), write r, q -- with no
// moments, no plan and no reduction: what the dominant kernel could reach on this device.
// bench.py reports the pass against it (roofline.stream_frac) beside the HBM-peak fraction,
// because the pass's 157 MB working set sits in the 256 MiB Infinity Cache.

namespace foto {
__global__ __launch_bounds__(256) void k_stream_fill(double* __restrict__ r, double* __restrict__ q, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        r[i] = 1e-3 * (double)((i * 2654435761u) % 1000) - 0.5;
        q[i] = 1e-3 * (double)((i * 40503u + 7) % 1000) - 0.5;
    }
}

template <bool WT>
__global__ __launch_bounds__(256) void k_stream_rq(double* __restrict__ r, double* __restrict__ q, int64_t n2,
                                                   double a, double b) {
    const __amdgpu_buffer_rsrc_t rr = wt_rsrc(r), rq = wt_rsrc(q);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (int64_t)gridDim.x * 256) {
        const dbl2 rv = reinterpret_cast<const dbl2*>(r)[i], qv = reinterpret_cast<const dbl2*>(q)[i];
        const dbl2 pn = b * qv + rv, rn = rv - a * pn;
        if (WT) {
            st_wt16(rr, (int)(i * 16), rn);
            st_wt16(rq, (int)(i * 16), pn);
        } else {
            reinterpret_cast<dbl2*>(r)[i] = rn;
            reinterpret_cast<dbl2*>(q)[i] = pn;
        }
    }
}
// the prox + RHS traffic: 4 fields in, 4 out, 16 B per lane per field (ping-pong between the
// two sets of four so every launch streams from HBM)
__global__ __launch_bounds__(256) void k_stream_4x4(const double* __restrict__ a0, const double* __restrict__ a1,
                                                    const double* __restrict__ a2, const double* __restrict__ a3,
                                                    double* __restrict__ b0, double* __restrict__ b1,
                                                    double* __restrict__ b2, double* __restrict__ b3, int64_t n2, double c) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (int64_t)gridDim.x * 256) {
        const dbl2 x0 = reinterpret_cast<const dbl2*>(a0)[i], x1 = reinterpret_cast<const dbl2*>(a1)[i];
        const dbl2 x2 = reinterpret_cast<const dbl2*>(a2)[i], x3 = reinterpret_cast<const dbl2*>(a3)[i];
        reinterpret_cast<dbl2*>(b0)[i] = x1 + c * x0;
        reinterpret_cast<dbl2*>(b1)[i] = x2 + c * x0;
        reinterpret_cast<dbl2*>(b2)[i] = x3 + c * x0;
        reinterpret_cast<dbl2*>(b3)[i] = x0 - c * (x1 + x2);
    }
}
}  // namespace foto

namespace foto {
struct EventPair {   // a probe's two timing events
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int init() {
        FOTO_HIP_CHECK(hipEventCreate(&e0));
        FOTO_HIP_CHECK(hipEventCreate(&e1));
        return 0;
    }
    ~EventPair() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};
}  // namespace foto

extern "C" int foto_stream_probe4(int64_t n, int reps, double* us) {
    using namespace foto;
    if (!us || n < 2 || n % 2 || reps < 1) {
        set_error("foto_stream_probe4: bad arguments (n even)");
        return FOTO_ERR_ARG;
    }
    EventPair ev;   // (declared first: released after the scope has drained the stream)
    CallScope S;
    FOTO_TRY(S.init());
    hipStream_t s = S.s;
    double* f[8] = {nullptr};
    for (int i = 0; i < 8; ++i) FOTO_TRY(S.dev((size_t)n, &f[i]));
    for (int i = 0; i < 8; i += 2) k_stream_fill<<<1024, 256, 0, s>>>(f[i], f[i + 1], n);   // non-zero data
    FOTO_HIP_CHECK(hipGetLastError());
    FOTO_TRY(ev.init());
    const int nb = 4 * cus_count();
    float best = 1e30f;
    for (int rep = 0; rep < 3; ++rep) {
        FOTO_HIP_CHECK(hipEventRecord(ev.e0, s));
        for (int k = 0; k < reps; ++k) {
            double** A = (k & 1) ? f + 4 : f;
            double** B = (k & 1) ? f : f + 4;
            k_stream_4x4<<<nb, 256, 0, s>>>(A[0], A[1], A[2], A[3], B[0], B[1], B[2], B[3], n / 2, 1e-9);
        }
        FOTO_HIP_CHECK(hipGetLastError());
        FOTO_HIP_CHECK(hipEventRecord(ev.e1, s));
        FOTO_HIP_CHECK(hipEventSynchronize(ev.e1));
        float t = 0.f;
        FOTO_HIP_CHECK(hipEventElapsedTime(&t, ev.e0, ev.e1));
        best = std::min(best, t);
    }
    us[0] = 1e3 * best / reps;
    return 0;
}

extern "C" int foto_stream_probe(int64_t n, int reps, double* us) {
    using namespace foto;
    if (!us || n < 2 || n % 2 || reps < 1 || n * 8 >= (int64_t(1) << 31)) {
        set_error("foto_stream_probe: bad arguments (n even, n * 8 < 2^31)");
        return FOTO_ERR_ARG;
    }
    EventPair ev;   // (declared first: released after the scope has drained the stream)
    CallScope S;
    FOTO_TRY(S.init());
    hipStream_t s = S.s;
    double *r = nullptr, *q = nullptr;
    FOTO_TRY(S.dev((size_t)n, &r));
    FOTO_TRY(S.dev((size_t)n, &q));
    // non-zero data: zero-filled buffers let the chip hold a higher clock (MI355X_MICROARCH.md,
    // DVFS give-back) and read 15-20 % faster than the solver's vectors do
    k_stream_fill<<<1024, 256, 0, s>>>(r, q, n);
    FOTO_HIP_CHECK(hipGetLastError());
    FOTO_TRY(ev.init());
    for (int wt = 0; wt < 2; ++wt) {
        float best = 1e30f;
        for (int rep = 0; rep < 3; ++rep) {
            FOTO_HIP_CHECK(hipEventRecord(ev.e0, s));
            for (int k = 0; k < reps; ++k) {
                if (wt) k_stream_rq<true><<<1024, 256, 0, s>>>(r, q, n / 2, 1e-9, 1e-9);
                else k_stream_rq<false><<<1024, 256, 0, s>>>(r, q, n / 2, 1e-9, 1e-9);
            }
            FOTO_HIP_CHECK(hipGetLastError());
            FOTO_HIP_CHECK(hipEventRecord(ev.e1, s));
            FOTO_HIP_CHECK(hipEventSynchronize(ev.e1));
            float t = 0.f;
            FOTO_HIP_CHECK(hipEventElapsedTime(&t, ev.e0, ev.e1));
            best = std::min(best, t);
        }
        us[wt] = 1e3 * best / reps;
    }
    return 0;
}
