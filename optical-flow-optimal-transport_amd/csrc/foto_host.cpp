// libfoto host services every translation unit uses: the per-thread error message, the
// process-wide stream pool, the *_dev stream contract (StreamLink) and the size rules of a grid or
// an image.  No kernel lives here.  (Declarations: foto_internal.h.)
#include <cstdarg>
#include <mutex>
#include <utility>

#include "foto_internal.h"

namespace foto {

static thread_local char g_err[2048] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

}  // namespace foto

extern "C" const char* foto_last_error(void) { return foto::g_err; }

namespace foto {

// ----------------------------------------------------------------------------- stream pool

static std::mutex g_pool_mu;
static std::vector<std::pair<int, hipStream_t>> g_pool;   // (device, stream) free list
static std::vector<std::pair<hipStream_t, int>> g_live;   // streams handed out, with their device

// a stream of the current device; stream_release files it under the device it was created on
// (not the device current at release: a context on device 1 closed while device 0 is current)
int stream_acquire(hipStream_t* out) {
    int dev = 0;
    FOTO_HIP_CHECK(hipGetDevice(&dev));
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (size_t i = 0; i < g_pool.size(); ++i)
            if (g_pool[i].first == dev) {
                *out = g_pool[i].second;
                g_pool.erase(g_pool.begin() + i);
                g_live.push_back({*out, dev});
                return 0;
            }
    }
    FOTO_HIP_CHECK(hipStreamCreateWithFlags(out, hipStreamNonBlocking));
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_live.push_back({*out, dev});
    return 0;
}

void stream_release(hipStream_t s) {
    if (!s) return;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (size_t i = 0; i < g_live.size(); ++i)
        if (g_live[i].first == s) {
            g_pool.push_back({g_live[i].second, s});
            g_live.erase(g_live.begin() + i);
            return;
        }
}

int stream_device(hipStream_t s) {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (const auto& e : g_live)
        if (e.first == s) return e.second;
    return -1;
}

// ----------------------------------------------------------------------------- stream contract

int StreamLink::enter(hipStream_t user, hipStream_t own) {
    if (!in) FOTO_HIP_CHECK(hipEventCreateWithFlags(&in, hipEventDisableTiming));
    if (!out) FOTO_HIP_CHECK(hipEventCreateWithFlags(&out, hipEventDisableTiming));
    FOTO_HIP_CHECK(hipEventRecord(in, user));
    FOTO_HIP_CHECK(hipStreamWaitEvent(own, in, 0));
    return 0;
}

int StreamLink::leave(hipStream_t own, hipStream_t user) {
    FOTO_HIP_CHECK(hipEventRecord(out, own));
    FOTO_HIP_CHECK(hipStreamWaitEvent(user, out, 0));
    return 0;
}

StreamLink::~StreamLink() {
    if (in) (void)hipEventDestroy(in);
    if (out) (void)hipEventDestroy(out);
}

// ----------------------------------------------------------------------------- size rules

int image_size_check(int w, int h, int min_side, const char* who) {
    if (w < min_side || h < min_side) {
        set_error("%s: image %dx%d: every axis needs >= %d point%s", who, w, h, min_side, min_side == 1 ? "" : "s");
        return FOTO_ERR_ARG;
    }
    if ((int64_t)w * h >= ((int64_t)1 << 31)) {   // pixel indices are 32-bit in the kernels
        set_error("%s: image %dx%d: w h must be < 2^31", who, w, h);
        return FOTO_ERR_ARG;
    }
    return 0;
}

int grid_size_check(int Nt, int Nx, int Ny, const char* who, int min_side) {
    if (Nt < 2) {   // benamou_brenier.py:194 divides by Nt - 1; operators.py's lap1d raises IndexError
        set_error("%s: grid (Nt=%d, Nx=%d, Ny=%d): Nt needs >= 2 points", who, Nt, Nx, Ny);
        return FOTO_ERR_ARG;
    }
    return image_size_check(Nx, Ny, min_side, who);
}

}  // namespace foto
