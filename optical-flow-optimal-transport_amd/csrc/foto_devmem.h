// Temporary device memory of the host layer, two owners:
//   a C-ABI call owns its resources through a CallScope;
//   a context or plan owns its blocks through a DevArena.
// (DevScratch in foto_internal.h is the third kind: one grow-only buffer kept between calls.)
#pragma once

#include "foto_internal.h"

namespace foto {

// A list of device blocks, freed together (in allocation order) by clear() or the destructor.
struct DevArena {
    std::vector<void*> blocks;
    DevArena() = default;
    DevArena(const DevArena&) = delete;
    DevArena& operator=(const DevArena&) = delete;
    int alloc(size_t bytes, void** out) {
        void* p = nullptr;
        FOTO_HIP_CHECK(hipMalloc(&p, std::max<size_t>(bytes, 1)));
        blocks.push_back(p);
        *out = p;
        return 0;
    }
    template <class T>
    int alloc_n(size_t n, T** out) {   // n elements of T
        return alloc(n * sizeof(T), (void**)out);
    }
    void clear() {
        for (void* p : blocks) (void)hipFree(p);
        blocks.clear();
    }
    ~DevArena() { clear(); }
};

// One C-ABI call's pooled stream, its device blocks and (at most) one pinned host block.  Every
// early return of the call releases them: the destructor waits for the stream (a kernel may still
// read a block), frees, and only then hands the stream back to the pool.
struct CallScope {
    hipStream_t s = nullptr;
    DevArena mem;
    void* pin = nullptr;
    int init() { return stream_acquire(&s); }
    int dev(size_t n, double** out) { return mem.alloc_n(n, out); }
    int up_to(const double* h, size_t n, double* dst) {
        FOTO_HIP_CHECK(hipMemcpyAsync(dst, h, n * sizeof(double), hipMemcpyHostToDevice, s));
        return 0;
    }
    int up(const double* h, size_t n, double** out) {
        FOTO_TRY(dev(n, out));
        return up_to(h, n, *out);
    }
    int down(double* h, const double* d, size_t n) {
        FOTO_HIP_CHECK(hipMemcpyAsync(h, d, n * sizeof(double), hipMemcpyDeviceToHost, s));
        return 0;
    }
    int sync() {
        FOTO_HIP_CHECK(hipStreamSynchronize(s));
        return 0;
    }
    int pinned(size_t bytes, void** out) {   // pinned host memory, one block per call
        if (pin) { set_error("CallScope: a second pinned block"); return FOTO_ERR_STATE; }
        FOTO_HIP_CHECK(hipHostMalloc(&pin, bytes));
        *out = pin;
        return 0;
    }
    ~CallScope() {
        if (s) (void)hipStreamSynchronize(s);
        mem.clear();
        if (pin) (void)hipHostFree(pin);
        stream_release(s);
    }
};

}  // namespace foto
