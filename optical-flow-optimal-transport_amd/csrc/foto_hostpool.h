// libfoto: a small pool of host threads for the copies between a caller's pageable arrays and
// pinned staging.  Host only (no HIP header), so it builds and runs under the host sanitizers
// on its own: tests/cpp/hostpool_check.cpp.
//
// The host side of a GN solve is two such copies: 5 MB in, 7.4 MB out at 640x480, 0.13 + 0.22 ms
// on one core against a 4.6 ms solve (FOTO_GN_TRACE).  A few workers made with the staging split
// them; the caller takes a share too.  FOTO_GN_HOST_THREADS (default 4) counts the workers; 0
// copies on the caller alone.
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace foto {

class HostPool {
public:
    explicit HostPool(int workers) {
        for (int t = 0; t < workers; ++t) th_.emplace_back([this] { loop(); });
    }
    ~HostPool() {
        {
            std::lock_guard<std::mutex> g(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    int workers() const { return (int)th_.size(); }
    // f(i) for every i < n, on the workers and the caller; returns when all have run
    void run(int n, const std::function<void(int)>& f) {
        if (th_.empty() || n <= 1) {
            for (int i = 0; i < n; ++i) f(i);
            return;
        }
        {
            std::lock_guard<std::mutex> g(mu_);
            job_ = &f;
            n_ = n;
            next_.store(0);
            pending_ = (int)th_.size();
            ++gen_;
        }
        cv_.notify_all();
        drain();
        std::unique_lock<std::mutex> g(mu_);
        done_.wait(g, [this] { return pending_ == 0; });
        job_ = nullptr;
    }

private:
    void drain() {
        for (int i; (i = next_.fetch_add(1)) < n_;) (*job_)(i);
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
            }
            drain();
            {
                std::lock_guard<std::mutex> g(mu_);
                --pending_;
            }
            done_.notify_one();
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    const std::function<void(int)>* job_ = nullptr;
    int n_ = 0, pending_ = 0;
    std::atomic<int> next_{0};
    uint64_t gen_ = 0;
    bool stop_ = false;
};

// memcpy in pieces of at least 256 KB over the pool (null: the caller alone)
inline void pool_memcpy(HostPool* pool, void* dst, const void* src, size_t bytes) {
    const size_t piece = 256 << 10;
    const int parts = pool ? (int)std::min<size_t>((size_t)pool->workers() + 1, (bytes + piece - 1) / piece) : 1;
    if (parts <= 1) {
        memcpy(dst, src, bytes);
        return;
    }
    const size_t step = ((bytes + parts - 1) / parts + 4095) & ~(size_t)4095;
    pool->run(parts, [&](int i) {
        const size_t a = (size_t)i * step;
        if (a < bytes) memcpy((char*)dst + a, (const char*)src + a, std::min(step, bytes - a));
    });
}

}  // namespace foto
