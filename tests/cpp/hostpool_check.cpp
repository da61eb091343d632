// Stand-alone check of csrc/foto_hostpool.h (HostPool, pool_memcpy), built by
// tests/test_hostpool_host.py with the host compiler under -fsanitize=thread and under
// -fsanitize=address,undefined.  Exit status 0: every check passed.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <numeric>

#include "foto_hostpool.h"

using foto::HostPool;
using foto::pool_memcpy;

static int fails = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);         \
            ++fails;                                                   \
        }                                                              \
    } while (0)

// pool_memcpy against memcpy: the bytes copied, and none written past them
static void copy_case(HostPool* pool, size_t bytes) {
    const size_t guard = 64;
    std::vector<unsigned char> src(bytes + 1), got(bytes + guard, 0xA5), want(bytes + guard, 0xA5);
    for (size_t i = 0; i < bytes; ++i) src[i] = (unsigned char)(i * 2654435761u >> 13);
    memcpy(want.data(), src.data(), bytes);
    pool_memcpy(pool, got.data(), src.data(), bytes);
    CHECK(got == want);
}

int main() {
    const size_t piece = 256 << 10;
    const size_t sizes[] = {0,                       // nothing
                            1,                       // one byte
                            piece,                   // one piece: the caller alone
                            5 * piece + 12345,       // not a multiple of the 4096-byte step
                            12u << 20};              // 12 MB
    for (int workers : {0, 1, 4}) {
        HostPool pool(workers);
        CHECK(pool.workers() == workers);
        for (size_t b : sizes) copy_case(&pool, b);
    }
    for (size_t b : sizes) copy_case(nullptr, b);   // no pool: plain memcpy
    {   // back-to-back jobs: the generation counter and the pending_ hand-off; every index runs once
        HostPool pool(4);
        std::vector<int> hits(37);
        long total = 0;
        for (int rep = 0; rep < 600; ++rep) {
            const int n = 1 + rep % 37;
            std::fill(hits.begin(), hits.end(), 0);
            pool.run(n, [&](int i) { hits[i] += 1; });
            for (int i = 0; i < 37; ++i) CHECK(hits[i] == (i < n ? 1 : 0));
            total += std::accumulate(hits.begin(), hits.end(), 0L);
        }
        CHECK(total > 0);
        pool.run(0, [&](int) { CHECK(false); });   // nothing to run
    }
    {   // pools that never ran a job
        HostPool a(4), b(0);
        (void)a;
        (void)b;
    }
    if (fails) {
        fprintf(stderr, "hostpool_check: %d failed\n", fails);
        return 1;
    }
    puts("hostpool_check ok");
    return 0;
}
