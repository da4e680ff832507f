// pool_resize.cpp -- the worker pool of librfxhost.so (csrc/host_pool.h) on its own: every index of a parallel region is visited
// exactly once, by the time run() returns, whatever the pool was resized to before or is being resized to meanwhile.
// Build: g++ -O2 -std=c++17 -pthread pool_resize.cpp (tests/test_host_pool_cpu.py); exits non-zero on any miscount.
#include "../../ransac-flow_amd/csrc/host_pool.h"

#include <atomic>
#include <cstdio>
#include <memory>
#include <thread>

using rfxhost::Pool;

namespace {

long g_bad = 0;
std::atomic<int> g_inside{0};       // the tag of the tagged region whose fn is running (second part of main)

// one parallel region over [0, total): fn bumps a counter per index; checked right after run() returns
void region(Pool& pool, int64_t total, int64_t block, const char* what, int tag = 0) {
    std::unique_ptr<std::atomic<int>[]> hits(new std::atomic<int>[total]);
    for (int64_t i = 0; i < total; ++i) hits[i].store(0, std::memory_order_relaxed);
    pool.run(total, block, [&](int64_t b, int64_t e) {
        if (tag) g_inside.store(tag);
        for (int64_t i = b; i < e; ++i) hits[i].fetch_add(1, std::memory_order_relaxed);
    });
    for (int64_t i = 0; i < total; ++i) {
        const int h = hits[i].load(std::memory_order_relaxed);
        if (h == 1) continue;
        if (g_bad++ < 10)
            std::fprintf(stderr, "%s: threads %d total %ld block %ld: index %ld visited %d times\n", what, pool.size(), (long)total,
                         (long)block, (long)i, h);
    }
}

void all_regions(Pool& pool, const char* what) {
    for (int64_t total : {1, 63, 64, 1025})
        for (int64_t block : {1, 16}) region(pool, total, block, what);
}

}  // namespace

int main() {
    // part 1: a used pool resized up and down, several regions at every size
    Pool pool(1);
    for (int threads : {1, 3, 8, 2, 8}) {
        pool.resize(threads);
        if (pool.size() != threads) { std::fprintf(stderr, "resize(%d) left %d threads\n", threads, pool.size()); return 1; }
        for (int rep = 0; rep < 3; ++rep) all_regions(pool, "sequential");
    }
    // part 2: resize() from one thread while another is inside run(), one resize per round: the resizer waits until round k's
    // region is running, the runner until round k's resize is done -- neither can starve the other, whatever the mutex's fairness
    const int rounds = 300;
    std::atomic<int> resized{0};
    std::thread resizer([&] {
        for (int k = 1; k <= rounds; ++k) {
            while (g_inside.load() != k) std::this_thread::yield();
            pool.resize(1 + (k * 3) % 8);
            resized.store(k);
        }
    });
    for (int k = 1; k <= rounds; ++k) {
        region(pool, 1025, k % 2 ? 16 : 1, "concurrent", k);
        region(pool, 64, 1, "concurrent");
        while (resized.load() != k) std::this_thread::yield();
    }
    resizer.join();
    if (g_bad) { std::fprintf(stderr, "%ld miscounted indices\n", g_bad); return 1; }
    std::printf("pool_resize OK: %d regions under %d concurrent resizes\n", 2 * rounds, resized.load());
    return 0;
}
