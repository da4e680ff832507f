// host_pool.h -- a small persistent pool of std::threads: parallel_for over item blocks (librfxhost.so, host_lapack.cpp).
// Plain C++17, no other dependency: tests/host/pool_resize.cpp compiles it on its own.
#pragma once

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace rfxhost {

class Pool {
  public:
    explicit Pool(int n) { resize(n); }
    ~Pool() { stop(); }
    int size() const { return n_.load(); }
    // waits for a running parallel region to end: workers are never joined in the middle of one
    void resize(int n) {
        if (n < 1) n = 1;
        std::lock_guard<std::mutex> serial(run_mutex_);
        if (n == size()) return;
        stop_locked();
        uint64_t gen;
        {
            std::lock_guard<std::mutex> lk(m_);
            quit_ = false;
            gen = gen_;
        }
        // a worker answers only the regions that begin after it was created: it starts from the generation read here, under m_ and
        // with run_mutex_ held (read by the worker itself, a region begun before the thread got going would be missed for ever)
        for (int i = 0; i < n - 1; ++i) workers_.emplace_back([this, gen] { loop(gen); });
        n_.store(n);
    }
    // fn(begin, end) over [0, total) in blocks of `block`, dealt dynamically; the caller works too and returns when all is done
    void run(int64_t total, int64_t block, const std::function<void(int64_t, int64_t)>& fn) {
        if (total <= 0) return;
        std::lock_guard<std::mutex> serial(run_mutex_);            // one parallel region at a time
        {
            std::lock_guard<std::mutex> lk(m_);
            fn_ = &fn; total_ = total; block_ = block; next_.store(0); pending_ = (int)workers_.size(); ++gen_;
        }
        cv_.notify_all();
        work();
        std::unique_lock<std::mutex> lk(m_);
        done_cv_.wait(lk, [this] { return pending_ == 0; });
        fn_ = nullptr;
    }

  private:
    void work() {
        for (;;) {
            const int64_t b = next_.fetch_add(block_);
            if (b >= total_) break;
            (*fn_)(b, b + block_ < total_ ? b + block_ : total_);
        }
    }
    void loop(uint64_t seen) {
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return quit_ || gen_ != seen; });
                if (quit_) return;
                seen = gen_;
            }
            work();
            std::lock_guard<std::mutex> lk(m_);
            if (--pending_ == 0) done_cv_.notify_one();
        }
    }
    void stop() {
        std::lock_guard<std::mutex> serial(run_mutex_);
        stop_locked();
    }
    void stop_locked() {                                           // run_mutex_ held
        {
            std::lock_guard<std::mutex> lk(m_);
            quit_ = true;
        }
        cv_.notify_all();
        for (auto& t : workers_) t.join();
        workers_.clear();
    }
    std::vector<std::thread> workers_;
    std::mutex m_, run_mutex_;
    std::condition_variable cv_, done_cv_;
    const std::function<void(int64_t, int64_t)>* fn_ = nullptr;
    std::atomic<int64_t> next_{0};
    std::atomic<int> n_{1};
    int64_t total_ = 0, block_ = 1;
    int pending_ = 0;
    uint64_t gen_ = 0;
    bool quit_ = false;
};

}  // namespace rfxhost
