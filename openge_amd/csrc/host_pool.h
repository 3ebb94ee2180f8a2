// host_pool.h -- the persistent host worker pool and the huge-page vector of the host phases (realign.cpp) and of
// the FASTA loader (fasta.h).
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "uvector.h"

namespace oge {

// The first call in a process touches every page of its per-read arrays for the first time (the scratch
// keeps them for later calls): those are hvectors (uvector.h: 2 MiB pages, no serial zero fill on a
// resize -- the workers that fill them touch their pages first).
template <class T>
using BigVec = hvector<T>;

// =====================================================================================  threads
// Persistent workers (kept across calls with the run's Scratch).  run_static maps index i to worker
// i % size(); run hands indices out one at a time (prepare and decide: intervals differ in size; r03
// mapped them statically so each interval's frees stayed in its allocating thread's arena -- the
// interval objects are now reused instead of freed).
inline thread_local int tl_worker = 0;  // the Pool worker running the current job (0 = the caller)

class Pool {
public:
    explicit Pool(int threads) {
        if (threads <= 0) threads = (int)std::max(1u, std::thread::hardware_concurrency());
        n_ = threads;
        for (int t = 1; t < n_; ++t) ts_.emplace_back([this, t]() { loop(t); });
    }
    ~Pool() {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : ts_) t.join();
    }
    int size() const { return n_; }
    template <class F>
    void run_static(size_t n, F f) {
        if (n_ == 1 || n <= 1) {
            for (size_t i = 0; i < n; ++i) f(i);
            return;
        }
        exec([&](int t) {
            tl_worker = t;
            for (size_t i = (size_t)t; i < n; i += (size_t)n_) f(i);
        });
    }
    template <class F>
    void run(size_t n, F f) {  // dynamic: indices handed out one at a time
        if (n_ == 1 || n <= 1) {
            for (size_t i = 0; i < n; ++i) f(i);
            return;
        }
        std::atomic<size_t> next(0);
        exec([&](int t) {
            tl_worker = t;
            for (size_t i; (i = next.fetch_add(1)) < n;) f(i);
        });
    }
    template <class F>
    void run_chunks(size_t n, size_t chunk, F f) {  // f(begin, end) over [0, n) in chunks
        run((n + chunk - 1) / chunk, [&](size_t c) { f(c * chunk, std::min(n, (c + 1) * chunk)); });
    }
    // f(0..n) handed out in increasing order to the workers while the calling thread runs lead() beside them
    // (and then helps with what is left); one thread: f over all, then lead
    template <class F, class G>
    void run_lead(size_t n, F f, G lead) {
        if (n_ == 1) {
            for (size_t i = 0; i < n; ++i) f(i);
            lead();
            return;
        }
        std::atomic<size_t> next(0);
        exec([&](int t) {
            tl_worker = t;
            if (t == 0) lead();
            for (size_t i; (i = next.fetch_add(1)) < n;) f(i);
        });
    }

private:
    void exec(const std::function<void(int)> &job) {
        {
            std::lock_guard<std::mutex> g(m_);
            job_ = &job;
            busy_ = n_ - 1;
            gen_++;
        }
        cv_.notify_all();
        job(0);
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [&] { return busy_ == 0; });
        job_ = nullptr;
    }
    void loop(int id) {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(int)> *job;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                job = job_;
            }
            (*job)(id);
            std::lock_guard<std::mutex> g(m_);
            if (--busy_ == 0) done_.notify_one();
        }
    }
    int n_ = 1;
    std::vector<std::thread> ts_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const std::function<void(int)> *job_ = nullptr;
    int busy_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
};

}  // namespace oge
