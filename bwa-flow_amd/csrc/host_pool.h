// host_pool.h — the thread pool of the host-side passes over a batch (the
// staging copy and check of bwagpu_chain2aln_submit in batch_host.h, seeding's
// validation and staging in seed_host.h).  Plain C++: compiles without HIP, so
// that the passes run under the host sanitizers (tests/cpp/batch_host_asan.cpp).
#pragma once
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace bwagpu {

// A persistent pool: creating threads per call cost 20-50 us each, and far
// more when several stage workers submit at once.  host_parallel(nt, f) runs
// f(1..nt-1) on the pool and f(0) on the caller, and returns when all are done;
// pool tasks never wait on the pool, so concurrent callers cannot deadlock.
class PassPool {
 public:
  // one pool per process: a static local of a function with external linkage
  // is the same object in every translation unit that includes this header
  static PassPool& get() {
    static PassPool p(7);
    return p;
  }
  void post(std::function<void()> f) {
    {
      std::lock_guard<std::mutex> g(mu_);
      q_.push_back(std::move(f));
    }
    cv_.notify_one();
  }
  ~PassPool() {
    {
      std::lock_guard<std::mutex> g(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }

 private:
  explicit PassPool(int n) {
    for (int i = 0; i < n; ++i) th_.emplace_back([this] { loop(); });
  }
  void loop() {
    for (;;) {
      std::function<void()> f;
      {
        std::unique_lock<std::mutex> g(mu_);
        cv_.wait(g, [this] { return stop_ || !q_.empty(); });
        if (q_.empty()) return;
        f = std::move(q_.front());
        q_.pop_front();
      }
      f();
    }
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::function<void()>> q_;
  std::vector<std::thread> th_;
  bool stop_ = false;
};

template <typename F>
void host_parallel(int nt, F f) {
  if (nt <= 1) {
    f(0);
    return;
  }
  int left = nt - 1;  // decremented under m: the caller cannot unwind before the last task released it
  std::mutex m;
  std::condition_variable done;
  for (int t = 1; t < nt; ++t)
    PassPool::get().post([&, t] {
      f(t);
      std::lock_guard<std::mutex> g(m);
      if (--left == 0) done.notify_all();
    });
  f(0);
  std::unique_lock<std::mutex> g(m);
  done.wait(g, [&] { return left == 0; });
}

}  // namespace bwagpu
