// The host's side threads, in one place: every thread of the library and the front ends is started here, except the few
// that say at their site why not ("Who owns a side thread and what it reads"). A SideTask owns its
// thread and its callable: what the thread reads is moved into the callable, or declared before the task. Standard
// library only, no HIP.
#pragma once
#include "options.hpp"

#include <stdint.h>
#include <stdlib.h>

#include <exception>
#include <memory>
#include <system_error>
#include <thread>
#include <utility>
#include <vector>

#ifdef HOST_THREADS_CHECK_SPAWN_HOOK
bool host_threads_check_spawn_fails();   // tools/host_threads_check.cpp alone: "this start finds no thread"
#endif

namespace zkpoa {

// One thread that runs fn() and keeps what it throws. The callable lives in the thread, exactly as long as the thread.
class SideTask {
 public:
  SideTask() = default;
  template <class Fn>
  explicit SideTask(Fn fn) : err_(new std::exception_ptr) {
    thread_ = spawn([fn = std::move(fn), err = err_.get(), options = opt_overlay()]() mutable {
      opt_overlay() = std::move(options);   // the task works for the request of the thread that started it
      try {
        fn();
      } catch (...) {
        *err = std::current_exception();
      }
    });
  }
  SideTask(SideTask&&) noexcept = default;
  SideTask& operator=(SideTask&& o) noexcept {   // over a running task: that one is waited for first
    wait();
    thread_ = std::move(o.thread_);
    err_ = std::move(o.err_);
    return *this;
  }
  ~SideTask() { wait(); }   // joins; an error nobody asked for is dropped
  void wait() noexcept {
    if (thread_.joinable()) thread_.join();
  }
  std::exception_ptr error() const { return err_ ? *err_ : nullptr; }   // after wait()
  void get() {   // joins and rethrows what the callable threw, once
    wait();
    if (std::exception_ptr e = error()) {
      *err_ = nullptr;
      std::rethrow_exception(e);
    }
  }

 private:
  template <class Fn>
  static std::thread spawn(Fn&& fn) {   // every start goes through here
#ifdef HOST_THREADS_CHECK_SPAWN_HOOK
    if (host_threads_check_spawn_fails()) throw std::system_error(std::make_error_code(std::errc::resource_unavailable_try_again));
#endif
    return std::thread(std::forward<Fn>(fn));
  }
  std::thread thread_;
  std::unique_ptr<std::exception_ptr> err_;   // on the heap: the task may move while its thread runs
};

// A set of tasks. A start that fails (std::system_error) leaves the tasks started so far owned: the destructor joins them.
class SideTasks {
 public:
  template <class Fn>
  void start(Fn fn) {
    tasks_.emplace_back(std::move(fn));
  }
  void wait() noexcept {
    for (SideTask& t : tasks_) t.wait();
  }
  void get() {   // all are joined, then the first error in the order of the starts is rethrown
    wait();
    for (SideTask& t : tasks_) t.get();
  }

 private:
  std::vector<SideTask> tasks_;
};

// At the layer-three shape `zkey new` reads 62 GB and writes 35 GB, and the device's share of the command is 3.5 s: what
// was left was one host thread parsing, copying and converting (54 s in all). Every host stage is split over the host's
// threads; the arrays they fill are not zero-filled first, the threads are the first to touch them.
inline unsigned host_threads() {
  unsigned t = std::thread::hardware_concurrency();
  if (const long v = opt_long(O_SETUP_THREADS)) t = (unsigned)v;
  return t < 1 ? 1 : (t > 32 ? 32 : t);
}
// fn(t) on T threads; all are joined, then the first exception in the order of t is rethrown (a thread that cannot be
// started: those that were are joined, then the std::system_error)
template <class Fn>
void run_threads(unsigned T, Fn fn) {
  SideTasks tasks;
  for (unsigned t = 0; t < T; t++) tasks.start([&fn, t] { fn(t); });
  tasks.get();
}
// fn(t, lo, hi) over [0, count) cut into host_threads() ranges
template <class Fn>
void parallel_ranges(uint64_t count, uint64_t min_per_thread, Fn fn) {
  unsigned T = host_threads();
  if (count / (min_per_thread ? min_per_thread : 1) < T) T = (unsigned)(count / (min_per_thread ? min_per_thread : 1));
  if (T <= 1) return fn(0u, (uint64_t)0, count);
  run_threads(T, [&](unsigned t) { fn(t, count * t / T, count * (t + 1) / T); });
}

}  // namespace zkpoa
