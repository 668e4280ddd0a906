// Host check of csrc/host_threads.hpp: the header's own text, compiled by g++ alone.
// Build: g++ -O2 -std=c++17 -pthread -DHOST_THREADS_CHECK_SPAWN_HOOK -I zk-proof-of-assets_amd/csrc
//            tools/host_threads_check.cpp -o host_threads_check
// Use:   host_threads_check CASE [ARGS]     (tests/test_host_threads.py drives it)
// Every case prints one line and exits 0; a case that finds the header wrong prints "FAILED: <what>" instead.
// Sanitizer builds of the same program (no GPU, never on a GPU machine):
//   HOST_THREADS_CHECK_FLAGS="-O1 -g -fsanitize=address,undefined" python -m pytest tests/test_host_threads.py
//   HOST_THREADS_CHECK_FLAGS="-O1 -g -fsanitize=thread" python -m pytest tests/test_host_threads.py
//   visit T                  run_threads(T): "visited T: each index once"
//   first-error              8 threads, 2 and 5 throw: "caught 2 with 8 bodies finished"
//   ranges COUNT MIN         parallel_ranges(COUNT, MIN) under the caller's ZKPOA_SETUP_THREADS: "covered COUNT in K ranges"
//   get-once                 SideTask::get(): "boom once, then quiet"
//   destructor               "flag seen after the scope"
//   move-assign              "old task done when the assignment returned"
//   zkey-new                 the shape of `zkey new`: a writer that owns a moved-in 64 MiB buffer, a scope that throws, the
//                            writer let go only once the unwinding has begun: "sum S"
//   spawn-fail run|tasks     the 3rd start of 6 finds no thread: "system_error, 2 bodies ran"
#include "host_threads.hpp"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <type_traits>

using namespace zkpoa;

static_assert(!std::is_copy_constructible<SideTask>::value && !std::is_copy_assignable<SideTask>::value, "SideTask is not copyable");
static_assert(std::is_nothrow_move_constructible<SideTask>::value && std::is_nothrow_move_assignable<SideTask>::value, "SideTask moves");

static int g_starts = 0, g_fail_at = 0;   // the g_fail_at-th start from now fails (0: none)
bool host_threads_check_spawn_fails() { return ++g_starts == g_fail_at; }

static int fail(const std::string& what) {
  printf("FAILED: %s\n", what.c_str());
  return 0;   // the line says it; a status other than 0 is left to mean that the program died
}
static void nap() { std::this_thread::sleep_for(std::chrono::milliseconds(50)); }

struct Latch {
  std::mutex m;
  std::condition_variable cv;
  bool open = false;
  void release() {
    {
      std::lock_guard<std::mutex> lk(m);
      open = true;
    }
    cv.notify_all();
  }
  void wait() {
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [&] { return open; });
  }
};

static int visit(unsigned T) {
  std::vector<std::atomic<int>> seen(T);
  run_threads(T, [&](unsigned t) { seen[t]++; });
  for (unsigned t = 0; t < T; t++)
    if (seen[t] != 1) return fail("index " + std::to_string(t) + " visited " + std::to_string(seen[t].load()) + " times");
  printf("visited %u: each index once\n", T);
  return 0;
}

static int first_error() {
  std::atomic<int> finished{0};
  try {
    run_threads(8, [&](unsigned t) {
      if (t == 2) nap();   // the later thrower is very likely the first in time
      finished++;
      if (t == 2 || t == 5) throw std::runtime_error(std::to_string(t));
    });
  } catch (const std::runtime_error& e) {
    printf("caught %s with %d bodies finished\n", e.what(), finished.load());
    return 0;
  }
  return fail("nothing was thrown");
}

static int ranges(uint64_t count, uint64_t min_per_thread) {
  std::mutex m;
  std::vector<std::pair<uint64_t, uint64_t>> got;
  parallel_ranges(count, min_per_thread, [&](unsigned, uint64_t lo, uint64_t hi) {
    std::lock_guard<std::mutex> lk(m);
    got.emplace_back(lo, hi);
  });
  std::sort(got.begin(), got.end());
  uint64_t at = 0;
  for (auto& r : got) {
    if (r.first != at || r.second < r.first) return fail("a range begins at " + std::to_string(r.first) + ", not at " + std::to_string(at));
    at = r.second;
  }
  if (at != count) return fail("the ranges end at " + std::to_string(at));
  printf("covered %llu in %zu ranges\n", (unsigned long long)count, got.size());
  return 0;
}

static int get_once() {
  SideTask t([] { throw std::runtime_error("boom"); });
  t.wait();
  if (!t.error()) return fail("error() is empty after wait()");
  std::string first;
  try {
    t.get();
  } catch (const std::runtime_error& e) {
    first = e.what();
  }
  t.get();   // quiet
  if (t.error()) return fail("the error is still kept after get()");
  SideTask good([] {});
  good.get();
  printf("%s once, then quiet\n", first.c_str());
  return 0;
}

static int destructor() {
  std::atomic<bool> flag{false};
  {
    SideTask t([&] {
      nap();
      flag = true;
    });
  }
  if (!flag) return fail("the scope was left before the task had finished");
  printf("flag seen after the scope\n");
  return 0;
}

static int move_assign() {
  std::atomic<bool> old_done{false}, new_done{false};
  SideTask t([&] {
    nap();
    old_done = true;
  });
  t = SideTask([&] { new_done = true; });
  if (!old_done) return fail("the assignment returned while the old task was running");
  SideTask u(std::move(t));   // the new task has moved twice by now
  u.get();
  if (!new_done) return fail("the new task was lost");
  printf("old task done when the assignment returned\n");
  return 0;
}

// `zkey new`: a point section comes back from the device, moves into its writer, and a later device stage throws. The
// writer is held back until the scope is being unwound. (The releasing object is declared AFTER the task: destructors
// run in reverse, so it lets the writer go before the task's destructor joins it -- declared before the task, it would
// run after that join and the two would wait for each other. A buffer that were a local of the scope declared after the
// task, as the sections once were, would be freed at this very point.)
static int zkey_new() {
  const size_t bytes = 64u << 20;   // free() unmaps a block of this size: reading it afterwards is a crash
  std::atomic<unsigned long long> sum{0};
  Latch latch;
  try {
    std::unique_ptr<char[]> section(new char[bytes]);
    for (size_t i = 0; i < bytes; i++) section[i] = (char)(i & 0xff);
    SideTasks writers;
    writers.start([&, sec = std::move(section)] {
      latch.wait();
      unsigned long long s = 0;
      for (size_t i = 0; i < bytes; i++) s += (unsigned char)sec[i];
      sum = s;
    });
    struct Release {
      Latch& l;
      ~Release() { l.release(); }
    } release{latch};
    if (section) return fail("the section was not moved");
    throw std::runtime_error("the device stage failed");
  } catch (const std::runtime_error&) {
  }
  printf("sum %llu\n", sum.load());
  return 0;
}

static int spawn_fail(const char* how) {
  std::atomic<int> ran{0};
  auto body = [&] {
    nap();   // still running when the failing start comes
    ran++;
  };
  g_starts = 0;
  g_fail_at = 3;
  try {
    if (!strcmp(how, "run")) {
      run_threads(6, [&](unsigned) { body(); });
    } else {
      SideTasks tasks;
      for (int i = 0; i < 6; i++) tasks.start(body);
      tasks.get();
    }
  } catch (const std::system_error&) {
    g_fail_at = 0;
    printf("system_error, %d bodies ran\n", ran.load());
    return 0;
  }
  return fail("no std::system_error");
}

int main(int argc, char** argv) {
  const std::string op = argc > 1 ? argv[1] : "";
  if (op == "visit" && argc == 3) return visit((unsigned)strtoul(argv[2], nullptr, 10));
  if (op == "first-error") return first_error();
  if (op == "ranges" && argc == 4) return ranges(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10));
  if (op == "get-once") return get_once();
  if (op == "destructor") return destructor();
  if (op == "move-assign") return move_assign();
  if (op == "zkey-new") return zkey_new();
  if (op == "spawn-fail" && argc == 3) return spawn_fail(argv[2]);
  fprintf(stderr, "usage: host_threads_check CASE [ARGS]\n");
  return 2;
}
