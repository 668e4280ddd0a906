// The file and thread side of the host programs, in one place: a whole file mapped read-only (MappedFile), output that
// appears under its name only when complete (AtomicFile, write_text_atomic), the entry writer over it (put_text,
// put_entries, write_entries), the host's threads (host_threads.hpp:
// SideTask, run_threads, parallel_ranges), the ZKPOA_VERBOSE phase timer, ZKPOA_DEVICE, and the device context started on a second
// thread while the first reads its input (ContextStart). Host only, no HIP: next to the public C header this is all a
// command-line front end needs. Failures are std::runtime_error.
#pragma once
#include "../../include/zkpoa_prover.h"
#include "host_threads.hpp"

#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <stdexcept>
#include <string>
#include <vector>

namespace zkpoa {

// ZKPOA_VERBOSE: where a command spends its time. One line per phase: "zkpoa: <command>: <what>  <ms since the last>"
struct PhaseTimer {
  const char* command;
  int width;   // of the <what> column (each command keeps its own: logs of different dates compare)
  const bool verbose = opt_verbose();
  struct timespec t0;
  PhaseTimer(const char* cmd, int w) : command(cmd), width(w) { clock_gettime(CLOCK_MONOTONIC, &t0); }
  void operator()(const char* what) {
    if (!verbose) return;
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    fprintf(stderr, "zkpoa: %s: %-*s %8.1f ms\n", command, width, what, (t.tv_sec - t0.tv_sec) * 1e3 + (t.tv_nsec - t0.tv_nsec) / 1e6);
    t0 = t;
  }
};

// A whole file, mapped read-only, and its descriptor (for pread and the uploader). An empty file is p == nullptr, size == 0.
struct MappedFile {
  const std::string path;
  const uint8_t* p = nullptr;
  uint64_t size = 0;
  int fd = -1;
  explicit MappedFile(const char* file) : path(file) {
    fd = open(file, O_RDONLY);
    if (fd < 0) throw std::runtime_error("cannot open " + path);
    struct stat sb;
    if (fstat(fd, &sb) != 0 || sb.st_size < 0) {
      close(fd);
      throw std::runtime_error("cannot stat " + path);
    }
    size = (uint64_t)sb.st_size;
    if (!size) return;
    void* m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (m == MAP_FAILED) {
      close(fd);
      throw std::runtime_error("cannot map " + path);
    }
    p = static_cast<const uint8_t*>(m);
  }
  ~MappedFile() {
    if (p) munmap(const_cast<uint8_t*>(p), size);
    if (fd >= 0) close(fd);
  }
  MappedFile(const MappedFile&) = delete;
  MappedFile& operator=(const MappedFile&) = delete;
  const char* begin() const { return reinterpret_cast<const char*>(p); }   // as text
  const char* end() const { return begin() + size; }
};

// Output files are written under a temporary name and renamed into place (as prover_main's write_atomic): a failure
// part-way (ENOSPC, HIP error, kill) never leaves a truncated .zkey under the final name for a later "skip if the zkey
// exists" step to pick up, and writing over the input of `zkey contribute` is safe (the mapping keeps the old inode).
struct AtomicFile {
  std::string path, tmp;
  int fd = -1;
  std::atomic<bool> ok{true};
  explicit AtomicFile(const char* final_path) : path(final_path), tmp(path + ".tmp." + std::to_string((long)getpid())) {
    fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) throw std::runtime_error("cannot create " + tmp);
  }
  // Absolute placement, for a file whose section offsets are known before their content: reserve() sizes it, put_at()
  // may then be called from several threads for disjoint ranges in any order.
  void reserve(uint64_t total) {
    if (ftruncate(fd, (off_t)total) != 0) ok = false;
  }
  // a payload of GBs is copied by several threads through a shared mapping of its final place (buffered write() calls to
  // one file queue up behind its inode lock -- measured on tmpfs: eight pwrite threads were no faster than one fwrite);
  // false without a shared mapping of this file: the caller writes the plain way
  bool mapped_copy(uint64_t off, const void* p, uint64_t len) {
    const uint64_t map_off = off & ~4095ull, lead = off - map_off;
    void* m = mmap(nullptr, lead + len, PROT_READ | PROT_WRITE, MAP_SHARED, fd, (off_t)map_off);
    if (m == MAP_FAILED) return false;
    char* dst = static_cast<char*>(m) + lead;
    parallel_ranges(len, 32ull << 20, [&](unsigned, uint64_t lo, uint64_t hi) { memcpy(dst + lo, static_cast<const char*>(p) + lo, hi - lo); });
    if (munmap(m, lead + len) != 0) ok = false;
    return true;
  }
  void put_at(uint64_t off, const void* p, uint64_t len) {
    if (len >= (64u << 20) && mapped_copy(off, p, len)) return;
    for (uint64_t done = 0; done < len;) {
      const ssize_t w = pwrite(fd, static_cast<const char*>(p) + done, len - done, (off_t)(off + done));
      if (w <= 0) {
        ok = false;
        return;
      }
      done += (uint64_t)w;
    }
  }
  void commit() {
    const bool good = (close(fd) == 0) && ok.load();
    fd = -1;
    if (!good || rename(tmp.c_str(), path.c_str()) != 0) {
      unlink(tmp.c_str());
      throw std::runtime_error("write to " + path + " failed");
    }
  }
  ~AtomicFile() {
    if (fd >= 0) {
      close(fd);
      unlink(tmp.c_str());
    }
  }
  AtomicFile(const AtomicFile&) = delete;
  AtomicFile& operator=(const AtomicFile&) = delete;
};
inline void write_text_atomic(const std::string& path, const std::string& text) {
  AtomicFile f(path.c_str());
  f.put_at(0, text.data(), text.size());
  f.commit();
}

// ---- the entry writer: a text file of many entries, formatted by the host threads and never held whole ----------------
inline void put_text(AtomicFile& fo, uint64_t& off, const std::string& s) {
  fo.put_at(off, s.data(), s.size());
  off += s.size();
}

// entry(o, i) appends entry i of n. The entries go to `off` in rounds of 2^16, each formatted by the host threads, a
// thread taking at least `least` entries and expecting `bytes_each` bytes per entry. round(i0, count) runs on the
// calling thread before the entries [i0, i0 + count) are formatted: what a round's entries read is fetched there.
constexpr uint64_t kEntryRound = 1u << 16;
template <class Round, class Fn>
void put_entries(AtomicFile& fo, uint64_t& off, uint64_t n, uint64_t least, uint64_t bytes_each, Round round, Fn entry) {
  for (uint64_t i0 = 0; i0 < n; i0 += kEntryRound) {
    const uint64_t count = std::min(kEntryRound, n - i0);
    round(i0, count);
    std::vector<std::string> parts(host_threads() + 1);
    parallel_ranges(count, least, [&](unsigned t, uint64_t lo, uint64_t hi) {
      std::string& o = parts[t];
      o.reserve((hi - lo) * bytes_each);
      for (uint64_t i = i0 + lo; i < i0 + hi; i++) entry(o, i);
    });
    for (const std::string& s : parts) put_text(fo, off, s);
  }
}
template <class Fn>
void put_entries(AtomicFile& fo, uint64_t& off, uint64_t n, uint64_t least, uint64_t bytes_each, Fn entry) {
  put_entries(fo, off, n, least, bytes_each, [](uint64_t, uint64_t) {}, entry);
}

// a whole file: head + the entries + tail, in place only when complete
template <class Fn>
void write_entries(const std::string& path, const std::string& head, const std::string& tail, uint64_t n, uint64_t bytes_each, Fn entry) {
  AtomicFile fo(path.c_str());
  uint64_t off = 0;
  put_text(fo, off, head);
  put_entries(fo, off, n, 256, bytes_each, entry);
  put_text(fo, off, tail);
  fo.commit();
}

inline int device_from_env() { return (int)opt_long(O_DEVICE); }   // ZKPOA_DEVICE, or 0

// The device context (HIP start-up, ~0.4 s) is created on a second thread while the first reads the command's input.
// get() waits for it and throws the text of a creation that failed; leaving the scope any other way joins the thread.
struct ContextStart {
  zkpoa_context* ctx = nullptr;
  char err[512] = {0};
  int rc = PROVER_OK;
  SideTask task;   // the last member: joined before the others go
  explicit ContextStart(int device) : task([this, device] { rc = zkpoa_context_create(device, &ctx, err, sizeof(err)); }) {}
  void wait() { task.wait(); }
  zkpoa_context* get() {
    task.get();
    if (rc != PROVER_OK) throw std::runtime_error(err);
    return ctx;
  }
  ContextStart(const ContextStart&) = delete;
  ContextStart& operator=(const ContextStart&) = delete;
};

}  // namespace zkpoa
