// Host -> HBM upload of large pageable buffers (an mmap'd .zkey: 1 GB for layer one, 21 GB for layer
// three). A plain hipMemcpy from pageable memory stages through one internal buffer
// (~4 GB/s measured); here T host threads each own a slice of the transfer, copy it chunk-wise into
// their own pinned double buffer and issue hipMemcpyAsync on their own stream, so page-cache reads,
// staging copies and PCIe DMA all overlap.
#pragma once
#include "device_ctx.hpp"
#include "host_threads.hpp"

#include <ctype.h>
#include <pthread.h>
#include <sched.h>
#include <string.h>
#include <unistd.h>

#include <atomic>
#include <mutex>
#include <thread>
#include <vector>

namespace zkpoa {

class FastUploader {
 public:
  static constexpr int kMaxThreads = 16;
  // 2 MiB per buffer, two per thread: large enough for full-rate DMA, and pinning the staging memory is a
  // start-up cost that a one-shot prover pays every time (12 x 8 MiB cost ~60 ms, 12 x 2 MiB ~15 ms)
  static constexpr size_t kChunk = 2u << 20;

  // `stream`: an existing stream of the caller that is idle during the upload (the context's lane 0). Creating
  // a HIP stream costs 10-50 ms (it brings up a hardware queue), which a one-shot prover pays on every run, so
  // the uploader owns none by default: the copies of all threads interleave on the one stream at full PCIe rate.
  // fd >= 0: the bytes are read with pread(fd, file_off + ...) straight into the pinned buffers instead of being
  // copied out of `src` (a fresh mmap of a page-cached 1 GB file costs a page fault per 64 KiB on top of the copy:
  // ~10 GB/s; pread from the page cache runs at memcpy speed and skips the second copy); `src` may then be null.
  void upload(void* dst, const void* src, size_t bytes, int device, hipStream_t stream, int fd = -1, uint64_t file_off = 0) {
    if (bytes < (4u << 20)) {  // small: not worth the threads
      std::vector<char> tmp;
      if (fd >= 0) {
        tmp.resize(bytes);
        read_all(fd, tmp.data(), bytes, file_off);
        src = tmp.data();
      }
      ZK_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
      return;
    }
    ensure(device, stream);
    const size_t per = ((bytes / threads_) + 4095) & ~size_t(4095);
    unsigned used = 0;   // the non-empty slices
    while ((int)used < threads_ && used * per < bytes) used++;
    run_threads(used, [&, this](unsigned t) {
      const size_t lo = t * per, hi = lo + per < bytes ? lo + per : bytes;
      ZK_HIP(hipSetDevice(device));
      if (have_cpus_) (void)pthread_setaffinity_np(pthread_self(), sizeof(cpus_), &cpus_);
      Slot& s = slots_[t];
      // streams: the caller's plus the uploader's own, as many as exist by now (they come up in the background);
      // one stream -- one SDMA queue -- moves ~36 GB/s whatever the thread count, four reach the link's ~53 GB/s
      const int ns = n_own_.load(std::memory_order_acquire);
      const int pick = (int)t % (ns + 1);
      hipStream_t st = pick == ns ? stream : own_[pick].s;
      int b = 0;
      for (size_t off = lo; off < hi; off += kChunk, b ^= 1) {
        size_t len = hi - off < kChunk ? hi - off : kChunk;
        ZK_HIP(hipEventSynchronize(s.done[b]));  // the DMA that last used this buffer has finished
        if (fd >= 0) read_all(fd, static_cast<char*>(s.pinned[b]), len, file_off + off);
        else memcpy(s.pinned[b], reinterpret_cast<const char*>(src) + off, len);
        ZK_HIP(hipMemcpyAsync(reinterpret_cast<char*>(dst) + off, s.pinned[b], len, hipMemcpyHostToDevice, st));
        ZK_HIP(hipEventRecord(s.done[b], st));
      }
      for (int k = 0; k < 2; k++) ZK_HIP(hipEventSynchronize(s.done[k]));
    });
  }

  // Streams of the uploader's own (ZKPOA_UPLOAD_STREAMS, default 3: four with the caller's). Called from the context's
  // background thread AFTER the lanes are up: a stream costs 10-50 ms to create, so a one-shot prover's first upload
  // (the witness) starts on the caller's stream alone and later sections find more streams as they appear.
  // Their priority is HIGH: on this runtime a host -> device copy is queued like a kernel, and at normal priority it
  // waits behind the lanes' kernels -- measured on an MI355X (tools/upload_bench.py, 8 GB from the page cache, four lanes
  // running 2^22-point MSMs): 3 GB/s on three normal-priority streams, 12 GB/s on one, 34 GB/s on one high-priority
  // stream (47 GB/s with the chip idle), 40 GB/s on three with GPU_MAX_HW_QUEUES=16 (which the `prover` executable sets
  // for its own process: with the default of 4 hardware queues the eleven streams of a context share queues, and a
  // copy then sits behind a kernel of the lane it shares with). Default: 1 own stream, 3 when GPU_MAX_HW_QUEUES >= 8.
  void add_streams(int device) {
    int want = (int)opt_long(O_UPLOAD_STREAMS);
    static_assert(kMaxOwnStreams == 8, "the range of ZKPOA_UPLOAD_STREAMS");
    if (want < 0) {
      const char* q = getenv("GPU_MAX_HW_QUEUES");
      want = q && atoi(q) >= 8 ? 3 : 1;
    }
    for (int i = n_own_.load(); i < want; i++) {
      if (hipSetDevice(device) != hipSuccess) return;
      int lo = 0, hi = 0;   // numerically lower = higher priority
      (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
      const int word = opt_choice(O_UPLOAD_STREAM_PRIO);   // high | normal | low
      const int prio = word == 1 ? (lo + hi) / 2 : word == 2 ? lo : hi;
      if (own_[i].try_create(prio) != hipSuccess) {
        (void)hipGetLastError();
        return;
      }
      n_own_.store(i + 1, std::memory_order_release);   // published once it exists
    }
  }

  // pin the staging buffers ahead of the first upload (a one-shot prover: on the context's background thread)
  void prepare(int device, hipStream_t stream) {
    std::lock_guard<std::mutex> lk(ensure_mutex_);
    ensure_locked(device, stream);
  }

 private:
  struct Slot {
    void* pinned[2] = {nullptr, nullptr};   // into block_
    DevEvent done[2];
  };
  Slot slots_[kMaxThreads];
  PinnedMem block_;
  bool ready_ = false;   // block_ and every slot of threads_ are in place
  int threads_ = 8;
  cpu_set_t cpus_;            // the CPUs of the GPU's NUMA node (staging copies stay on its socket)
  bool have_cpus_ = false;
  static constexpr int kMaxOwnStreams = 8;
  DevStream own_[kMaxOwnStreams];
  std::atomic<int> n_own_{0};

  static void read_all(int fd, char* out, size_t len, uint64_t pos) {
    size_t got = 0;
    while (got < len) {
      ssize_t r = pread(fd, out + got, len - got, (off_t)(pos + got));
      if (r <= 0) throw HipError("upload: short read from the file");
      got += (size_t)r;
    }
  }

  // CPUs of the NUMA node the GPU hangs off (sysfs: the PCI device's numa_node, that node's cpulist); false when unknown
  static bool gpu_node_cpus(int device, cpu_set_t* out) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof(bus), device) != hipSuccess) return false;
    for (char* c = bus; *c; c++) *c = (char)tolower(*c);
    char path[256];
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE* f = fopen(path, "r");
    int node = -1;
    if (!f || fscanf(f, "%d", &node) != 1) node = -1;
    if (f) fclose(f);
    if (node < 0) return false;
    snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
    f = fopen(path, "r");
    if (!f) return false;
    CPU_ZERO(out);
    int a = 0, b = 0, n = 0;
    char sep = 0;
    while (fscanf(f, "%d", &a) == 1) {
      b = a;
      int ch = fgetc(f);
      if (ch == '-') {
        if (fscanf(f, "%d", &b) != 1) break;
        ch = fgetc(f);
      }
      for (int c = a; c <= b && c < CPU_SETSIZE; c++) {
        CPU_SET(c, out);
        n++;
      }
      sep = (char)ch;
      if (sep != ',') break;
    }
    fclose(f);
    // only CPUs this process may use at all
    cpu_set_t allowed;
    if (sched_getaffinity(0, sizeof(allowed), &allowed) == 0) {
      CPU_AND(out, out, &allowed);
      n = CPU_COUNT(out);
    }
    return n > 0;
  }

  std::mutex ensure_mutex_;
  void ensure(int device, hipStream_t stream) {
    std::lock_guard<std::mutex> lk(ensure_mutex_);
    ensure_locked(device, stream);
  }
  void ensure_locked(int device, hipStream_t stream) {
    if (ready_) return;
    // Threads: each copies its slice through its own pair of pinned buffers. Measured on an MI355X box (r04,
    // tools/file_inclusive.py): see DESIGN.md section 7 for the rates; ZKPOA_UPLOAD_THREADS overrides (1..16).
    static_assert(kMaxThreads == 16, "the range of ZKPOA_UPLOAD_THREADS");
    threads_ = (int)opt_long(O_UPLOAD_THREADS);
    unsigned hw = std::thread::hardware_concurrency();
    if (hw && (int)hw < threads_) threads_ = (int)hw;
    ZK_HIP(hipSetDevice(device));
    // the staging threads (and the first touch of their pinned buffers) stay on the CPUs of the GPU's NUMA node: 51 vs
    // 47 GB/s on a two-socket box (ZKPOA_UPLOAD_AFFINITY=off: wherever the scheduler puts them)
    if (opt_choice(O_UPLOAD_AFFINITY) == 0) have_cpus_ = gpu_node_cpus(device, &cpus_);   // gpu | off
    cpu_set_t before;
    const bool moved = have_cpus_ && pthread_getaffinity_np(pthread_self(), sizeof(before), &before) == 0 &&
                       pthread_setaffinity_np(pthread_self(), sizeof(cpus_), &cpus_) == 0;
    // built aside and moved in whole: a failure half-way leaves nothing behind, and the next call starts afresh
    PinnedMem block;
    {
      struct Restore {   // the calling thread goes back to its own CPUs, also when the pinning fails
        const cpu_set_t* to;
        ~Restore() {
          if (to) (void)pthread_setaffinity_np(pthread_self(), sizeof(*to), to);
        }
      } restore{moved ? &before : nullptr};
      block.alloc((size_t)threads_ * 2 * kChunk);         // one pinning call
      if (moved) memset(block.get(), 0, block.bytes());   // first touch on the GPU's node
    }
    DevEvent done[kMaxThreads][2];
    for (int t = 0; t < threads_; t++) {
      for (int b = 0; b < 2; b++) {
        done[t][b].create(hipEventDefault);
        ZK_HIP(hipEventRecord(done[t][b], stream));
      }
    }
    for (int t = 0; t < threads_; t++) {
      for (int b = 0; b < 2; b++) {
        slots_[t].pinned[b] = block.as<char>() + ((size_t)t * 2 + b) * kChunk;
        slots_[t].done[b] = std::move(done[t][b]);
      }
    }
    block_ = std::move(block);
    ready_ = true;
  }
};

}  // namespace zkpoa
