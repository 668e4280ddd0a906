// Owning handles of the HIP resources the library holds: device memory, events, streams, pinned host memory.
// The rule: every HIP resource has one owning member, and giving it back is that member's destructor. All four types
// are empty by default and move-only; their destructors ignore errors, and none of them synchronises anything -- an
// owner whose resource may still be in use waits for that use itself, before the member goes. Each resource is given
// back on whatever device is current: an owner with a device of its own makes it current first.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdexcept>
#include <string>
#include <utility>

namespace zkpoa {

struct HipError : std::runtime_error {
  explicit HipError(const std::string& s) : std::runtime_error(s) {}
};

#define ZK_HIP(expr)                                                                              \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess)                                                                         \
      throw ::zkpoa::HipError(std::string(#expr) + " failed: " + hipGetErrorString(_e) + " at " + \
                              __FILE__ + ":" + std::to_string(__LINE__));                         \
  } while (0)

// Device memory with one owner, for whatever outlives a call: the arrays of a key handle, exchange buffers, a CSR on
// its way into a handle. Empty by default, move-only. An owner gives its memory back with hipFree and with nothing
// else: a member of a long-lived object must never land in a deferred_free_sink() merely because it is destroyed while
// one is set. Handing memory to a sink (or out through the C ABI) is always the explicit `sink.push_back(m.take())`.
// lent(p) makes the one non-owning state -- memory that belongs to the caller: used like any other, never freed.
// Temporaries of one call that should wait in the sink are DevBuf (zkpoa_internal.hpp).
class DevMem {
  void* p_ = nullptr;
  bool owned_ = true;

 public:
  DevMem() = default;
  static DevMem lent(const void* callers) {
    DevMem m;
    m.p_ = const_cast<void*>(callers);
    m.owned_ = false;
    return m;
  }
  DevMem(DevMem&& o) noexcept : p_(o.p_), owned_(o.owned_) { o.forget(); }
  DevMem& operator=(DevMem&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_;
      owned_ = o.owned_;
      o.forget();
    }
    return *this;
  }
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  ~DevMem() { reset(); }
  void alloc(size_t bytes) {   // replaces what was held; 0 bytes still gives a valid pointer
    reset();
    ZK_HIP(hipMalloc(&p_, bytes ? bytes : 1));
  }
  // alloc() for a caller that tells the errors apart (Arena::reserve: out of memory is not a failure of the call):
  // the error is returned, still set as the thread's last error, and the handle is empty
  hipError_t try_alloc(size_t bytes) {
    reset();
    const hipError_t e = hipMalloc(&p_, bytes ? bytes : 1);
    if (e != hipSuccess) p_ = nullptr;
    return e;
  }
  void reset() {
    if (p_ && owned_) (void)hipFree(p_);
    forget();
  }
  void* take() {   // the raw pointer, now the caller's to free; lent memory cannot be given away
    void* p = owned_ ? p_ : nullptr;
    forget();
    return p;
  }
  void* get() const { return p_; }
  template <class T>
  T* as() const { return static_cast<T*>(p_); }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  void forget() {
    p_ = nullptr;
    owned_ = true;
  }
};

struct DevEvent {   // an owned hipEvent_t; empty = not created
  hipEvent_t e = nullptr;
  DevEvent() = default;
  DevEvent(DevEvent&& o) noexcept : e(o.e) { o.e = nullptr; }
  DevEvent& operator=(DevEvent&& o) noexcept {
    std::swap(e, o.e);
    return *this;
  }
  ~DevEvent() {
    if (e) (void)hipEventDestroy(e);
  }
  // on the current device; flags: hipEventDefault for a pair that is timed, hipEventDisableTiming for one that orders
  void create(unsigned flags) { ZK_HIP(hipEventCreateWithFlags(&e, flags)); }
  operator hipEvent_t() const { return e; }
};

struct DevStream {   // an owned hipStream_t, non-blocking; empty = not created
  hipStream_t s = nullptr;
  DevStream() = default;
  DevStream(DevStream&& o) noexcept : s(o.s) { o.s = nullptr; }
  DevStream& operator=(DevStream&& o) noexcept {
    std::swap(s, o.s);
    return *this;
  }
  ~DevStream() {
    if (s) (void)hipStreamDestroy(s);
  }
  // on the current device; the error is the caller's to judge (a stream that is only a head start may be done without)
  hipError_t try_create(int priority) {
    const hipError_t e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority);
    if (e != hipSuccess) s = nullptr;
    return e;
  }
  void create(int priority) { ZK_HIP(try_create(priority)); }
  operator hipStream_t() const { return s; }
};

class PinnedMem {   // an owned hipHostMalloc block and its size; empty = not allocated
  void* p_ = nullptr;
  void* dev_ = nullptr;
  size_t bytes_ = 0;

 public:
  PinnedMem() = default;
  PinnedMem(PinnedMem&& o) noexcept : p_(o.p_), dev_(o.dev_), bytes_(o.bytes_) { o.p_ = o.dev_ = nullptr, o.bytes_ = 0; }
  PinnedMem& operator=(PinnedMem&& o) noexcept {
    std::swap(p_, o.p_);
    std::swap(dev_, o.dev_);
    std::swap(bytes_, o.bytes_);
    return *this;
  }
  ~PinnedMem() {
    if (p_) (void)hipHostFree(p_);
  }
  void alloc(size_t bytes) {   // an empty handle only
    const hipError_t e = hipHostMalloc(&p_, bytes, hipHostMallocDefault);
    if (e != hipSuccess) p_ = nullptr;
    ZK_HIP(e);
    bytes_ = bytes;
  }
  // the same memory as kernels address it (a read-back that a kernel writes, not a copy): asked for once, then dev()
  void map_to_device() { ZK_HIP(hipHostGetDevicePointer(&dev_, p_, 0)); }
  void* get() const { return p_; }
  void* dev() const { return dev_; }
  size_t bytes() const { return bytes_; }
  template <class T>
  T* as() const { return static_cast<T*>(p_); }
  explicit operator bool() const { return p_ != nullptr; }
};

}  // namespace zkpoa
