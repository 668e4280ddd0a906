// What the one-item-per-lane entry points of ecdsa_star.hip, ecdsa_sign.hip and bip32.hip share: the check of their
// arguments, the arrays of a call on the device, the loop over launches, and the wait after them. Internal to those files.
#pragma once
#include "zkpoa_internal.hpp"

namespace zkpoa {

inline uint32_t blocks_of(uint64_t lanes, uint32_t threads) { return (uint32_t)((lanes + threads - 1) / threads); }

inline void finish(hipStream_t st) {
  ZK_HIP(hipStreamSynchronize(st));
  ZK_HIP(hipGetLastError());
}

// The arguments of a call over n items; false: n == 0, and the call has nothing to do.
inline bool batch_wanted(const char* name, const char* items, uint64_t n, bool all_given) {
  if (n == 0) return false;
  if (n > (1ull << 32)) throw HipError(std::string(name) + ": at most 2^32 " + items + " per call");
  if (!all_given) throw HipError(std::string(name) + ": null argument");
  return true;
}

// A call's device memory that held keys or nonces: overwritten on the stream before it is given back.
struct SecretBuf : DevBuf {
  size_t bytes;
  hipStream_t st;
  SecretBuf(size_t n, hipStream_t s) : DevBuf(n), bytes(n), st(s) {}
  ~SecretBuf() {
    if (bytes) (void)hipMemsetAsync(p, 0, bytes, st);
    (void)hipStreamSynchronize(st);
  }
};

// One array of a call on the device: n items of `each` bytes, which is said here and nowhere else. Buf is DevBuf, or
// SecretBuf (with its stream as the last argument) for keys and nonces.
template <class Buf>
struct LaneArray {
  Buf buf;
  size_t each;
  uint64_t n;
  template <class... A>
  LaneArray(size_t each_, uint64_t n_, A... a) : buf(each_ * n_, a...), each(each_), n(n_) {}
  template <class T>
  T* at(uint64_t i0) const {   // item i0, where a launch over the items from i0 on begins
    return reinterpret_cast<T*>(static_cast<char*>(buf.p) + each * i0);
  }
};
template <class Buf = DevBuf>
struct LaneIn : LaneArray<Buf> {   // uploaded from the caller's array
  template <class... A>
  LaneIn(const void* host, size_t each_, uint64_t n_, A... a) : LaneArray<Buf>(each_, n_, a...) {
    this->buf.up(host, each_ * n_);
  }
};
template <class Buf = DevBuf>
struct LaneOut : LaneArray<Buf> {   // down() copies it into the caller's array
  void* host;
  template <class... A>
  LaneOut(void* host_, size_t each_, uint64_t n_, A... a) : LaneArray<Buf>(each_, n_, a...), host(host_) {}
  void down() const { ZK_HIP(hipMemcpy(host, this->buf.p, this->each * this->n, hipMemcpyDeviceToHost)); }
};

// launch(i0, m) for the items i0 .. i0 + m - 1, at most `slab` of them at a time
template <class Fn>
void for_slabs(uint64_t n, uint64_t slab, Fn launch) {
  for (uint64_t i0 = 0; i0 < n; i0 += slab) launch(i0, std::min(slab, n - i0));
}

// the launches of a call that reports its kernel time: between the context's event pair, waited for, into ms[8]
template <class Fn>
void timed_launches(zkpoa_context* ctx, hipStream_t st, Fn launches) {
  ZK_HIP(hipEventRecord(ctx->ev_a[0], st));
  launches();
  ZK_HIP(hipEventRecord(ctx->ev_b[0], st));
  finish(st);
  ZK_HIP(hipEventElapsedTime(&ctx->ms[8], ctx->ev_a[0], ctx->ev_b[0]));
}

}  // namespace zkpoa
