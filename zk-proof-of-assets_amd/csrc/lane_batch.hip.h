// What the one-item-per-lane entry points of ecdsa_star.hip, ecdsa_sign.hip, bip32.hip and hooks_secp.hip add to the
// library's call shape (zkpoa_internal.hpp: LaneIn / LaneOut, for_slabs, blocks_of, finish, timed with kMsLaneBatch):
// the check of their arguments, and device memory that is wiped before it is given back.
#pragma once
#include "zkpoa_internal.hpp"

namespace zkpoa {

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

}  // namespace zkpoa
