// The one parser of the numbers that the setup commands take from the environment (ZKPOA_DELTA, ZKPOA_PHASE1_S,
// ZKPOA_PHASE2_S: tests and reproducible records only). Host only, no HIP: csrc/setup_main.hip uses it next to
// csrc/worker_exit.hpp, the library through csrc/setup_common.hip.h (env_scalars, which adds the range check).
#pragma once
#include <stdint.h>
#include <string.h>

namespace zkpoa {

// [begin, end): decimal, or 0x / 0X and hex digits of either case -> 32 little-endian bytes. False for no digits, a
// character that is no digit of the base, or a value of 2^256 and above.
inline bool parse_u256(const char* begin, const char* end, uint8_t out[32]) {
  memset(out, 0, 32);
  const bool hex = end - begin >= 2 && begin[0] == '0' && (begin[1] | 32) == 'x';
  if (hex) begin += 2;
  if (begin == end) return false;
  for (const char* p = begin; p < end; p++) {
    unsigned carry;
    if (*p >= '0' && *p <= '9') carry = (unsigned)(*p - '0');
    else if (hex && (*p | 32) >= 'a' && (*p | 32) <= 'f') carry = (unsigned)((*p | 32) - 'a' + 10);
    else return false;
    for (int i = 0; i < 32; i++) {
      const unsigned v = out[i] * (hex ? 16u : 10u) + carry;
      out[i] = (uint8_t)v;
      carry = v >> 8;
    }
    if (carry) return false;
  }
  return true;
}

}  // namespace zkpoa
