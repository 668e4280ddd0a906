// What the prover (prover.hip) and the setup commands (setup_common.hip.h) both read of iden3's binary files, host code
// only: the container's section table, the Groth16 header of a .zkey, the point sections of a .ptau, and random bytes. Nothing here throws a file
// error of its own: each caller turns a failure into its own exception type and text (include/zkpoa_prover.h lists
// the prover's).
#pragma once
#include "host_field.hpp"

#include <fcntl.h>
#include <stdint.h>
#include <string.h>
#include <unistd.h>

#include <array>
#include <functional>
#include <map>

namespace zkpoa {

inline uint32_t rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
inline uint64_t rd64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }

// ---- container: magic(4) version(u32) nSections(u32) then { type(u32) size(u64) payload } ------------------------------
struct Sec {
  uint64_t off = 0, len = 0;   // of the payload
};
enum BinScan { kBinOk, kBinBadMagic, kBinVersion, kBinTruncatedTable, kBinTruncatedSection };
// The section table of a file of `size` bytes; read(pos, out, len) fetches bytes of it (12 at a time: a file on disk is
// walked with pread, payloads are skipped). The first section of a type wins (as snarkjs' readers).
inline BinScan bin_scan(const std::function<void(uint64_t, void*, size_t)>& read, uint64_t size, const char* magic,
                        uint32_t max_version, std::map<uint32_t, Sec>& out) {
  uint8_t h[12];
  if (size < 12) return kBinBadMagic;
  read(0, h, 12);
  if (memcmp(h, magic, 4) != 0) return kBinBadMagic;
  if (rd32(h + 4) > max_version) return kBinVersion;
  const uint32_t n = rd32(h + 8);
  uint64_t pos = 12;
  for (uint32_t i = 0; i < n; i++) {
    if (pos + 12 > size) return kBinTruncatedTable;
    read(pos, h, 12);
    const uint32_t type = rd32(h);
    const uint64_t len = rd64(h + 4);
    pos += 12;
    if (len > size - pos) return kBinTruncatedSection;
    if (!out.count(type)) out[type] = Sec{pos, len};
    pos += len;
  }
  return kBinOk;
}
inline BinScan bin_scan(const uint8_t* buf, uint64_t size, const char* magic, uint32_t max_version,
                        std::map<uint32_t, Sec>& out) {
  return bin_scan([buf](uint64_t pos, void* o, size_t len) { memcpy(o, buf + pos, len); }, size, magic, max_version, out);
}

// ---- Groth16 header (zkey section 2): n8q(u32) q(32) n8r(u32) r(32) nVars nPublic domain (u32 each), then six points ----
constexpr uint64_t kHdr = 4 + 32 + 4 + 32 + 12, kAlpha1 = kHdr, kBeta1 = kHdr + 64, kBeta2 = kHdr + 128,
                   kGamma2 = kHdr + 256, kDelta1 = kHdr + 384, kDelta2 = kHdr + 448, kHdrLen = kHdr + 576;
struct ZkeyHeader {
  uint32_t n8q, n8r;   // field sizes in bytes: 32
  bool q_ok, r_ok;     // the moduli are BN254's
  uint32_t nVars, nPublic, domain;
  const uint8_t *alpha1, *beta1, *beta2, *gamma2, *delta1, *delta2;   // G1: 64 B, G2: 128 B, wire format
};
// p: the section's payload, at least kHdrLen bytes. What a wrong size or modulus means is the caller's policy.
inline ZkeyHeader read_zkey_header(const uint8_t* p) {
  return {rd32(p), rd32(p + 36), memcmp(p + 4, HFqParams::P, 32) == 0, memcmp(p + 40, HFrParams::P, 32) == 0,
          rd32(p + 72), rd32(p + 76), rd32(p + 80),
          p + kAlpha1, p + kBeta1, p + kBeta2, p + kGamma2, p + kDelta1, p + kDelta2};
}

// ---- ceremony file (.ptau) of power p, N = 2^p: its point sections, G1 points of 64 B and G2 points of 128 B ------------
struct PowerSec {   // the powers: tau^i G1, tau^i G2, alpha tau^i G1, beta tau^i G1, beta G2
  uint32_t id;
  int group;
  uint64_t count;
  uint64_t unit() const { return group == 2 ? 128 : 64; }
  uint64_t bytes() const { return count * unit(); }
};
inline std::array<PowerSec, 5> ptau_power_secs(uint32_t power) {
  const uint64_t N = 1ull << power;
  return {{{2, 1, 2 * N - 1}, {3, 2, N}, {4, 1, N}, {5, 1, N}, {6, 2, 1}}};
}
struct LagrangeSec {   // section dst: levels 0..top, level l = the 2^l Lagrange-form points of the first 2^l of section src
  uint32_t src, dst;
  int group;
  uint32_t top;
  uint64_t unit() const { return group == 2 ? 128 : 64; }
  uint64_t count() const { return (2ull << top) - 1; }
  uint64_t bytes() const { return count() * unit(); }
};
inline std::array<LagrangeSec, 4> ptau_lagrange_secs(uint32_t power) {
  return {{{2, 12, 1, power + 1}, {3, 13, 2, power}, {4, 14, 1, power}, {5, 15, 1, power}}};
}

// len bytes of /dev/urandom (short reads are continued); returns null, or what went wrong
inline const char* read_urandom(void* dst, size_t len) {
  const int fd = open("/dev/urandom", O_RDONLY);
  if (fd < 0) return "cannot open /dev/urandom";
  size_t got = 0;
  while (got < len) {
    const ssize_t k = read(fd, static_cast<char*>(dst) + got, len - got);
    if (k <= 0) break;
    got += (size_t)k;
  }
  close(fd);
  return got == len ? nullptr : "short read from /dev/urandom";
}

}  // namespace zkpoa
