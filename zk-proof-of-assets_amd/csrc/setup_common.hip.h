// What the file commands of csrc/setup.hip (`zkey new`, `zkey verify`, ...) and csrc/ptau_verify.hip
// (`powersoftau verify`) share: the iden3 binary container, and the device passes that check the points of a section
// (curve, range, G2 subgroup). Internal linkage: each translation unit has its own copy.
#pragma once
#include "bn254_ec.hip.h"
#include "device_ctx.hpp"
#include "pairing.hpp"

#include <fcntl.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <map>
#include <stdexcept>
#include <string>

using namespace zkpoa;

namespace zkpoa {
template <class HF>
Affine<HF> host_generator();
template <> Affine<HFq> host_generator<HFq>();     // hooks_g1.hip
template <> Affine<HFq2> host_generator<HFq2>();   // hooks_g2.hip
}

namespace {

struct SetupError : std::runtime_error {
  explicit SetupError(const std::string& m) : std::runtime_error(m) {}
};

uint32_t rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
uint64_t rd64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }

struct MappedFile {
  const uint8_t* p = nullptr;
  uint64_t size = 0;
  int fd = -1;
  explicit MappedFile(const char* path) {
    fd = open(path, O_RDONLY);
    if (fd < 0) throw SetupError(std::string("cannot open ") + path);
    struct stat sb;
    if (fstat(fd, &sb) != 0 || sb.st_size <= 0) {
      close(fd);
      throw SetupError(std::string("cannot stat ") + path);
    }
    size = (uint64_t)sb.st_size;
    void* m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (m == MAP_FAILED) {
      close(fd);
      throw SetupError(std::string("cannot map ") + path);
    }
    p = static_cast<const uint8_t*>(m);
  }
  ~MappedFile() {
    if (p) munmap(const_cast<uint8_t*>(p), size);
    if (fd >= 0) close(fd);
  }
  MappedFile(const MappedFile&) = delete;
  MappedFile& operator=(const MappedFile&) = delete;
};

struct Sec {
  uint64_t off = 0, len = 0;
  bool present = false;
};

// iden3 binary container: magic(4) version(u32) nSections(u32) then { type(u32) size(u64) payload }
std::map<uint32_t, Sec> bin_sections(const MappedFile& f, const char* magic, uint32_t max_version, const char* what) {
  if (f.size < 12 || memcmp(f.p, magic, 4) != 0) throw SetupError(std::string(what) + ": bad magic");
  if (rd32(f.p + 4) > max_version) throw SetupError(std::string(what) + ": unsupported version");
  const uint32_t n = rd32(f.p + 8);
  std::map<uint32_t, Sec> out;
  uint64_t pos = 12;
  for (uint32_t i = 0; i < n; i++) {
    if (pos + 12 > f.size) throw SetupError(std::string(what) + ": truncated section table");
    const uint32_t type = rd32(f.p + pos);
    const uint64_t len = rd64(f.p + pos + 4);
    pos += 12;
    if (len > f.size - pos) throw SetupError(std::string(what) + ": section runs past the end of the file");
    if (!out.count(type)) out[type] = Sec{pos, len, true};   // the first section of a type (as snarkjs' readers)
    pos += len;
  }
  return out;
}

struct DevArr {
  void* p = nullptr;
  explicit DevArr(size_t bytes) { ZK_HIP(hipMalloc(&p, bytes ? bytes : 1)); }
  ~DevArr() { if (p) (void)hipFree(p); }
  DevArr(const DevArr&) = delete;
  DevArr& operator=(const DevArr&) = delete;
  void up(const void* src, size_t bytes, size_t at = 0) {
    if (bytes) ZK_HIP(hipMemcpy(static_cast<char*>(p) + at, src, bytes, hipMemcpyHostToDevice));
  }
};

// The curve's b in the wire encoding (G1: 3, first 32 B; G2: 3 / (9 + u), 64 B), made on the host.
struct CurveB {
  uint4 q[4];
};
// One streaming pass over n affine points (wire format): flags |= 1 for a coordinate >= q (the range check of
// range_check_kernel), |= 2 for a point that is neither on the curve nor the all-zero point at infinity.
template <class F>
static __global__ __launch_bounds__(256) void point_check_kernel(const void* __restrict__ pts, uint64_t n, CurveB b,
                                                                 uint32_t* __restrict__ flags) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  constexpr int kWords = FieldBytes<F>::N / 16;   // 32-byte coordinate words per point: 2 (G1), 4 (G2)
  const uint4* q = reinterpret_cast<const uint4*>(pts) + (size_t)2 * kWords * i;
  uint32_t over = 0, nz = 0;
#pragma unroll
  for (int w = 0; w < kWords; w++) {
    const uint4 a = q[2 * w], c = q[2 * w + 1];
    const uint32_t l[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
    uint32_t bw = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      (void)subb(l[k], FqParams::P[k], bw);
      nz |= l[k];
    }
    over |= bw ^ 1u;   // no borrow: value >= q
  }
  if (over) {
    atomicOr(flags, 1u);
    return;
  }
  if (!nz) return;
  const Affine<F> p = load_affine<F>(pts, i);
  if (p.y.sqr() != p.x.sqr() * p.x + load_field<F>(b.q)) atomicOr(flags, 2u);
}

// G2 subgroup membership over n points: flags |= 4 unless Q is in G2 (the all-zero infinity passes). The endomorphism
// test for BN curves (eprint 2022/348, sections 3 and 5.1): Q is in G2 iff
//   [x+1]Q + psi([x]Q) + psi^2([x]Q) == psi^3([2x]Q),   x = 4965661367192848881 (the BN parameter, 63 bits)
// with psi the twisted Frobenius (pairing.hpp FrobConsts). One 63-bit double-and-add instead of a 254-bit [r]Q ladder;
// every lane follows the same bit pattern, and the additions handle the exceptional cases (P + P, P - P) that points
// outside G2 can meet.
struct FrobArg {   // psi(x, y) = (conj(x) g2c, conj(y) g3c): g2c then g3c, wire form, made on the host (frob_arg)
  uint4 q[8];
};
inline FrobArg frob_arg() {
  FrobArg a;
  pairing::frob_consts().g2c.to_bytes(&a.q[0]);
  pairing::frob_consts().g3c.to_bytes(&a.q[4]);
  return a;
}
// psi on XYZZ coordinates: conj is a field automorphism, so (conj(X) g2c, conj(Y) g3c, conj(ZZ), conj(ZZZ))
ZK_DEV XYZZ<Fq2> g2_psi(const XYZZ<Fq2>& a, const Fq2& cx, const Fq2& cy) {
  return {Fq2{a.x.c0, a.x.c1.neg()} * cx, Fq2{a.y.c0, a.y.c1.neg()} * cy, Fq2{a.zz.c0, a.zz.c1.neg()},
          Fq2{a.zzz.c0, a.zzz.c1.neg()}};
}
static __global__ __launch_bounds__(256) void g2_subgroup_kernel(const void* __restrict__ pts, uint64_t n, FrobArg fa,
                                                                 uint32_t* __restrict__ flags) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const Affine<Fq2> p = load_affine<Fq2>(pts, i);
  if (p.is_inf()) return;
  constexpr uint64_t kX = 4965661367192848881ull;
  XYZZ<Fq2> xq = XYZZ<Fq2>::inf();
  for (int bit = 62; bit >= 0; bit--) {
    xq = xyzz_dbl(xq);
    if ((kX >> bit) & 1u) xyzz_add_affine(xq, p, false);
  }
  const Fq2 cx = load_field<Fq2>(&fa.q[0]), cy = load_field<Fq2>(&fa.q[4]);
  XYZZ<Fq2> lhs = xq;
  xyzz_add_affine(lhs, p, false);                         // [x+1]Q
  XYZZ<Fq2> t = g2_psi(xq, cx, cy);
  xyzz_add(lhs, t);                                       // + psi([x]Q)
  t = g2_psi(t, cx, cy);
  xyzz_add(lhs, t);                                       // + psi^2([x]Q)
  const XYZZ<Fq2> rhs = g2_psi(g2_psi(g2_psi(xyzz_dbl(xq), cx, cy), cx, cy), cx, cy);
  xyzz_add(lhs, xyzz_neg(rhs));
  if (!lhs.is_inf()) atomicOr(flags, 4u);
}

}  // namespace
