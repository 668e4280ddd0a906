// What the file commands of csrc/setup.hip (`zkey new`, `zkey contribute`, `wtns check`), csrc/zkey_verify.hip (`zkey
// verify`), csrc/ptau_verify.hip (`powersoftau verify`), csrc/ptau_prepare.hip (`powersoftau prepare phase2`) and
// csrc/ptau_contribute.hip (the other `powersoftau` commands) share: the section tables of mapped files (the scan
// and the point sections of a ceremony file: binfile.hpp), the ptau header and the shape of its power sections (the
// file itself: ptau_file.hip.h), the scalars a command draws or takes from the environment (scalar_in_range,
// random_scalar, env_scalars), output files whose sections are placed in any order (SectionFile), host arrays, the r1cs
// parser and its CSR, the ptau ranges a key is made from, the constraint-fold kernels, the piece loop that streams a
// section from its file through HBM (for_each_piece, piece_from_free_hbm), and the device passes that check the points
// of a section (curve, range, G2 subgroup: PointChecker). Internal linkage: each translation unit has its own copy.
// What is neither device nor setup -- mapped files, AtomicFile, the phase timer, host threads, numbers as text -- is
// host_files.hpp and host_text.hpp.
#pragma once
#include "binfile.hpp"
#include "bn254_ec.hip.h"
#include "device_ctx.hpp"
#include "host_files.hpp"
#include "host_text.hpp"
#include "msm.hip.h"
#include "pairing.hpp"
#include "zkpoa_internal.hpp"

#include <algorithm>
#include <map>
#include <memory>

using namespace zkpoa;

namespace zkpoa {
template <class HF>
Affine<HF> host_generator();
template <> Affine<HFq> host_generator<HFq>();     // hooks_g1.hip
template <> Affine<HFq2> host_generator<HFq2>();   // hooks_g2.hip
// One-shot commands (zkpoa-setup) leave the tens of GB of host arrays of a `zkey new` to the process's exit: giving
// 100 GB back page by page takes seconds that nobody is waiting for any more (zkpoa_setup_defer_host_frees).
// setup.hip: the transcript checks of `zkey verify` (ZKPOA_ZKEY_CSHASH | ZKPOA_ZKEY_CONTRIBUTIONS) on a key whose circuit
// hash is not zero; a malformed section 10 throws
uint32_t phase2_verify(zkpoa_context* ctx, const char* r1cs_path, const char* ptau_path, const char* zkey_path);
// setup.hip: the test hooks zkpoa_hash_form / zkpoa_compressed_form. The hash form (compressed: the compressed form) of n
// points of group 1 / 2 (host, wire form) streamed in pieces of piece_points, its Blake2b-512 digest and, with out, the bytes
void points_form(zkpoa_context* ctx, int group, const void* points, uint64_t n, uint64_t piece_points, bool compressed,
                 void* out, uint8_t digest[64]);
inline std::atomic<bool>& defer_host_frees() {   // one flag for all the units
  static std::atomic<bool> on{false};
  return on;
}
}

namespace {

struct SetupError : std::runtime_error {
  explicit SetupError(const std::string& m) : std::runtime_error(m) {}
};

// Every input of these commands begins with a header: an empty file is refused in the words the commands always had for
// it. bin_sections does this for the files that have a section table; a command that maps another kind calls it itself.
void nonempty(const MappedFile& f) {
  if (!f.size) throw SetupError("cannot stat " + f.path);
}

// the section table of an iden3 binary file (binfile.hpp), with the setup commands' error texts
std::map<uint32_t, Sec> bin_sections(const MappedFile& f, const char* magic, uint32_t max_version, const char* what) {
  static const char* const why[] = {"", "bad magic", "unsupported version", "truncated section table",
                                    "section runs past the end of the file"};
  nonempty(f);
  std::map<uint32_t, Sec> out;
  const BinScan r = bin_scan(f.p, f.size, magic, max_version, out);
  if (r != kBinOk) throw SetupError(std::string(what) + ": " + why[r]);
  return out;
}

// header of a .ptau (section 1): n8(u32) q(32) power(u32) ceremony power(u32); returns the power
uint32_t ptau_header(const MappedFile& f, const Sec& h, uint32_t* ceremony = nullptr) {
  if (h.len < 4 + 32 + 8 || rd32(f.p + h.off) != 32) throw SetupError("ptau: header too short or field size != 32");
  if (memcmp(f.p + h.off + 4, HFqParams::P, 32) != 0) throw SetupError("ptau: not a BN254 ceremony");
  if (ceremony) *ceremony = rd32(f.p + h.off + 40);
  return rd32(f.p + h.off + 36);
}

// The power sections of a ceremony file (`powersoftau verify`, `powersoftau prepare phase2`): sections 1-7 present, a
// BN254 header, a power in [1, 28], and sections 2-6 of the lengths that power gives (N = 2^power: 2N - 1 G1, N G2, N G1,
// N G1, one G2). Anything else is a malformed file.
struct PtauShape {
  uint32_t power, ceremony, contributions;
};
PtauShape ptau_power_sections(const MappedFile& fp, std::map<uint32_t, Sec>& ps) {
  for (uint32_t t = 1; t <= 7; t++)
    if (!ps.count(t)) throw SetupError("ptau: section " + std::to_string(t) + " missing");
  PtauShape s{0, 0, 0};
  s.power = ptau_header(fp, ps[1], &s.ceremony);
  if (s.power < 1 || s.power > 28) throw SetupError("ptau: power " + std::to_string(s.power) + " is outside [1, 28]");
  for (const PowerSec& sc : ptau_power_secs(s.power))
    if (ps[sc.id].len != sc.bytes()) throw SetupError("ptau: section " + std::to_string(sc.id) + " has the wrong length for power " + std::to_string(s.power));
  if (ps[7].len < 4) throw SetupError("ptau: section 7 has the wrong length");
  s.contributions = rd32(fp.p + ps[7].off);
  return s;
}
// level power + 1 of section 12 is a transform of 2^(power + 1) points, and BN254's Fr has 2^28-th roots of unity at most
void ptau_check_preparable(uint32_t power) {
  if (power > 27) throw SetupError("ptau: a prepared file of power above 27 has no root of unity for its top level");
}

void urandom(void* dst, size_t len) {
  if (const char* err = read_urandom(dst, len)) throw SetupError(err);
}

// ---- scalars: 32 B little-endian, standard form ---------------------------------------------------------------------
bool scalar_in_range(const uint8_t le[32], bool nonzero) {   // below r, and not zero when nonzero
  uint64_t v[4];
  memcpy(v, le, 32);
  return !HFr::geq_p(v) && (!nonzero || (v[0] | v[1] | v[2] | v[3]));
}
void random_scalar(uint8_t d[32]) {   // uniform on [1, r): 254 random bits, rejected while >= r or zero
  do {
    urandom(d, 32);
    d[31] &= 0x3f;
  } while (!scalar_in_range(d, true));
}
// Tests / reproducible records only: `count` numbers in [1, r), decimal or 0x... hex, separated by commas, from the
// text row `id`. False when it is not set; anything else than `shape` throws; a warning names `secrets`.
bool env_scalars(Opt id, uint8_t out[][32], int count, const char* shape, const char* secrets) {
  const char *e = opt_text(id), *name = opt_row(id).name;
  if (!e) return false;
  for (int k = 0; k < count; k++) {
    const char* end = strchr(e, ',');
    if ((k < count - 1) != (end != nullptr)) end = nullptr;   // too few numbers, or too many
    else if (!end) end = e + strlen(e);
    U256 x;
    const bool parsed = end && x.parse_number(e, end);
    x.to_le(out[k]);
    if (!parsed || !scalar_in_range(out[k], true)) throw SetupError(std::string(name) + " is not " + shape);
    e = end + 1;
  }
  fprintf(stderr, "zkpoa: WARNING: %s taken from %s -- for tests only\n", secrets, name);
  return true;
}
Fr fr_dev(const HFr& h) {   // a kernel argument: the same limbs
  Fr f;
  memcpy(&f, &h, 32);
  return f;
}
ZK_DEV Fr fr_pow_u64(Fr b, uint64_t e) {
  Fr r = Fr::one();
  while (e) {
    if (e & 1u) r = r * b;
    b = b.sqr();
    e >>= 1;
  }
  return r;
}

bool same_file(const char* a, const char* b) {
  struct stat sa, sb;
  if (stat(a, &sa) != 0 || stat(b, &sb) != 0) return false;
  return sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino;
}

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


// The point checks of a section on lane 0: point_check_kernel, for G2 optionally g2_subgroup_kernel.
struct PointChecker {
  Lane& lane;
  DevBuf flags{64};   // word 0: the checks' bits; words 1-15 are free for the caller's kernels. Zero between read()s.
  CurveB b1{}, b2{};
  const FrobArg frob = frob_arg();
  explicit PointChecker(zkpoa_context* ctx) : lane(ctx->dev.lanes[0]) {
    HFq::from_u64(3).to_bytes(&b1.q[0]);
    pairing::twist_b().to_bytes(&b2.q[0]);
    ZK_HIP(hipMemsetAsync(flags.p, 0, 64, lane.stream));
  }
  uint32_t* fl() { return reinterpret_cast<uint32_t*>(flags.p); }
  uint32_t read() {   // word 0 (the stream is synchronised), then every flag word zeroed
    msm_read_back(lane, flags.p, 4);
    uint32_t f;
    memcpy(&f, lane.pinned.get(), 4);
    ZK_HIP(hipMemsetAsync(flags.p, 0, 64, lane.stream));
    return f;
  }
  // over count points of group 1 / 2 at d: bit 1 = a point off its curve, bit 2 (subgroup) = a G2 point outside G2;
  // a coordinate that is no field element throws
  uint32_t check(const void* d, uint64_t count, int group, bool subgroup, const char* what) {
    if (!count) return 0u;
    const dim3 grid((uint32_t)((count + 255) / 256));
    if (group == 1) hipLaunchKernelGGL((point_check_kernel<Fq>), grid, dim3(256), 0, lane.stream, d, count, b1, fl());
    else hipLaunchKernelGGL((point_check_kernel<Fq2>), grid, dim3(256), 0, lane.stream, d, count, b2, fl());
    if (subgroup) hipLaunchKernelGGL(g2_subgroup_kernel, grid, dim3(256), 0, lane.stream, d, count, frob, fl());
    const uint32_t f = read();
    if (f & 1u) throw SetupError(std::string(what) + ": a coordinate is not a field element (>= q)");
    return f;
  }
  // the same for a command that refuses the file: either bit throws
  void require(const void* d, uint64_t count, int group, bool subgroup, const char* what) {
    const uint32_t f = check(d, count, group, subgroup, what);
    if (f & 2u) throw SetupError(std::string(what) + ": a point is not on the curve");
    if (f & 4u) throw SetupError(std::string(what) + ": a point is outside G2");
  }
};

// ---- a section streamed from its file through HBM ------------------------------------------------------------------------
// `count` elements of `unit` bytes at file_offset of fd, at most `piece` of them at a time: each piece is uploaded to d_buf
// (the context's pinned uploader, lane 0's stream), then fn(i0, cnt) runs. upload_ms: the host's time in the uploads.
template <class Fn>
void for_each_piece(zkpoa_context* ctx, int fd, uint64_t file_offset, uint64_t count, uint64_t unit, uint64_t piece,
                    void* d_buf, Fn fn, double* upload_ms = nullptr) {
  for (uint64_t i0 = 0; i0 < count; i0 += piece) {
    const uint64_t cnt = std::min(piece, count - i0);
    const auto t0 = std::chrono::steady_clock::now();
    ctx->uploader.upload(d_buf, nullptr, cnt * unit, ctx->dev.device, ctx->dev.lanes[0].stream, fd, file_offset + i0 * unit);
    if (upload_ms) *upload_ms += ms_since(t0);
    fn(i0, cnt);
  }
}
// points per piece when a quarter of the free HBM goes to the pieces' buffers, within [lo, hi]
uint64_t piece_from_free_hbm(uint64_t bytes_per_point, uint64_t lo, uint64_t hi) {
  size_t free_b = 0, total_b = 0;
  ZK_HIP(hipMemGetInfo(&free_b, &total_b));
  return std::max<uint64_t>(lo, std::min<uint64_t>(free_b / 4 / bytes_per_point, hi));
}

// ---- `snarkjs wtns check`: constraint c holds iff <A_c, w> * <B_c, w> == <C_c, w> ------------------------------------
// row_ptr[3 * c + m .. +1): the terms of matrix m of constraint c; coefficients and witness in Montgomery form.
// flags[0] = number of violated constraints, flags[1] = the smallest violated index (atomicMin, starts at ~0).
// folds (optional, `zkey verify`): the three products are also stored, Montgomery form, at folds[m * fold_stride + c].
static __global__ __launch_bounds__(256) void wtns_check_kernel(const uint32_t* __restrict__ row_ptr,
                                                                const uint32_t* __restrict__ sig,
                                                                const void* __restrict__ coef_m,
                                                                const void* __restrict__ w_m, uint32_t n_cons,
                                                                uint32_t* __restrict__ flags, void* __restrict__ folds,
                                                                uint32_t fold_stride) {
  uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= n_cons) return;
  Fr v[3];
#pragma unroll
  for (int m = 0; m < 3; m++) {
    Fr acc = Fr::zero();
    for (uint32_t t = row_ptr[3 * c + m]; t < row_ptr[3 * c + m + 1]; t++)
      acc = acc + load_field<Fr>(reinterpret_cast<const char*>(coef_m) + 32 * (size_t)t) *
                      load_field<Fr>(reinterpret_cast<const char*>(w_m) + 32 * (size_t)sig[t]);
    v[m] = acc;
    if (folds) store_field(reinterpret_cast<char*>(folds) + 32 * ((size_t)m * fold_stride + c), acc);
  }
  if (!(v[0] * v[1] - v[2]).is_zero()) {
    atomicAdd(&flags[0], 1u);
    atomicMin(&flags[1], c);
  }
}
// in place: standard form (canonical, < r checked by the caller's flag) -> Montgomery
static __global__ __launch_bounds__(256) void fr_to_mont_kernel(void* __restrict__ data, uint64_t n, uint32_t* __restrict__ bad) {
  uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  char* p = reinterpret_cast<char*>(data) + 32 * i;
  Fr v = load_field<Fr>(p);
  uint32_t bw = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) (void)subb(v.l[k], FrParams::P[k], bw);
  if (!bw) atomicOr(bad, 1u);
  store_field(p, v.to_mont());
}

// the threads that fill a host array are the first to touch it (host_files.hpp: parallel_ranges)
template <class T>
struct UVec {   // a sized array of trivially copyable elements whose storage is NOT value-initialised
  std::unique_ptr<T[]> p;
  size_t n = 0;
  UVec() = default;
  UVec(UVec&&) = default;
  UVec& operator=(UVec&&) = default;
  ~UVec() {
    if (defer_host_frees().load()) (void)p.release();
  }
  explicit UVec(size_t count) { alloc(count); }
  void alloc(size_t count) {
    p.reset(new T[count ? count : 1]);
    n = count;
  }
  size_t size() const { return n; }
  bool empty() const { return n == 0; }
  T* data() { return p.get(); }
  const T* data() const { return p.get(); }
  T& operator[](size_t i) { return p[i]; }
  const T& operator[](size_t i) const { return p[i]; }
  const T* begin() const { return p.get(); }
  const T* end() const { return p.get() + n; }
};

// An iden3 binary file whose section lengths are known before their content: the file is sized, the magic, version 1,
// the section count and the table (sections in the order of ids) are written, and a payload is then placed from any
// thread, in any order.
struct SectionFile {
  AtomicFile file;
  std::map<uint32_t, Sec> secs;   // where each payload goes
  SectionFile(const char* path, const char* magic, const uint32_t* ids, const uint64_t* lens, uint32_t count) : file(path) {
    uint64_t total = 12;
    for (uint32_t i = 0; i < count; i++) {
      secs[ids[i]] = Sec{total + 12, lens[i]};
      total += 12 + lens[i];
    }
    file.reserve(total);
    const uint32_t hdr[2] = {1, count};   // version, sections
    file.put_at(0, magic, 4);
    file.put_at(4, hdr, 8);
    for (uint32_t i = 0; i < count; i++) {
      file.put_at(off(ids[i]) - 12, &ids[i], 4);
      file.put_at(off(ids[i]) - 8, &lens[i], 8);
    }
  }
  uint64_t off(uint32_t id) const { return secs.at(id).off; }
  uint64_t len(uint32_t id) const { return secs.at(id).len; }
  void put(uint32_t id, const void* p, uint64_t n) {   // the whole section
    if (n != len(id)) throw SetupError("internal: section " + std::to_string(id) + " has an unexpected size");
    file.put_at(off(id), p, n);
  }
  void put_at(uint32_t id, uint64_t byte_offset, const void* p, uint64_t n) { file.put_at(off(id) + byte_offset, p, n); }
  void commit() { file.commit(); }
};

// Untrusted inputs: the device keeps Fq elements lazily in [0, 2q) and takes file bytes raw, so every
// coordinate that reaches a kernel or is copied into the key must be a canonical field element (< q).
void host_check_coords(const uint8_t* p, uint64_t count32, const char* what) {
  parallel_ranges(count32, 1u << 20, [&](unsigned, uint64_t lo, uint64_t hi) {
    for (uint64_t i = lo; i < hi; i++) {
      uint64_t v[4];
      memcpy(v, p + 32 * i, 32);
      if (v[3] >= HFqParams::P[3] && HFq::geq_p(v)) throw SetupError(std::string(what) + ": a coordinate is not a field element (>= q)");
    }
  });
}
struct Term {
  uint32_t c, s;
  uint8_t coef[32];
};

struct R1cs {
  uint32_t nWires = 0, nPublic = 0, nConstraints = 0;
  UVec<Term> A, B, C;   // per constraint in file order, terms of one linear combination ascending by signal
};

// Two passes: the first walks the term counts only (three words per constraint) and notes, every 2^14 constraints, where
// the constraint starts in the file and how many A / B / C terms precede it; the second parses those blocks in parallel
// straight into their places.
R1cs parse_r1cs(const MappedFile& f) {
  auto secs = bin_sections(f, "r1cs", 1, "r1cs");
  if (!secs.count(1) || !secs.count(2)) throw SetupError("r1cs: header or constraint section missing");
  const Sec h = secs[1], cs = secs[2];
  if (h.len < 4 + 32 + 4 * 4 + 8 + 4 || rd32(f.p + h.off) != 32) throw SetupError("r1cs: header too short or field size != 32");
  for (int i = 0; i < 4; i++)
    if (rd64(f.p + h.off + 4 + 8 * i) != HFrParams::P[i]) throw SetupError("r1cs: not over the BN254 scalar field");
  const uint8_t* q = f.p + h.off + 36;
  R1cs r;
  r.nWires = rd32(q);
  const uint64_t n_public = (uint64_t)rd32(q + 4) + rd32(q + 8);   // outputs + public inputs (no 32-bit wrap)
  r.nConstraints = rd32(q + 24);
  if (r.nWires == 0 || n_public + 1 > r.nWires) throw SetupError("r1cs: inconsistent wire counts");
  r.nPublic = (uint32_t)n_public;
  const uint64_t end = cs.off + cs.len;
  constexpr uint32_t kBlock = 1u << 14;
  struct Mark { uint64_t pos, cnt[3]; };
  std::vector<Mark> marks;
  marks.reserve(r.nConstraints / kBlock + 2);
  {
    uint64_t pos = cs.off, cnt[3] = {0, 0, 0};
    for (uint32_t c = 0; c < r.nConstraints; c++) {
      if ((c & (kBlock - 1)) == 0) marks.push_back(Mark{pos, {cnt[0], cnt[1], cnt[2]}});
      for (int m = 0; m < 3; m++) {
        if (pos + 4 > end) throw SetupError("r1cs: constraint section truncated");
        const uint32_t nt = rd32(f.p + pos);
        pos += 4;
        if ((uint64_t)nt * 36 > end - pos) throw SetupError("r1cs: constraint section truncated");
        pos += (uint64_t)nt * 36;
        cnt[m] += nt;
      }
    }
    marks.push_back(Mark{pos, {cnt[0], cnt[1], cnt[2]}});
  }
  const Mark& tot = marks.back();
  r.A.alloc(tot.cnt[0]);
  r.B.alloc(tot.cnt[1]);
  r.C.alloc(tot.cnt[2]);
  const uint64_t blocks = marks.size() - 1;
  parallel_ranges(blocks, 1, [&](unsigned, uint64_t b0, uint64_t b1) {
    for (uint64_t b = b0; b < b1; b++) {
      uint64_t pos = marks[b].pos, at[3] = {marks[b].cnt[0], marks[b].cnt[1], marks[b].cnt[2]};
      const uint32_t c1 = (uint32_t)std::min<uint64_t>((b + 1) * kBlock, r.nConstraints);
      for (uint32_t c = (uint32_t)(b * kBlock); c < c1; c++) {
        for (int m = 0; m < 3; m++) {
          const uint32_t nt = rd32(f.p + pos);
          pos += 4;
          Term* dst = (m == 0 ? r.A.data() : (m == 1 ? r.B.data() : r.C.data())) + at[m];
          for (uint32_t t = 0; t < nt; t++, pos += 36) {
            Term& x = dst[t];
            x.c = c;
            x.s = rd32(f.p + pos);
            memcpy(x.coef, f.p + pos + 4, 32);
            if (x.s >= r.nWires) throw SetupError("r1cs: wire index out of range");
            uint64_t v[4];
            memcpy(v, x.coef, 32);
            if (HFr::geq_p(v)) throw SetupError("r1cs: coefficient is not a field element (>= r)");
          }
          // snarkjs holds a linear combination as an object keyed by the signal: iteration is ascending by signal
          std::stable_sort(dst, dst + nt, [](const Term& a, const Term& b) { return a.s < b.s; });
          for (uint32_t t = 1; t < nt; t++)
            if (dst[t].s == dst[t - 1].s) throw SetupError("r1cs: a signal occurs twice in one linear combination");
          at[m] += nt;
        }
      }
    }
  });
  return r;
}

void pread_all(int fd, void* dst, uint64_t len, uint64_t off, const char* what) {
  parallel_ranges(len, 32ull << 20, [&](unsigned, uint64_t lo, uint64_t hi) {
    uint64_t got = lo;
    while (got < hi) {
      ssize_t n = pread(fd, static_cast<char*>(dst) + got, hi - got, (off_t)(off + got));
      if (n <= 0) throw SetupError(std::string("ptau: short read of ") + what);
      got += (uint64_t)n;
    }
  });
}

// the domain of `zkey new`: the smallest power of two that holds the constraints and the nPublic + 1 extra rows (zkey_new.js)
uint32_t domain_log2(const R1cs& r) {
  uint32_t cp = 0;
  while ((1ull << cp) < (uint64_t)r.nConstraints + r.nPublic + 1) cp++;
  if (cp > 27) throw SetupError("circuit too large (domain above 2^27)");
  return cp;
}

// what `zkey new` (and `zkey verify`) read of a phase-2 .ptau for a domain of 2^cp: level cp of sections 12-15, level
// cp + 1 of section 12 (the 2n basis, whose odd points are H), and alpha*G1, beta*G1, beta*G2 (sections 4-6)
struct PtauRanges {
  UVec<uint8_t> L1, L2, aL, bL, Hs;
  uint8_t alpha1[64], beta1[64], beta2[128];
};
PtauRanges read_ptau_ranges(const char* ptau_path, uint32_t cp) {
  const uint64_t n = 1ull << cp;
  MappedFile fp(ptau_path);   // mapped for the section table only; the point ranges are read with pread
  auto ps = bin_sections(fp, "ptau", 1, "ptau");
  for (uint32_t t : {1u, 4u, 5u, 6u, 12u, 13u, 14u, 15u})
    if (!ps.count(t)) throw SetupError("ptau: section " + std::to_string(t) + " missing (the file must be prepared for phase 2)");
  const uint32_t power = ptau_header(fp, ps[1]);
  if (cp > power) throw SetupError("ptau: ceremony of 2^" + std::to_string(power) + " is too small for a 2^" + std::to_string(cp) + " domain");
  auto level = [&](uint32_t sec, uint32_t lvl, uint64_t unit, uint64_t count, const char* what) {
    const uint64_t off = ((1ull << lvl) - 1) * unit;
    if (off + count * unit > ps[sec].len) throw SetupError(std::string("ptau: section too short for ") + what);
    return ps[sec].off + off;
  };
  PtauRanges pt;
  UVec<uint8_t>&L1 = pt.L1, &L2 = pt.L2, &aL = pt.aL, &bL = pt.bL, &Hs = pt.Hs;
  L1.alloc(n * 64);
  L2.alloc(n * 128);
  aL.alloc(n * 64);
  bL.alloc(n * 64);
  Hs.alloc(2 * n * 64);
  pread_all(fp.fd, L1.data(), L1.size(), level(12, cp, 64, n, "tau*G1 (Lagrange)"), "tau*G1 (Lagrange)");
  pread_all(fp.fd, L2.data(), L2.size(), level(13, cp, 128, n, "tau*G2 (Lagrange)"), "tau*G2 (Lagrange)");
  pread_all(fp.fd, aL.data(), aL.size(), level(14, cp, 64, n, "alpha*tau*G1 (Lagrange)"), "alpha*tau*G1 (Lagrange)");
  pread_all(fp.fd, bL.data(), bL.size(), level(15, cp, 64, n, "beta*tau*G1 (Lagrange)"), "beta*tau*G1 (Lagrange)");
  pread_all(fp.fd, Hs.data(), Hs.size(), level(12, cp + 1, 64, 2 * n, "tau*G1 (Lagrange, 2n)"), "tau*G1 (Lagrange, 2n)");
  uint8_t *alpha1 = pt.alpha1, *beta1 = pt.beta1, *beta2 = pt.beta2;
  if (ps[4].len < 64 || ps[5].len < 64 || ps[6].len < 128) throw SetupError("ptau: alpha / beta sections too short");
  pread_all(fp.fd, alpha1, 64, ps[4].off, "alpha*G1");
  pread_all(fp.fd, beta1, 64, ps[5].off, "beta*G1");
  pread_all(fp.fd, beta2, 128, ps[6].off, "beta*G2");
  host_check_coords(alpha1, 2, "ptau alpha*G1");
  host_check_coords(beta1, 2, "ptau beta*G1");
  host_check_coords(beta2, 4, "ptau beta*G2");
  host_check_coords(Hs.data(), 4 * n, "ptau tau*G1 (Lagrange, 2n)");   // copied into section 9 without touching the device
  return pt;
}

// CSR over (constraint, matrix) of an R1CS, as wtns_check_kernel walks it: row_ptr[3 c + m], signals, coefficients
// (standard form). The three term lists are already grouped by constraint in file order.
struct R1csRows {
  std::vector<uint32_t> row_ptr, sig;
  std::vector<uint8_t> coef;
};
R1csRows r1cs_rows(const R1cs& r) {
  const uint64_t nnz = r.A.size() + r.B.size() + r.C.size();
  if (nnz >= (1ull << 32)) throw SetupError("more than 2^32 coefficients");
  R1csRows out;
  std::vector<uint32_t>&row_ptr = out.row_ptr, &sig = out.sig;
  std::vector<uint8_t>& coef = out.coef;
  row_ptr.assign(3 * (size_t)r.nConstraints + 1, 0);
  sig.resize(nnz);
  coef.resize(nnz * 32);
  {
    size_t ia = 0, ib = 0, ic = 0, t = 0;
    auto take = [&](const UVec<Term>& v, size_t& i, uint32_t c) {
      for (; i < v.size() && v[i].c == c; i++, t++) {
        sig[t] = v[i].s;
        memcpy(&coef[t * 32], v[i].coef, 32);
      }
    };
    for (uint32_t c = 0; c < r.nConstraints; c++) {
      row_ptr[3 * (size_t)c] = (uint32_t)t;
      take(r.A, ia, c);
      row_ptr[3 * (size_t)c + 1] = (uint32_t)t;
      take(r.B, ib, c);
      row_ptr[3 * (size_t)c + 2] = (uint32_t)t;
      take(r.C, ic, c);
    }
    row_ptr[3 * (size_t)r.nConstraints] = (uint32_t)t;
  }
  return out;
}

}  // namespace
