// `snarkjs powersoftau new / contribute / beacon` on the device: making a ceremony file and extending it by one
// contribution (DESIGN.md "Phase-1 transcript"; csrc/phase1.hpp holds the record, the key and the host checks).
//
// snarkjs ptau layout, power p, N = 2^p (as csrc/ptau_verify.hip). A contribution with secrets tau, alpha, beta takes
//   section 2, point i < 2N - 1:  * tau^i        section 3, i < N:  * tau^i
//   section 4, i < N:  * alpha tau^i             section 5, i < N:  * beta tau^i          section 6:  * beta
// Every point meets its own full-width scalar. The scalars are made on the device (power_scalars_kernel: first *
// ratio^(i0 + i), one exponentiation per workgroup, a short one and a chain per thread), the products by
// scalar_mul_each (csrc/ptau_contribute.hip.h: fixed signed 4-bit windows, every lane of a wave on the same path). The
// sections stream through HBM in pieces (csrc/setup_common.hip.h: for_each_piece over the rows of ptau_power_secs, the
// upload through the context's pinned uploader), point checks as `powersoftau prepare phase2` makes them
// (PointChecker::require), scalars, products, the compressed form of the piece into the response hash
// (HashStream, double-buffered pinned staging into the one serial Blake2b), read-back into one of two pinned buffers
// behind the stream's kernels and a writer thread that puts it at its place in the output while the device takes the
// next piece. A second pass over the written sections makes their hash form for nextChallenge, which starts with the
// response hash and so cannot share the first pass. A piece is at most 2^20 points: from power 20 up no section is ever
// whole on the host.
#include "phase1.hpp"
#include "phase2_dev.hip.h"
#include "setup_common.hip.h"
#include "zkpoa_internal.hpp"

using namespace zkpoa;

namespace {

namespace p1 = zkpoa::phase1;
namespace p2 = zkpoa::phase2;

constexpr uint32_t kPowRun = 8;                 // consecutive scalars per thread
constexpr uint32_t kPowBlock = 256 * kPowRun;   // scalars per workgroup

// out[i] = first * ratio^(i0 + i), i < n, standard form. Thread 0 of a workgroup raises ratio to the workgroup's first
// exponent (64 bits: a streamed piece starts anywhere) and shares first * that through LDS; every thread then needs an
// exponent below kPowBlock and a chain of kPowRun products.
static __global__ __launch_bounds__(256) void power_scalars_kernel(Fr first, Fr ratio, uint64_t i0, uint64_t n,
                                                                   void* __restrict__ out) {
  __shared__ uint32_t base[8];
  if (threadIdx.x == 0) {
    const Fr b = first * fr_pow_u64(ratio, i0 + (uint64_t)blockIdx.x * kPowBlock);
#pragma unroll
    for (int k = 0; k < 8; k++) base[k] = b.l[k];
  }
  __syncthreads();
  const uint64_t e0 = (uint64_t)blockIdx.x * kPowBlock + threadIdx.x * kPowRun;
  if (e0 >= n) return;
  Fr t;
#pragma unroll
  for (int k = 0; k < 8; k++) t.l[k] = base[k];
  t = t * fr_pow_u64(ratio, threadIdx.x * kPowRun);
  const uint32_t m = (uint32_t)(n - e0 < kPowRun ? n - e0 : kPowRun);
  char* o = reinterpret_cast<char*>(out) + 32 * e0;
#pragma unroll
  for (uint32_t k = 0; k < kPowRun; k++) {
    if (k < m) {
      store_field(o + 32 * k, t.from_mont());
      t = t * ratio;
    }
  }
}

// enqueued on lane 0's stream; first, ratio: standard form, below r
void power_scalars(zkpoa_context* ctx, const uint8_t first_le[32], const uint8_t ratio_le[32], uint64_t i0, uint64_t n, void* d_out) {
  if (!n) return;
  if (i0 + n < i0) throw SetupError("power scalars: the exponents pass 2^64");
  if (!scalar_in_range(first_le, false) || !scalar_in_range(ratio_le, false)) throw SetupError("power scalars: a scalar is not below r");
  const uint64_t blocks = (n + kPowBlock - 1) / kPowBlock;
  if (blocks >> 31) throw SetupError("power scalars: too many scalars in one call");
  hipLaunchKernelGGL(power_scalars_kernel, dim3((uint32_t)blocks), dim3(256), 0, ctx->dev.lanes[0].stream,
                     fr_dev(HFr::from_bytes(first_le).to_mont()), fr_dev(HFr::from_bytes(ratio_le).to_mont()), i0, n, d_out);
  ZK_HIP(hipGetLastError());
}

// toxic waste does not outlive the command: host copies are overwritten (through a volatile pointer, so that the
// stores stay), the device array of their powers is cleared before it is freed
void wipe(void* p, size_t len) {
  volatile uint8_t* v = static_cast<volatile uint8_t*>(p);
  for (size_t i = 0; i < len; i++) v[i] = 0;
}

// a ceremony file of sections 1-7 whose section 7 has len7 bytes, sized, its table and its header (section 1) written
struct PtauFile : SectionFile {
  static std::array<uint64_t, 7> lens(uint32_t power, uint64_t len7) {
    std::array<uint64_t, 7> l{{4 + 32 + 8, 0, 0, 0, 0, 0, len7}};
    for (const PowerSec& sc : ptau_power_secs(power)) l[sc.id - 1] = sc.bytes();
    return l;
  }
  static constexpr uint32_t kIds[7] = {1, 2, 3, 4, 5, 6, 7};
  PtauFile(const char* path, uint32_t power, uint32_t ceremony, uint64_t len7)
      : SectionFile(path, "ptau", kIds, lens(power, len7).data(), 7) {
    uint8_t s1[44];
    const uint32_t n8 = 32;
    memcpy(s1, &n8, 4);
    memcpy(s1 + 4, HFqParams::P, 32);
    memcpy(s1 + 36, &power, 4);
    memcpy(s1 + 40, &ceremony, 4);
    put(1, s1, 44);
  }
};

void ptau_new(uint32_t power, const char* out_path) {
  if (power < 1 || power > 28) throw SetupError("powersoftau new: power " + std::to_string(power) + " is outside [1, 28]");
  PtauFile fo(out_path, power, power, 4);
  uint8_t g1[64], g2[128];
  h_affine_to_bytes<HFq>(host_generator<HFq>(), g1);
  h_affine_to_bytes<HFq2>(host_generator<HFq2>(), g2);
  constexpr uint64_t kRunPoints = 1u << 14;
  std::vector<uint8_t> run1(64 * kRunPoints), run2(128 * kRunPoints);
  for (uint64_t i = 0; i < kRunPoints; i++) {
    memcpy(&run1[64 * i], g1, 64);
    memcpy(&run2[128 * i], g2, 128);
  }
  for (const PowerSec& sc : ptau_power_secs(power))
    for (uint64_t done = 0; done < sc.count; done += kRunPoints)
      fo.put_at(sc.id, done * sc.unit(), sc.group == 2 ? run2.data() : run1.data(), sc.unit() * std::min<uint64_t>(kRunPoints, sc.count - done));
  const uint32_t zero = 0;
  fo.put(7, &zero, 4);
  fo.commit();
}

void ptau_contribute(zkpoa_context* ctx, const char* in_path, const char* out_path, const uint8_t* secrets_le, const p2::RecordParams& ap) {
  PhaseTimer phase("powersoftau contribute", 34);
  if (same_file(in_path, out_path)) throw SetupError("powersoftau contribute: the output path names the input file");
  MappedFile fi(in_path);   // mapped for the section table and section 7; the point sections stream with pread
  auto ps = bin_sections(fi, "ptau", 1, "ptau");
  const PtauShape shape = ptau_power_sections(fi, ps);
  const uint32_t power = shape.power;
  const uint64_t N = 1ull << power;
  std::vector<p1::Record> records = p1::parse_section7(fi.p + ps[7].off, ps[7].len);
  if (ps.count(12) || ps.count(13) || ps.count(14) || ps.count(15))
    fprintf(stderr, "zkpoa: powersoftau contribute: sections 12-15 (Lagrange form) of the input are dropped: they would be stale; "
                    "run `powersoftau prepare phase2` on the result\n");
  uint8_t challenge[64];
  if (records.empty()) p1::fresh_challenge(power, challenge);
  else memcpy(challenge, records.back().next_challenge, 64);

  // ---- the secrets and the key
  p1::Secrets sec;
  struct WipeSecrets {
    p1::Secrets& s;
    ~WipeSecrets() { wipe(&s, sizeof s); }
  } wipe_sec{sec};
  if (ap.type == 1) {
    p1::beacon_secrets(ap.beacon.data(), ap.beacon.size(), ap.num_iterations_exp, &sec);
  } else {
    for (int k = 0; k < 3; k++) {
      if (secrets_le) memcpy(sec.x[k], secrets_le + 32 * k, 32);
      else random_scalar(sec.x[k]);
    }
    uint8_t s[3][32];
    // ZKPOA_PHASE1_S: "s_tau,s_alpha,s_beta", the s of the key's g1_s = s * G1
    if (!env_scalars("ZKPOA_PHASE1_S", s, 3, "three numbers in [1, r) separated by commas", "the secrets of the contribution key's g1_s"))
      for (int k = 0; k < 3; k++) random_scalar(s[k]);
    uint8_t g1[64];
    h_affine_to_bytes<HFq>(host_generator<HFq>(), g1);
    for (int k = 0; k < 3; k++) p2::mul_wire<HFq>(g1, s[k], sec.g1_s[k]);
    wipe(s, sizeof s);
  }
  for (int k = 0; k < 3; k++)
    if (!scalar_in_range(sec.x[k], true)) throw SetupError("powersoftau contribute: tau, alpha and beta must be in [1, r)");
  p1::Record rec;
  static_cast<p2::RecordParams&>(rec) = ap;
  p1::make_key(sec, challenge, rec.key);
  phase("sections, challenge, key");

  // ---- pass 1: the new sections, their compressed form into the response hash
  constexpr uint64_t kMaxPiece = 1ull << 20;   // 2 x 128 MiB of pinned read-back buffers; from power 20 up no section is whole on the host
  uint64_t piece = (uint64_t)ctx->opt_ptau_piece_points;
  if (!piece) piece = piece_from_free_hbm(128 + 128 + 32 + 256, 1ull << 12, kMaxPiece);   // a piece's points, results, scalars and XYZZ scratch
  piece = std::min<uint64_t>(std::min<uint64_t>(piece, kMaxPiece), 2 * N);
  PtauFile fo(out_path, power, shape.ceremony, ps[7].len + p1::kRecordHead + rec.len());
  hipStream_t st = ctx->dev.lanes[0].stream;
  PointChecker points(ctx);
  const uint64_t slab = (uint64_t)ctx->opt_ptau_mul_slab;
  DevBuf d_in(piece * 128), d_out(piece * 128), d_k(piece * 32), d_flag(64),
      d_scratch(std::max(scalar_mul_each_scratch_g1(piece, slab), scalar_mul_each_scratch_g2(piece, slab)));   // once per command
  struct WipeScalars {   // the powers of the secrets
    DevBuf& k;
    size_t len;
    ~WipeScalars() { (void)hipMemset(k.p, 0, len); }
  } wipe_k{d_k, (size_t)piece * 32};
  ZK_HIP(hipMemsetAsync(d_flag.p, 0, 64, st));
  p2::Blake2b resp;
  resp.update(challenge, 64);
  uint8_t one[32] = {1};
  // point i of section 2 + t takes first[t] * ratio[t]^i
  const uint8_t* const first[5] = {one, one, sec.x[1], sec.x[2], sec.x[2]};
  const uint8_t* const ratio[5] = {sec.x[0], sec.x[0], sec.x[0], sec.x[0], one};
  double read_ms = 0, compute_ms = 0, hash_ms = 0;
  // Read-back: piece p comes back into pinned buffer p & 1 behind the stream's kernels, and a writer thread puts it into
  // the file when its copy has landed -- while the device takes piece p + 1. A buffer is reused when its writer is done.
  struct ReadBack {
    uint8_t* pinned[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    std::thread writer[2];
    std::atomic<bool> failed{false};
    double write_ms[2] = {0, 0};   // each touched by its own writer only
    explicit ReadBack(size_t bytes) {
      for (int b = 0; b < 2; b++) {
        ZK_HIP(hipHostMalloc((void**)&pinned[b], bytes, hipHostMallocDefault));
        ZK_HIP(hipEventCreateWithFlags(&ev[b], hipEventDisableTiming));
      }
    }
    void wait(int b) {
      if (writer[b].joinable()) writer[b].join();
    }
    ~ReadBack() {
      for (int b = 0; b < 2; b++) {
        wait(b);
        if (ev[b]) (void)hipEventDestroy(ev[b]);
        if (pinned[b]) (void)hipHostFree(pinned[b]);
      }
    }
  } rb(piece * 128);
  {
    HashStream hs(ctx, resp, 0);
    uint64_t p = 0;
    for (const PowerSec& j : ptau_power_secs(power)) {
      const uint64_t unit = j.unit();
      const std::string what = "ptau section " + std::to_string(j.id);
      for_each_piece(ctx, fi.fd, ps[j.id].off, j.count, unit, piece, d_in.p, [&](uint64_t i0, uint64_t cnt) {
        const int b = (int)(p++ & 1);
        auto t0 = std::chrono::steady_clock::now();
        points.require(d_in.p, cnt, j.group, j.group == 2, what.c_str());
        power_scalars(ctx, first[j.id - 2], ratio[j.id - 2], i0, cnt, d_k.p);
        if (j.group == 2) scalar_mul_each_g2(ctx, d_in.p, d_k.p, cnt, d_out.p, (uint32_t*)d_flag.p, d_scratch.p, slab);
        else scalar_mul_each_g1(ctx, d_in.p, d_k.p, cnt, d_out.p, (uint32_t*)d_flag.p, d_scratch.p, slab);
        ZK_HIP(hipStreamSynchronize(st));
        compute_ms += ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        hs.points(d_out.p, cnt, j.group, false, true);
        hash_ms += ms_since(t0);
        rb.wait(b);
        ZK_HIP(hipMemcpyAsync(rb.pinned[b], d_out.p, cnt * unit, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipEventRecord(rb.ev[b], st));
        const uint32_t id = j.id;
        const uint64_t at = i0 * unit, len = cnt * unit;
        const int device = ctx->dev.device;
        rb.writer[b] = std::thread([&rb, &fo, b, id, at, len, device] {
          const auto w0 = std::chrono::steady_clock::now();
          if (hipSetDevice(device) != hipSuccess || hipEventSynchronize(rb.ev[b]) != hipSuccess) {
            rb.failed = true;
            return;
          }
          fo.put_at(id, at, rb.pinned[b], len);
          rb.write_ms[b] += ms_since(w0);
        });
      }, &read_ms);
    }
    rb.wait(0);
    rb.wait(1);
    if (rb.failed) throw SetupError("powersoftau contribute: the read-back of a piece failed");
  }
  const double write_ms = rb.write_ms[0] + rb.write_ms[1];
  {
    uint32_t bad = 0;
    ZK_HIP(hipMemcpy(&bad, d_flag.p, 4, hipMemcpyDeviceToHost));
    if (bad) throw SetupError("powersoftau contribute: internal: a scalar was not below r");
  }
  p1::blake2b_save(resp, rec.partial);
  p1::hash_key(resp, rec.key);
  uint8_t response[64];
  resp.final(response);

  // ---- pass 2: nextChallenge = Blake2b(response hash | hash form of the new sections 2-6), from the written file
  struct ReadFd {   // the output is open for writing only: its bytes are read back through a descriptor of their own
    int fd;
    ~ReadFd() {
      if (fd >= 0) close(fd);
    }
  } out_r{open(fo.file.tmp.c_str(), O_RDONLY | O_CLOEXEC)};
  if (out_r.fd < 0) throw SetupError("powersoftau contribute: cannot read the output back");
  const int out_fd = out_r.fd;
  {
    auto t0 = std::chrono::steady_clock::now();
    p2::Blake2b next;
    next.update(response, 64);
    HashStream hs(ctx, next, 0);
    hash_form_ptau_sections(ctx, hs, out_fd, fo.secs, power, d_in.p, piece);
    next.final(rec.next_challenge);
    hash_ms += ms_since(t0);
  }
  auto back = [&](uint32_t sec, uint64_t point, uint64_t unit, uint8_t* dst) {
    if (pread(out_fd, dst, unit, (off_t)(fo.off(sec) + point * unit)) != (ssize_t)unit) throw SetupError("powersoftau contribute: cannot read the output back");
  };
  back(2, 1, 64, rec.tau_g1);
  back(3, 1, 128, rec.tau_g2);
  back(4, 0, 64, rec.alpha_g1);
  back(5, 0, 64, rec.beta_g1);
  back(6, 0, 128, rec.beta_g2);
  records.push_back(rec);
  const std::vector<uint8_t> s7 = p1::write_section7(records);
  fo.put(7, s7.data(), s7.size());
  fo.commit();
  if (phase.verbose) {
    const char* what[4] = {"read (file -> HBM)", "compute (checks, scalars, products)", "hashes (response, nextChallenge)", "write (HBM -> file; overlaps the rest)"};
    const double ms[4] = {read_ms, compute_ms, hash_ms, write_ms};
    for (int i = 0; i < 4; i++) fprintf(stderr, "zkpoa: %s: %-*s %8.1f ms\n", phase.command, phase.width, what[i], ms[i]);
  }
  phase("sections 2-7 written, file renamed into place");
}

}  // namespace

extern "C" int zkpoa_scalar_mul_each_device(zkpoa_context* ctx, int group, const void* d_points, const void* d_scalars,
                                            uint64_t n, void* d_out) {
  ZK_API_BEGIN(ctx)
  if (group != 1 && group != 2) throw SetupError("scalar_mul_each: group must be 1 (G1) or 2 (G2)");
  if (n && (!d_points || !d_scalars || !d_out)) throw SetupError("scalar_mul_each: null pointer");
  const uint64_t slab = (uint64_t)ctx->opt_ptau_mul_slab;
  DevBuf flag(64), scratch(group == 2 ? scalar_mul_each_scratch_g2(n, slab) : scalar_mul_each_scratch_g1(n, slab));
  ZK_HIP(hipMemsetAsync(flag.p, 0, 64, ctx->dev.lanes[0].stream));
  if (group == 2) scalar_mul_each_g2(ctx, d_points, d_scalars, n, d_out, (uint32_t*)flag.p, scratch.p, slab);
  else scalar_mul_each_g1(ctx, d_points, d_scalars, n, d_out, (uint32_t*)flag.p, scratch.p, slab);
  ZK_HIP(hipStreamSynchronize(ctx->dev.lanes[0].stream));
  ZK_HIP(hipGetLastError());
  uint32_t bad = 0;
  ZK_HIP(hipMemcpy(&bad, flag.p, 4, hipMemcpyDeviceToHost));
  if (bad) throw SetupError("scalar_mul_each: a scalar is not below r");
  ZK_API_END(ctx)
}

extern "C" int zkpoa_power_scalars_device(zkpoa_context* ctx, const uint8_t first_le[32], const uint8_t ratio_le[32],
                                          uint64_t i0, uint64_t n, void* d_out) {
  ZK_API_BEGIN(ctx)
  if (!first_le || !ratio_le || (n && !d_out)) throw SetupError("power scalars: null argument");
  power_scalars(ctx, first_le, ratio_le, i0, n, d_out);
  ZK_HIP(hipStreamSynchronize(ctx->dev.lanes[0].stream));
  ZK_HIP(hipGetLastError());
  ZK_API_END(ctx)
}

extern "C" int zkpoa_compressed_form(zkpoa_context* ctx, int group, const void* points, uint64_t n, uint64_t piece_points,
                                     void* out_bytes, uint8_t digest[64]) {
  ZK_API_BEGIN(ctx)
  points_form(ctx, group, points, n, piece_points, true, out_bytes, digest);
  ZK_API_END(ctx)
}

extern "C" int zkpoa_ptau_new(zkpoa_context* ctx, uint32_t power, const char* out_path) {
  ZK_API_BEGIN(ctx)
  if (!out_path) throw SetupError("powersoftau new: null path");
  ptau_new(power, out_path);
  ZK_API_END(ctx)
}

extern "C" int zkpoa_ptau_contribute(zkpoa_context* ctx, const char* in_path, const char* out_path, const uint8_t* secrets_le,
                                     const char* name) {
  ZK_API_BEGIN(ctx)
  if (!in_path || !out_path) throw SetupError("powersoftau contribute: null path");
  p2::RecordParams ap;
  ap.name = name ? name : "";
  ap.check("powersoftau contribute");
  ptau_contribute(ctx, in_path, out_path, secrets_le, ap);
  ZK_API_END(ctx)
}

extern "C" int zkpoa_ptau_beacon(zkpoa_context* ctx, const char* in_path, const char* out_path, const uint8_t* beacon,
                                 unsigned long beacon_len, uint32_t num_iterations_exp, const char* name) {
  ZK_API_BEGIN(ctx)
  if (!in_path || !out_path || (!beacon && beacon_len)) throw SetupError("powersoftau beacon: null argument");
  p2::RecordParams ap;
  ap.type = 1;
  ap.name = name ? name : "";
  ap.beacon.assign(beacon, beacon + beacon_len);
  ap.num_iterations_exp = num_iterations_exp;
  ap.check("powersoftau beacon");
  ptau_contribute(ctx, in_path, out_path, nullptr, ap);
  ZK_API_END(ctx)
}

// host only: the records of section 7, one line "<type> <name> <response hash>" each
extern "C" int zkpoa_ptau_contributions(const char* ptau_path, uint32_t* count, char* text, unsigned long cap) {
  try {
    if (!ptau_path || !count) return PROVER_ERROR;
    MappedFile fp(ptau_path);
    auto ps = bin_sections(fp, "ptau", 1, "ptau");
    if (!ps.count(7)) return PROVER_ERROR;
    const std::vector<p1::Record> records = p1::parse_section7(fp.p + ps[7].off, ps[7].len);
    *count = (uint32_t)records.size();
    std::string out;
    for (const auto& r : records) {
      uint8_t h[64];
      char hex[129] = "-";
      if (p1::response_hash(r.partial, r.key, h))
        for (int i = 0; i < 64; i++) snprintf(hex + 2 * i, 3, "%02x", h[i]);
      out += std::string(r.type == 1 ? "beacon " : "contribution ") + r.name + " " + hex + "\n";
    }
    if (text && cap) zkpoa::set_err(text, cap, out);
    return PROVER_OK;
  } catch (const std::exception&) {
    return PROVER_ERROR;
  }
}

extern "C" int zkpoa_blake2b_state(void* state, uint8_t out[216]) {
  if (!state || !out) return PROVER_ERROR;
  p1::blake2b_save(*static_cast<p2::Blake2b*>(state), out);
  return PROVER_OK;
}
extern "C" void* zkpoa_blake2b_restore(const uint8_t saved[216]) {
  if (!saved) return nullptr;
  p2::Blake2b* b = new p2::Blake2b();
  if (!p1::blake2b_restore(saved, b)) {
    delete b;
    return nullptr;
  }
  return b;
}
