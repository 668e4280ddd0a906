// `snarkjs powersoftau new / contribute / beacon / export challenge / challenge contribute / import response` on the
// device: making a ceremony file, extending it by one contribution, and the same contribution by somebody who never holds
// the file (DESIGN.md "Phase-1 transcript", "Challenge and response files"; csrc/phase1.hpp: the record, the key, the host
// checks; csrc/ptau_file.hip.h: the file as it is opened and written; csrc/ptau_response.hip: back into wire form).
//
// snarkjs ptau layout, power p, N = 2^p (as csrc/ptau_verify.hip). A contribution with secrets tau, alpha, beta takes
//   section 2, point i < 2N - 1:  * tau^i        section 3, i < N:  * tau^i
//   section 4, i < N:  * alpha tau^i             section 5, i < N:  * beta tau^i          section 6:  * beta
// Every point meets its own full-width scalar: made on the device (power_scalars_kernel), multiplied by scalar_mul_each
// (csrc/ptau_contribute.hip.h). The sections stream through HBM in pieces of at most 2^20 points (for_each_piece of
// csrc/setup_common.hip.h: from power 20 up no section is ever whole on the host). The four streaming commands are made of
// the same parts: PtauInput; MulStep (point checks, scalars, products); HashStream (a piece's compressed or hash form into
// the one serial Blake2b) with HashedWriter where the hashed bytes are the output; ReadBack (a writer thread per pinned
// buffer puts a piece into the output while the device takes the next); close_record (a second pass over the written
// sections: nextChallenge starts with the response hash and so cannot share the first) and append_record.
#include "phase2_dev.hip.h"
#include "ptau_file.hip.h"
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

// ---- the parts the streaming commands are made of ------------------------------------------------------------------------
struct WipedSecrets : p1::Secrets {   // a command's secrets cannot be held without their wipe
  ~WipedSecrets() { wipe(static_cast<p1::Secrets*>(this), sizeof(p1::Secrets)); }
};
// tau, alpha, beta and the g1_s of their keys: a beacon's generator (type 1), else secrets_le (NULL: /dev/urandom) and
// ZKPOA_PHASE1_S ("s_tau,s_alpha,s_beta", the s of g1_s = s * G1) or /dev/urandom
void draw_secrets(const p2::RecordParams& ap, const uint8_t* secrets_le, const char* what, p1::Secrets& sec) {
  if (ap.type == 1) {
    p1::beacon_secrets(ap.beacon.data(), ap.beacon.size(), ap.num_iterations_exp, &sec);
  } else {
    for (int k = 0; k < 3; k++) {
      if (secrets_le) memcpy(sec.x[k], secrets_le + 32 * k, 32);
      else random_scalar(sec.x[k]);
    }
    uint8_t s[3][32];
    if (!env_scalars(O_PHASE1_S, s, 3, "three numbers in [1, r) separated by commas", "the secrets of the contribution key's g1_s"))
      for (int k = 0; k < 3; k++) random_scalar(s[k]);
    uint8_t g1[64];
    h_affine_to_bytes<HFq>(host_generator<HFq>(), g1);
    for (int k = 0; k < 3; k++) p2::mul_wire<HFq>(g1, s[k], sec.g1_s[k]);
    wipe(s, sizeof s);
  }
  for (int k = 0; k < 3; k++)
    if (!scalar_in_range(sec.x[k], true)) throw SetupError(std::string(what) + ": tau, alpha and beta must be in [1, r)");
}
constexpr uint64_t kMulBytesPerPoint = 128 + 128 + 32 + 256;   // a piece's points (the caller's), results, scalars and XYZZ scratch
// The multiply step of a contribution, once per command: point i of section 2 + t times first[t] * ratio[t]^i. The
// powers of the secrets (d_k) are cleared on the device by the destructor's body, which runs before any member is
// destroyed: d_k still owns their memory then and is freed after it, on every exit path, exceptions included.
struct MulStep {
  zkpoa_context* ctx;
  const std::string command;
  const uint64_t slab;
  PointChecker points;
  const uint8_t one[32] = {1};
  const uint8_t *const first[5], *const ratio[5];   // into `one` and the caller's secrets
  DevBuf d_out, d_flag, d_scratch, d_k;   // a piece's products; the "scalar not below r" word; XYZZ scratch; the scalars
  const size_t k_bytes;
  MulStep(zkpoa_context* c, uint64_t piece, const char* cmd, const p1::Secrets& sec)
      : ctx(c), command(cmd), slab((uint64_t)c->opt_ptau_mul_slab), points(c),
        first{one, one, sec.x[1], sec.x[2], sec.x[2]}, ratio{sec.x[0], sec.x[0], sec.x[0], sec.x[0], one},
        d_out(piece * 128), d_flag(64), d_scratch(std::max(scalar_mul_each_scratch(1, piece, slab), scalar_mul_each_scratch(2, piece, slab))),
        d_k(piece * 32), k_bytes((size_t)piece * 32) {
    ZK_HIP(hipMemsetAsync(d_flag.p, 0, 64, ctx->dev.lanes[0].stream));
  }
  ~MulStep() { (void)hipMemset(d_k.p, 0, k_bytes); }
  // d_out = the products of the cnt points at d_in (wire form, checked here: `what` names them); the stream is idle on return
  void run(const PowerSec& j, const void* d_in, uint64_t i0, uint64_t cnt, const char* what) {
    points.require(d_in, cnt, j.group, j.group == 2, what);
    power_scalars(ctx, first[j.id - 2], ratio[j.id - 2], i0, cnt, d_k.p);
    scalar_mul_each(ctx, j.group, d_in, d_k.p, cnt, d_out.p, (uint32_t*)d_flag.p, d_scratch.p, slab);
    ZK_HIP(hipStreamSynchronize(ctx->dev.lanes[0].stream));
  }
  void finish() {   // after the last piece
    uint32_t bad = 0;
    ZK_HIP(hipMemcpy(&bad, d_flag.p, 4, hipMemcpyDeviceToHost));
    if (bad) throw SetupError(command + ": internal: a scalar was not below r");
  }
};
// Read-back: piece p comes back into pinned buffer p & 1 behind the stream's kernels, and a writer thread puts it into
// the file when its copy has landed -- while the device takes piece p + 1. A buffer is reused when its writer is done.
struct ReadBack {
  PinnedMem pinned[2];
  DevEvent ev[2];
  SideTask writer[2];
  bool failed = false;   // a writer threw: kept here, its slot takes the next piece
  double write_ms[2] = {0, 0};   // each touched by its own writer only
  zkpoa_context* ctx;
  uint64_t sent = 0;
  ReadBack(zkpoa_context* c, size_t bytes) : ctx(c) {
    for (int b = 0; b < 2; b++) {
      pinned[b].alloc(bytes);
      ev[b].create(hipEventDisableTiming);
    }
  }
  void wait(int b) noexcept {
    try {
      writer[b].get();
    } catch (...) {
      failed = true;
    }
  }
  // len bytes at d_src, behind what lane 0's stream holds, to byte `at` of section id of fo
  void send(const void* d_src, uint64_t len, SectionFile& fo, uint32_t id, uint64_t at) {
    const int b = (int)(sent++ & 1), device = ctx->dev.device;
    hipStream_t st = ctx->dev.lanes[0].stream;
    wait(b);
    ZK_HIP(hipMemcpyAsync(pinned[b].get(), d_src, len, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipEventRecord(ev[b], st));
    writer[b] = SideTask([this, &fo, b, id, at, len, device] {
      const auto w0 = std::chrono::steady_clock::now();
      ZK_HIP(hipSetDevice(device));
      ZK_HIP(hipEventSynchronize(ev[b]));
      fo.put_at(id, at, pinned[b].get(), len);
      write_ms[b] += ms_since(w0);
    });
  }
  void finish(const std::string& command) {   // after the last piece: every writer done, or the command fails
    wait(0);
    wait(1);
    if (failed) throw SetupError(command + ": the read-back of a piece failed");
  }
  ~ReadBack() {   // the writers are done before the buffers and events they read go
    wait(0);
    wait(1);
  }
};

// The record of the sections just written, closed: rec->next_challenge = Blake2b(response hash | hash form of the new
// sections 2-6) and the record's five points, from the file as written (a second pass through d_piece, piece x 128 B of
// device memory). An output is open for writing only (AtomicFile): its bytes are read through a descriptor of their own.
void close_record(zkpoa_context* ctx, const PtauFile& fo, const uint8_t response[64], void* d_piece, uint64_t piece,
                  const std::string& command, p1::Record* rec) {
  struct ReadFd {
    int fd;
    ~ReadFd() {
      if (fd >= 0) close(fd);
    }
  } out{open(fo.file.tmp.c_str(), O_RDONLY | O_CLOEXEC)};
  if (out.fd < 0) throw SetupError(command + ": cannot read the output back");
  p2::Blake2b next;
  next.update(response, 64);
  HashStream hs(ctx, next, 0);
  hash_form_ptau_sections(ctx, hs, out.fd, fo.secs, fo.power, d_piece, piece);
  next.final(rec->next_challenge);
  auto back = [&](uint32_t sec, uint64_t point, uint64_t unit, uint8_t* dst) {
    if (pread(out.fd, dst, unit, (off_t)(fo.off(sec) + point * unit)) != (ssize_t)unit) throw SetupError(command + ": cannot read the output back");
  };
  back(2, 1, 64, rec->tau_g1);
  back(3, 1, 128, rec->tau_g2);
  back(4, 0, 64, rec->alpha_g1);
  back(5, 0, 64, rec->beta_g1);
  back(6, 0, 128, rec->beta_g2);
}
// the closed record after the input's, section 7 written, the file renamed into place
void append_record(PtauFile& fo, std::vector<p1::Record>& records, const p1::Record& rec) {
  records.push_back(rec);
  const std::vector<uint8_t> s7 = p1::write_section7(records);
  fo.put(7, s7.data(), s7.size());
  fo.commit();
}

template <class Fn>
void timed(double& ms, Fn fn) {   // ms += the host's time in fn
  const auto t0 = std::chrono::steady_clock::now();
  fn();
  ms += ms_since(t0);
}
void verbose_split(const PhaseTimer& phase, std::initializer_list<std::pair<const char*, double>> parts) {
  if (!phase.verbose) return;
  for (const auto& p : parts) fprintf(stderr, "zkpoa: %s: %-*s %8.1f ms\n", phase.command, phase.width, p.first, p.second);
}
// A command that also writes what it hashes (HashStream::sink): each hashed piece, in order, at a running offset of fo
struct HashedWriter {
  AtomicFile& fo;
  uint64_t at;
  double write_ms = 0;   // inside the stream's hash_ms
  void operator()(const uint8_t* p, uint64_t len) {
    timed(write_ms, [&] { fo.put_at(at, p, len); });
    at += len;
  }
};

void ptau_contribute(zkpoa_context* ctx, const char* in_path, const char* out_path, const uint8_t* secrets_le, const p2::RecordParams& ap) {
  PhaseTimer phase("powersoftau contribute", 34);
  if (same_file(in_path, out_path)) throw SetupError("powersoftau contribute: the output path names the input file");
  PtauInput in(in_path);
  const uint32_t power = in.shape.power;
  in.warn_lagrange_dropped(phase.command);
  uint8_t challenge[64];
  p1::trail_challenge(in.records, power, challenge);

  // ---- the secrets and the key
  WipedSecrets sec;
  draw_secrets(ap, secrets_le, phase.command, sec);
  p1::Record rec{ap};
  p1::make_key(sec, challenge, rec.key);
  phase("sections, challenge, key");

  // ---- pass 1: the new sections, their compressed form into the response hash
  const uint64_t piece = ptau_piece(ctx, 1ull << power, kMulBytesPerPoint);
  // fo before rb: rb is destroyed first, and its destructor joins the writer threads, which write into fo -- also when
  // an exception leaves the piece loop
  PtauFile fo(out_path, power, in.shape.ceremony, in.ps[7].len + p1::kRecordHead + rec.len());
  DevBuf d_in(piece * 128);
  MulStep mul(ctx, piece, phase.command, sec);   // once per command
  p2::Blake2b resp;
  resp.update(challenge, 64);
  double read_ms = 0, compute_ms = 0, hash_ms = 0;
  ReadBack rb(ctx, piece * 128);
  {
    HashStream hs(ctx, resp, 0);
    for (const PowerSec& j : ptau_power_secs(power)) {
      const std::string what = "ptau section " + std::to_string(j.id);
      for_each_piece(ctx, in.f.fd, in.ps[j.id].off, j.count, j.unit(), piece, d_in.p, [&](uint64_t i0, uint64_t cnt) {
        timed(compute_ms, [&] { mul.run(j, d_in.p, i0, cnt, what.c_str()); });
        timed(hash_ms, [&] { hs.points(mul.d_out.p, cnt, j.group, false, true); });
        rb.send(mul.d_out.p, cnt * j.unit(), fo, j.id, i0 * j.unit());
      }, &read_ms);
    }
    rb.finish(phase.command);
  }
  mul.finish();
  p1::blake2b_save(resp, rec.partial);
  p1::hash_key(resp, rec.key);
  uint8_t response[64];
  resp.final(response);

  // ---- pass 2: nextChallenge from the written file, the record, section 7
  timed(hash_ms, [&] { close_record(ctx, fo, response, d_in.p, piece, phase.command, &rec); });
  append_record(fo, in.records, rec);
  verbose_split(phase, {{"read (file -> HBM)", read_ms}, {"compute (checks, scalars, products)", compute_ms},
                        {"hashes (response, nextChallenge)", hash_ms}, {"write (HBM -> file; overlaps the rest)", rb.write_ms[0] + rb.write_ms[1]}});
  phase("sections 2-7 written, file renamed into place");
}

// ---- challenge and response files (DESIGN.md "Phase-1 transcript", "Challenge and response files") ----------------------
// challenge: 64 B (the last response hash) | hash form of sections 2-6;  response: 64 B (the challenge) | compressed form
// of the new sections 2-6 | the key's nine points in hash form
uint64_t challenge_file_bytes(uint32_t power) {
  uint64_t n = 64;
  for (const PowerSec& sc : ptau_power_secs(power)) n += sc.bytes();
  return n;
}
uint64_t response_file_bytes(uint32_t power) { return 64 + (challenge_file_bytes(power) - 64) / 2 + p1::kKeyLen; }

// `powersoftau export challenge`: the hash form that a challenge covers, written out as well as hashed
void ptau_export_challenge(zkpoa_context* ctx, const char* in_path, const char* out_path, uint8_t challenge_hash[64]) {
  PhaseTimer phase("powersoftau export challenge", 40);
  if (same_file(in_path, out_path)) throw SetupError("powersoftau export challenge: the output path names the input file");
  PtauInput in(in_path);
  const uint32_t power = in.shape.power;
  uint8_t want[64], last_response[64];
  p1::trail_challenge(in.records, power, want);
  if (!p1::trail_response(in.records, last_response))
    throw SetupError("powersoftau export challenge: the last record's partialHash is no Blake2b state");
  AtomicFile fo(out_path);
  fo.reserve(challenge_file_bytes(power));
  fo.put_at(0, last_response, 64);
  const uint64_t piece = ptau_piece(ctx, 1ull << power, 128);
  DevBuf d_piece(piece * 128);
  p2::Blake2b h;
  h.update(last_response, 64);
  double read_ms = 0;
  HashedWriter out{fo, 64};
  phase("sections, records");
  {
    HashStream hs(ctx, h, 0);
    hs.sink = std::ref(out);
    hash_form_ptau_sections(ctx, hs, in.f.fd, in.ps, power, d_piece.p, piece, &read_ms);
    verbose_split(phase, {{"read (file -> HBM)", read_ms}, {"convert (waiting for the device)", hs.convert_ms},
                          {"hash (Blake2b)", hs.hash_ms - out.write_ms}, {"write (challenge file)", out.write_ms}});
  }
  uint8_t got[64];
  h.final(got);
  if (out.at != challenge_file_bytes(power)) throw SetupError("powersoftau export challenge: internal: the challenge has an unexpected size");
  if (memcmp(got, want, 64))
    throw SetupError("powersoftau export challenge: the hash of sections 2-6 is not the file's challenge: they are not the sections "
                     "its last record describes (a file without records must hold the generators)");
  fo.commit();
  if (challenge_hash) memcpy(challenge_hash, got, 64);
  phase("challenge written, file renamed into place");
}

// `powersoftau challenge contribute`: `powersoftau contribute` without the ceremony file. The challenge is the hash of
// the whole input and opens both the response and its hash, so the input is hashed in a pass of its own (host, from the
// mapping) before the pass that converts, multiplies, compresses, hashes and writes.
void ptau_challenge_contribute(zkpoa_context* ctx, const char* in_path, const char* out_path, const uint8_t* secrets_le,
                               uint8_t response_hash[64]) {
  PhaseTimer phase("powersoftau challenge contribute", 40);
  if (same_file(in_path, out_path)) throw SetupError("powersoftau challenge contribute: the output path names the input file");
  MappedFile fi(in_path);
  nonempty(fi);
  uint32_t power = 1;
  while (power <= 28 && challenge_file_bytes(power) != fi.size) power++;
  if (power > 28) throw SetupError("powersoftau challenge contribute: a file of " + std::to_string(fi.size) + " bytes is no challenge of a power in [1, 28]");
  uint8_t challenge[64];
  {
    p2::Blake2b h;
    for (uint64_t done = 0; done < fi.size; done += 64ull << 20) h.update(fi.p + done, std::min<uint64_t>(64ull << 20, fi.size - done));
    h.final(challenge);
  }
  phase("challenge (Blake2b of the input)");
  WipedSecrets sec;
  draw_secrets(p2::RecordParams{}, secrets_le, phase.command, sec);
  uint8_t key[p1::kKeyLen];
  p1::make_key(sec, challenge, key);
  phase("key");

  const uint64_t piece = ptau_piece(ctx, 1ull << power, 128 + kMulBytesPerPoint);   // and the piece in hash form
  AtomicFile fo(out_path);
  fo.reserve(response_file_bytes(power));
  fo.put_at(0, challenge, 64);
  FormConverter conv(ctx);
  DevBuf d_raw(piece * 128), d_in(piece * 128);
  MulStep mul(ctx, piece, phase.command, sec);
  p2::Blake2b resp;
  resp.update(challenge, 64);
  double read_ms = 0, convert_ms = 0, compute_ms = 0, hash_ms = 0;
  HashedWriter out{fo, 64};
  uint64_t in_off = 64;
  {
    HashStream hs(ctx, resp, 0);
    hs.sink = std::ref(out);
    for (const PowerSec& j : ptau_power_secs(power)) {
      const std::string what = "powersoftau challenge contribute: section " + std::to_string(j.id);
      for_each_piece(ctx, fi.fd, in_off, j.count, j.unit(), piece, d_raw.p, [&](uint64_t i0, uint64_t cnt) {
        timed(convert_ms, [&] {
          conv.convert(false, j.group, d_raw.p, cnt, d_in.p);
          conv.require(i0, what.c_str());
        });
        timed(compute_ms, [&] { mul.run(j, d_in.p, i0, cnt, what.c_str()); });
        timed(hash_ms, [&] { hs.points(mul.d_out.p, cnt, j.group, false, true); });
      }, &read_ms);
      in_off += j.bytes();
    }
  }
  mul.finish();
  uint8_t key_form[p1::kKeyLen];
  for (int i = 0; i < 6; i++) p2::g1_hash_form(h_affine_from_bytes<HFq>(key + 64 * i), key_form + 64 * i);
  for (int i = 0; i < 3; i++) p2::g2_hash_form(h_affine_from_bytes<HFq2>(key + 384 + 128 * i), key_form + 384 + 128 * i);
  resp.update(key_form, sizeof key_form);
  fo.put_at(out.at, key_form, sizeof key_form);
  if (out.at + sizeof key_form != response_file_bytes(power)) throw SetupError("powersoftau challenge contribute: internal: the response has an unexpected size");
  uint8_t response[64];
  resp.final(response);
  fo.commit();
  if (response_hash) memcpy(response_hash, response, 64);
  verbose_split(phase, {{"read (file -> HBM)", read_ms}, {"convert (hash form -> wire form)", convert_ms},
                        {"compute (checks, scalars, products)", compute_ms}, {"hash (compressed form, Blake2b)", hash_ms - out.write_ms},
                        {"write (response file)", out.write_ms}});
  phase("response written, file renamed into place");
}

// `powersoftau import response`: the response's sections decompressed and checked as `prepare phase2` checks points, written
// as sections 2-6 of the new file; the record from the response's bytes and the new sections; the record checked against
// the old file's trail as `powersoftau verify` checks a last record. That the sections are powers is left to `verify`.
void ptau_import_response(zkpoa_context* ctx, const char* old_path, const char* resp_path, const char* new_path,
                          const p2::RecordParams& ap) {
  PhaseTimer phase("powersoftau import response", 40);
  if (same_file(old_path, new_path) || same_file(resp_path, new_path))
    throw SetupError("powersoftau import response: the output path names an input file");
  PtauInput in(old_path);
  const uint32_t power = in.shape.power;
  in.warn_lagrange_dropped(phase.command);
  p1::Trail trail;
  if (!p1::trail_end(in.records, power, &trail))
    throw SetupError("powersoftau import response: a point of the old file's last record is not a point of its group");
  MappedFile fr(resp_path);
  nonempty(fr);
  if (fr.size != response_file_bytes(power))
    throw SetupError("powersoftau import response: a response to a challenge of power " + std::to_string(power) + " has " +
                     std::to_string(response_file_bytes(power)) + " bytes, this file has " + std::to_string(fr.size));
  if (memcmp(fr.p, trail.challenge, 64)) throw SetupError("powersoftau import response: the response answers another challenge than the old file's");
  p1::Record rec{ap};
  const uint8_t* key_form = fr.p + fr.size - p1::kKeyLen;
  for (int i = 0; i < 9; i++) {
    const bool ok = i < 6 ? p2::g1_from_hash_form(key_form + 64 * i, rec.key + 64 * i)
                          : p2::g2_from_hash_form(key_form + 384 + 128 * (i - 6), rec.key + 384 + 128 * (i - 6));
    if (!ok) throw SetupError("powersoftau import response: point " + std::to_string(i) + " of the key is not in hash form (a coordinate not below q, or a flag bit)");
  }
  phase("old file, response, key");

  // ---- pass 1: the response's sections into the new file; their bytes into the response hash
  const uint64_t piece = ptau_piece(ctx, 1ull << power, 64 + 128);   // a piece compressed and in wire form
  PtauFile fo(new_path, power, in.shape.ceremony, in.ps[7].len + p1::kRecordHead + rec.len());   // before rb, as in ptau_contribute
  PointChecker points(ctx);
  FormConverter conv(ctx);
  DevBuf d_raw(piece * 64), d_pts(piece * 128);
  ReadBack rb(ctx, piece * 128);
  p2::Blake2b resp;
  resp.update(fr.p, 64);
  double read_ms = 0, decompress_ms = 0, check_ms = 0, hash_ms = 0;
  uint64_t off = 64;
  for (const PowerSec& j : ptau_power_secs(power)) {
    const uint64_t unit = j.unit(), in_unit = unit / 2;
    const std::string what = "powersoftau import response: section " + std::to_string(j.id);
    for_each_piece(ctx, fr.fd, off, j.count, in_unit, piece, d_raw.p, [&](uint64_t i0, uint64_t cnt) {
      timed(hash_ms, [&] {
        conv.convert(true, j.group, d_raw.p, cnt, d_pts.p);
        resp.update(fr.p + off + i0 * in_unit, cnt * in_unit);   // the host hashes while the device takes the roots
      });
      timed(decompress_ms, [&] { conv.require(i0, what.c_str()); });
      timed(check_ms, [&] { points.require(d_pts.p, cnt, j.group, j.group == 2, what.c_str()); });
      rb.send(d_pts.p, cnt * unit, fo, j.id, i0 * unit);
    }, &read_ms);
    off += j.count * in_unit;
  }
  rb.finish(phase.command);
  p1::blake2b_save(resp, rec.partial);
  resp.update(key_form, p1::kKeyLen);
  uint8_t response[64];
  resp.final(response);

  // ---- pass 2: nextChallenge from the written sections, as `powersoftau contribute` makes it; the record against the trail
  timed(hash_ms, [&] { close_record(ctx, fo, response, d_pts.p, piece, phase.command, &rec); });
  if (!p1::verify_record(rec, trail))
    throw SetupError("powersoftau import response: the record does not verify against the old file: the response's key does not "
                     "tie its points to the old file's points and challenge");
  append_record(fo, in.records, rec);
  verbose_split(phase, {{"read (file -> HBM)", read_ms}, {"decompress (waiting for the device)", decompress_ms},
                        {"checks (curve, G2 subgroup)", check_ms}, {"hashes (response, nextChallenge)", hash_ms},
                        {"write (HBM -> file; overlaps the rest)", rb.write_ms[0] + rb.write_ms[1]}});
  phase("sections 2-7 written, file renamed into place");
}

// a command's record parameters from its --name and, for a beacon (type 1), its bytes and exponent: checked once, whole
// (RecordParams::check throws "<command>: ...")
p2::RecordParams record_params(const char* command, const char* name, uint32_t type = 0, const uint8_t* beacon = nullptr,
                               unsigned long beacon_len = 0, uint32_t num_iterations_exp = 0) {
  p2::RecordParams ap{type, name ? name : "", {beacon, beacon + beacon_len}, num_iterations_exp};
  ap.check(command);
  return ap;
}

}  // namespace

extern "C" int zkpoa_scalar_mul_each_device(zkpoa_context* ctx, int group, const void* d_points, const void* d_scalars,
                                            uint64_t n, void* d_out) {
  ZK_API_BEGIN(ctx)
  if (group != 1 && group != 2) throw SetupError("scalar_mul_each: group must be 1 (G1) or 2 (G2)");
  if (n && (!d_points || !d_scalars || !d_out)) throw SetupError("scalar_mul_each: null pointer");
  const uint64_t slab = (uint64_t)ctx->opt_ptau_mul_slab;
  DevBuf flag(64), scratch(scalar_mul_each_scratch(group, n, slab));
  ZK_HIP(hipMemsetAsync(flag.p, 0, 64, ctx->dev.lanes[0].stream));
  scalar_mul_each(ctx, group, d_points, d_scalars, n, d_out, (uint32_t*)flag.p, scratch.p, slab);
  finish(ctx->dev.lanes[0].stream);
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
  finish(ctx->dev.lanes[0].stream);
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
  ptau_contribute(ctx, in_path, out_path, secrets_le, record_params("powersoftau contribute", name));
  ZK_API_END(ctx)
}

extern "C" int zkpoa_ptau_beacon(zkpoa_context* ctx, const char* in_path, const char* out_path, const uint8_t* beacon,
                                 unsigned long beacon_len, uint32_t num_iterations_exp, const char* name) {
  ZK_API_BEGIN(ctx)
  if (!in_path || !out_path || (!beacon && beacon_len)) throw SetupError("powersoftau beacon: null argument");
  ptau_contribute(ctx, in_path, out_path, nullptr, record_params("powersoftau beacon", name, 1, beacon, beacon_len, num_iterations_exp));
  ZK_API_END(ctx)
}

extern "C" int zkpoa_ptau_export_challenge(zkpoa_context* ctx, const char* ptau_path, const char* challenge_path,
                                           uint8_t challenge_hash[64]) {
  ZK_API_BEGIN(ctx)
  if (!ptau_path || !challenge_path) throw SetupError("powersoftau export challenge: null path");
  ptau_export_challenge(ctx, ptau_path, challenge_path, challenge_hash);
  ZK_API_END(ctx)
}

extern "C" int zkpoa_ptau_challenge_contribute(zkpoa_context* ctx, const char* challenge_path, const char* response_path,
                                               const uint8_t* secrets_le, uint8_t response_hash[64]) {
  ZK_API_BEGIN(ctx)
  if (!challenge_path || !response_path) throw SetupError("powersoftau challenge contribute: null path");
  ptau_challenge_contribute(ctx, challenge_path, response_path, secrets_le, response_hash);
  ZK_API_END(ctx)
}

extern "C" int zkpoa_ptau_import_response(zkpoa_context* ctx, const char* old_path, const char* response_path,
                                          const char* new_path, const char* name) {
  ZK_API_BEGIN(ctx)
  if (!old_path || !response_path || !new_path) throw SetupError("powersoftau import response: null path");
  ptau_import_response(ctx, old_path, response_path, new_path, record_params("powersoftau import response", name));
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
