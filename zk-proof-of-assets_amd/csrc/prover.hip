// Groth16 prove on the device: zkey/wtns container parsing, device-resident proving key,
// buildABC -> coset NTT chain -> joinABC -> five MSMs -> randomised assembly -> JSON.
//
// This is what runs behind the reference's exec boundary scripts/g16_prove.sh:248-252
// (`prover <zkey> <wtns> <proof.json> <public.json>`); algorithm per snarkjs 0.7.2
// groth16_prove.js as restated in SURVEY.md 3.2 / 8c (the reference vendors no prover source).
#include "abc.hip.h"
#include "binfile.hpp"
#include "msm.hip.h"
#include "ntt.hip.h"
#include "zkpoa_internal.hpp"

#include <fcntl.h>
#include <stdlib.h>
#include <string.h>
#include <sys/file.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <exception>
#include <functional>
#include <future>
#include <memory>
#include <map>
#include <mutex>
#include <system_error>
#include <thread>

using namespace zkpoa;

namespace {

struct ProverError : std::runtime_error {
  int code;
  ProverError(int c, const std::string& s) : std::runtime_error(s), code(c) {}
};

// ---- binfile container (the scan itself: binfile.hpp) with the prover's error texts
struct Section {
  const uint8_t* p = nullptr;
  uint64_t len = 0;
};
typedef std::map<uint32_t, Section> Sections;

void check_scan(BinScan r, const char* magic) {
  static const char* const why[] = {"", "invalid file format (bad magic)", "version not supported",
                                    "truncated section table", "truncated section"};
  if (r != kBinOk) throw ProverError(PROVER_ERROR, std::string(magic) + " file: " + why[r]);
}

Sections parse_binfile(const uint8_t* buf, uint64_t size, const char* magic, uint32_t max_version) {
  std::map<uint32_t, Sec> secs;
  check_scan(bin_scan(buf, size, magic, max_version, secs), magic);
  Sections out;
  for (const auto& kv : secs) out[kv.first] = Section{buf + kv.second.off, kv.second.len};
  return out;
}

const Section& need(const Sections& s, uint32_t id, const char* what) {
  auto it = s.find(id);
  if (it == s.end()) throw ProverError(PROVER_ERROR, std::string("missing section ") + what);
  return it->second;
}

const uint8_t kR[32] = {0x01, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9, 0x79, 0x48, 0xe8, 0x33, 0x28,
                        0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};

DevMem dev_upload(zkpoa_context* ctx, const void* src, size_t bytes) {
  DevMem d;
  auto t0 = std::chrono::steady_clock::now();
  d.alloc(bytes);
  auto t1 = std::chrono::steady_clock::now();
  if (bytes) ctx->uploader.upload(d.get(), src, bytes, ctx->dev.device, ctx->dev.lanes[0].stream);
  if (bytes > (16u << 20))
    vlog("zkpoa:   upload %.0f MB: hipMalloc %.1f ms, copy %.1f ms\n", bytes / 1e6,
         std::chrono::duration<double, std::milli>(t1 - t0).count(), ms_since(t1));
  return d;
}

}  // namespace

#include "zkey_handle.hip.h"   // zkpoa_zkey: what a resident key holds and owns, its shard arithmetic, its header points

namespace {

// count x 32-byte elements at d must all be below the modulus (Fq: point coordinates, Fr: witness values)
template <class PRM>
void range_check(hipStream_t st, const void* d, uint64_t count, uint32_t* d_flag) {
  if (count)
    hipLaunchKernelGGL((range_check_kernel<PRM>), dim3((uint32_t)((count + 255) / 256)), dim3(256), 0, st, d, count, d_flag);
}

// Every coordinate of the part of a point section the handle holds must be a canonical Fq element (< q): one pass over
// it on `st`, which ORs into the caller's zeroed flag word. The section must be resident.
enum { kSecA, kSecB1, kSecB2, kSecC, kSecH };
void section_range_check(const zkpoa_zkey* zk, int sec, hipStream_t st, uint32_t* d_flag) {
  const bool cyclic = zk->split_world > 1;
  switch (sec) {
    case kSecA: return range_check<FqParams>(st, zk->dA.get(), zk->wcnt * 2, d_flag);
    case kSecB1: return range_check<FqParams>(st, zk->dB1.get(), zk->wcnt * 2, d_flag);
    case kSecB2: return range_check<FqParams>(st, zk->dB2.get(), zk->wcnt * 4, d_flag);
    case kSecC: return range_check<FqParams>(st, zk->dC.get(), zk->ccnt * 2, d_flag);
    default:
      return range_check<FqParams>(st, cyclic ? zk->dHs.get() : zk->dH.get(),
                                   (cyclic ? zk->h_scalar_count() : zk->hcnt) * 2, d_flag);
  }
}

// CSR of the coefficient list by output row (2*c + m), into the handle; d_recs = device copy of the 44-byte records.
// Also allocates the A/B/C work area and the witness buffer. With split_log > 0 (split chain loaded from a
// file) only the records of this rank's constraints are kept, rows renumbered c >> split_log.
void build_csr(zkpoa_context* ctx, zkpoa_zkey* zk, const void* d_recs, bool local_rows = false, hipStream_t st_in = nullptr) {
  hipStream_t st = st_in ? st_in : ctx->dev.lanes[0].stream;
  const uint32_t lp = local_rows ? zk->split_log : 0u, part = local_rows ? zk->split_rank : 0u;
  const uint64_t n = zk->domain, m = zk->nVars;
  // work area: the chain transforms A_T, B_T, C_T in place (a split shard: its n / G rows of each)
  if (!zk->d_abc) zk->d_abc.alloc((size_t)3 * (n >> lp) * 32);
  if (!zk->wbuf[0]) {
    zk->wbuf[0].alloc((size_t)m * 32);
    zk->d_witness = zk->wbuf[0].get();
  }
  if (!zk->d_flag) zk->d_flag.alloc(1024);   // + scratch of msm_density at +256
  AbcCsr csr;
  abc_build_csr(st, d_recs, zk->nCoefs, zk->domain, zk->nVars, lp, part, csr);
  if (csr.err & 2u) throw ProverError(PROVER_ERROR, "zkey coefficient value is not a field element (>= r)");
  if (csr.err) throw ProverError(PROVER_ERROR, "zkey coefficient record out of range (matrix/constraint/signal)");
  zk->nCoefsLocal = csr.total;
  zk->csr_local = local_rows;
  zk->d_row_ptr = std::move(csr.row_ptr);
  zk->d_sig = std::move(csr.sig);
  zk->d_vals = std::move(csr.vals);
  zk->d_long = std::move(csr.long_list);
  zk->n_long = csr.n_long;
}

// this shard's slice of a compacted query: two 4-byte reads of the position array
void query_set_slice(const zkpoa_zkey* zk, CompactQuery& q) {
  uint32_t a = 0, b = 0;
  const uint32_t* pos = q.pos.as<uint32_t>();
  ZK_HIP(hipMemcpy(&a, pos + (zk->wlo - zk->wbase), 4, hipMemcpyDeviceToHost));
  ZK_HIP(hipMemcpy(&b, pos + (zk->wlo - zk->wbase + zk->wcnt), 4, hipMemcpyDeviceToHost));
  q.lo = a;
  q.cnt = b - a;
}
void queries_set_slice(zkpoa_zkey* zk) {
  query_set_slice(zk, zk->qA);
  query_set_slice(zk, zk->qB);
}

// Compact the resident range [wbase, wbase + wres) of a query (d1: G1 section, d2: its G2 twin or null) once per key.
void query_compact(zkpoa_context* ctx, zkpoa_zkey* zk, CompactQuery& q, const void* d1, const void* d2,
                   uint64_t wres, hipStream_t st_in = nullptr) {
  hipStream_t st = st_in ? st_in : ctx->dev.lanes[0].stream;
  const uint32_t n = (uint32_t)wres;
  DevBuf keep(((size_t)n + 1) * 4), bs(((size_t)n / kScanTile + 2) * 4), misc(64);
  q.pos.alloc(((size_t)n + 1) * 4);
  uint32_t* pos = q.pos.as<uint32_t>();
  ZK_HIP(hipMemsetAsync(misc.p, 0, 64, st));
  uint32_t total = 0;
  if (n) {
    hipLaunchKernelGGL(query_keep_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (const uint4*)d1, (const uint4*)d2, n,
                       (uint32_t*)keep.p);
    scan_u32(st, (const uint32_t*)keep.p, n, 0, 0, pos, (uint32_t*)bs.p, (uint32_t*)misc.p, nullptr);
    ZK_HIP(hipMemcpyAsync(&total, pos + n, 4, hipMemcpyDeviceToHost, st));
  } else {
    ZK_HIP(hipMemsetAsync(pos, 0, 4, st));
  }
  finish(st);
  q.res = total;
  const size_t cnt = total ? total : 1;
  q.g1.alloc(cnt * 64);
  if (d2) q.g2.alloc(cnt * 128);
  q.scalars.alloc(cnt * 32);
  q.wire.alloc(cnt * 4);
  if (n) {
    hipLaunchKernelGGL(query_compact_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (const uint4*)d1, (const uint4*)d2,
                       (const uint32_t*)pos, n, (uint32_t)zk->wbase, zk->bc_log, zk->bc_rank, zk->bc_world,
                       q.g1.as<uint4>(), q.g2.as<uint4>(), q.wire.as<uint32_t>());
    finish(st);
  }
  query_set_slice(zk, q);
}

// Both witness queries; the originals go afterwards (nothing reads them again: the MSMs use the compacted copies) --
// freed when they are the handle's own, merely let go of when the caller lent them.
void queries_compact(zkpoa_context* ctx, zkpoa_zkey* zk, uint64_t wres) {
  query_compact(ctx, zk, zk->qA, zk->dA.get(), nullptr, wres);
  query_compact(ctx, zk, zk->qB, zk->dB1.get(), zk->dB2.get(), wres);
  zk->dA.reset();
  zk->dB1.reset();
  zk->dB2.reset();
}

// the five point sections and the coefficient section of a parsed zkey
struct ZkeySections {
  Section s4, s5, s6, s7, s8, s9;
};

// container + header validation; fills the handle's scalar fields, header points and verification key (host state only)
KeyPtr zkey_parse(const uint8_t* buf, uint64_t size, ZkeySections& out) {
  Sections secs = parse_binfile(buf, size, "zkey", 2);
  const Section& s1 = need(secs, 1, "1 (protocol)");
  if (s1.len < 4 || rd32(s1.p) != 1) throw ProverError(PROVER_ERROR, "zkey file is not groth16");
  const Section& s2 = need(secs, 2, "2 (groth16 header)");
  if (s2.len < kHdrLen) throw ProverError(PROVER_ERROR, "zkey header too short");
  const ZkeyHeader h = read_zkey_header(s2.p);
  if (h.n8q != 32 || !h.q_ok) throw ProverError(PROVER_ERROR, "zkey curve not supported (q is not BN254)");
  if (h.n8r != 32 || !h.r_ok) throw ProverError(PROVER_ERROR, "zkey curve not supported (r is not BN254)");
  KeyPtr zk(new zkpoa_zkey());
  zk->nVars = h.nVars;
  zk->nPublic = h.nPublic;
  zk->domain = h.domain;
  if (zk->domain == 0 || (zk->domain & (zk->domain - 1))) throw ProverError(PROVER_ERROR, "zkey domainSize is not a power of two");
  zk->power = 0;
  while ((1u << zk->power) < zk->domain) zk->power++;
  if (zk->power > 28) throw ProverError(PROVER_ERROR, "zkey domainSize exceeds 2^28");
  if (zk->nPublic + 1 > zk->nVars) throw ProverError(PROVER_ERROR, "zkey nPublic >= nVars");
  zk->hdr = header_points(h.alpha1, h.beta1, h.beta2, h.delta1, h.delta2);
  // section 3 (IC) is optional for proving; with it the handle can verify its own proofs
  {
    auto it3 = secs.find(3);
    if (it3 != secs.end() && it3->second.len == ((uint64_t)zk->nPublic + 1) * 64) {
      zk->vkey_points.resize(448 + it3->second.len);
      uint8_t* v = zk->vkey_points.data();
      memcpy(v, h.alpha1, 64);
      memcpy(v + 64, h.beta2, 128);
      memcpy(v + 192, h.gamma2, 128);   // verifier only: kept for the self-check
      memcpy(v + 320, h.delta2, 128);
      memcpy(v + 448, it3->second.p, it3->second.len);
    }
  }
  out.s4 = need(secs, 4, "4 (coefficients)");
  if (out.s4.len < 4) throw ProverError(PROVER_ERROR, "zkey coefficient section too short");
  zk->nCoefs = rd32(out.s4.p);
  if (out.s4.len != 4 + zk->nCoefs * 44) throw ProverError(PROVER_ERROR, "zkey coefficient section has the wrong size");
  out.s5 = need(secs, 5, "5 (A points)");
  out.s6 = need(secs, 6, "6 (B1 points)");
  out.s7 = need(secs, 7, "7 (B2 points)");
  out.s8 = need(secs, 8, "8 (C points)");
  out.s9 = need(secs, 9, "9 (H points)");
  const uint64_t m = zk->nVars, n = zk->domain;
  if (out.s5.len != m * 64 || out.s6.len != m * 64 || out.s7.len != m * 128 ||
      out.s8.len != (m - zk->nPublic - 1) * 64 || out.s9.len != n * 64)
    throw ProverError(PROVER_ERROR, "zkey point section has the wrong size");
  return zk;
}

struct LoadPhases {   // ZKPOA_VERBOSE: where a key load spends its time
  bool verbose = opt_verbose();
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void operator()(const char* what) {
    if (verbose) fprintf(stderr, "zkpoa: zkey load: %-34s %7.1f ms\n", what, ms_since(t));
    t = std::chrono::steady_clock::now();
  }
};

// The rest of a key load, once the point sections are resident: compacted queries, CSR and per-proof buffers, NTT
// tables; synchronised on return. recs: the 44-byte coefficient records, in device memory or (recs_on_host) still in
// the file: those go up only after the queries' originals are freed, and their device copy goes once the CSR exists.
void finish_load(zkpoa_context* ctx, zkpoa_zkey* zk, const void* recs, bool recs_on_host, bool split, LoadPhases phase) {
  hipStream_t st = ctx->dev.lanes[0].stream;
  if (zk->bc_log) zk->d_cscal.alloc(zk->ccnt * 32);
  queries_compact(ctx, zk, zk->wcnt);
  phase("A / B queries without infinity");
  DevMem uploaded;
  if (recs_on_host) {
    uploaded = dev_upload(ctx, recs, zk->nCoefs * 44);
    recs = uploaded.get();
    phase("coefficient section -> HBM");
  }
  build_csr(ctx, zk, recs, split);
  uploaded.reset();
  phase("CSR of the coefficients");
  ntt_prepare(ctx, st, zk->power);
  if (split) ntt_prepare(ctx, st, zk->power - zk->split_log);
  ZK_HIP(hipStreamSynchronize(st));
  phase("NTT tables");
}

KeyPtr zkey_load_impl(zkpoa_context* ctx, const uint8_t* buf, uint64_t size, uint64_t rank = 0,
                      uint64_t world = 1, bool split = false, uint32_t bc_log = 0) {
  ZkeySections zs;
  KeyPtr zk = zkey_parse(buf, size, zs);
  const Section &s4 = zs.s4, &s5 = zs.s5, &s6 = zs.s6, &s7 = zs.s7, &s8 = zs.s8, &s9 = zs.s9;
  const uint64_t m = zk->nVars;
  shard_init(zk.get(), rank, world, split, bc_log);
  zk->device = ctx->dev.device;   // from here on the handle holds device memory
  LoadPhases phase;
  // each rank uploads only its byte range(s) of every point section: one contiguous range, or with block-cyclic
  // shards its blocks of 2^bc_log items one after the other (each still a contiguous byte range of the file)
  auto upload_items = [&](const uint8_t* sec, uint64_t n_items, uint64_t lo, uint64_t cnt, size_t unit) -> DevMem {
    if (!zk->bc_log) return dev_upload(ctx, sec + lo * unit, cnt * unit);
    DevMem d;
    d.alloc(cnt * unit);
    const uint64_t B = 1ull << zk->bc_log;
    for (uint64_t lb = 0;; lb++) {
      const uint64_t start = (lb * world + rank) << zk->bc_log;
      if (start >= n_items) break;
      const uint64_t len = n_items - start < B ? n_items - start : B;
      ctx->uploader.upload(d.as<char>() + (lb << zk->bc_log) * unit, sec + start * unit, len * unit, ctx->dev.device,
                           ctx->dev.lanes[0].stream);
    }
    return d;
  };
  zk->dA = upload_items(s5.p, m, zk->wlo, zk->wcnt, 64);
  zk->dB1 = upload_items(s6.p, m, zk->wlo, zk->wcnt, 64);
  zk->dB2 = upload_items(s7.p, m, zk->wlo, zk->wcnt, 128);
  zk->dC = upload_items(s8.p, m - zk->nPublic - 1, zk->clo, zk->ccnt, 64);
  if (split) {
    // cyclic H shard: H[t * world + rank], gathered on the host (the section is walked once per rank)
    const uint64_t cnt = zk->h_scalar_count();
    std::vector<uint8_t> stage(cnt * 64);
    const unsigned nthreads = 6;
    run_threads(nthreads, [&](unsigned k) {
      for (uint64_t t = cnt * k / nthreads; t < cnt * (k + 1) / nthreads; t++)
        memcpy(stage.data() + t * 64, s9.p + (t * world + rank) * 64, 64);
    });
    zk->dHs = dev_upload(ctx, stage.data(), cnt * 64);
  } else {
    zk->dH = dev_upload(ctx, s9.p + zk->hlo * 64, zk->hcnt * 64);
  }
  phase("point sections 5-9 -> HBM");
  {   // every coordinate must be a canonical Fq element (< q)
    hipStream_t st0 = ctx->dev.lanes[0].stream;
    DevBuf flag(64);
    ZK_HIP(hipMemsetAsync(flag.p, 0, 64, st0));
    for (int sec : {kSecA, kSecB1, kSecB2, kSecC, kSecH}) section_range_check(zk.get(), sec, st0, (uint32_t*)flag.p);
    uint32_t bad = 0;
    ZK_HIP(hipMemcpyAsync(&bad, flag.p, 4, hipMemcpyDeviceToHost, st0));
    ZK_HIP(hipStreamSynchronize(st0));
    if (bad) throw ProverError(PROVER_ERROR, "zkey point coordinate is not a field element (>= q)");
    phase("coordinate range check");
  }
  finish_load(ctx, zk.get(), s4.p + 4, /*recs_on_host=*/true, split, phase);
  return zk;
}

// H-scalar chain on lane.stream: A_T,B_T,C_T -> odd coset -> P (standard form) left in abc[0 .. n)
void h_chain(zkpoa_context* ctx, hipStream_t st, const uint32_t* row_ptr, const uint32_t* sig, const void* vals,
             const uint32_t* long_list, uint32_t n_long, const void* d_witness, uint32_t domain, uint32_t power,
             void* d_abc) {
  char* A = reinterpret_cast<char*>(d_abc);
  char* B = A + (size_t)domain * 32;
  char* C = B + (size_t)domain * 32;
  uint32_t grid = (domain + 255) / 256;
  hipLaunchKernelGGL(abc_rows_kernel, dim3(grid), dim3(256), 0, st, row_ptr, sig, vals, d_witness, domain, 0u, 1u,
                     (void*)A, (void*)B, (void*)C);
  if (n_long)
    hipLaunchKernelGGL(abc_long_rows_kernel, dim3((n_long + 3) / 4), dim3(256), 0, st, row_ptr, sig, vals, d_witness,
                       long_list, n_long, 0u, 0u, (void*)A, (void*)B, (void*)C);
  ntt_to_odd_coset(ctx, st, A, power, 3, (size_t)domain * 32);   // A, B and C together: 4-6 launches instead of 12-18
  hipLaunchKernelGGL(abc_join_kernel, dim3(grid), dim3(256), 0, st, (const void*)A, (const void*)B, (const void*)C,
                     domain, (void*)A);
}

// ---- split chain: three local stages around two all-to-all exchanges the caller runs ----
// Exchange buffers (caller's device memory, e.g. torch tensors handed to RCCL): [G ranks][3 polynomials A, B, C]
// [Q = M / G elements] x 32 B, M = domain / G. Chunk h (3 Q elements, contiguous) is what rank h receives from this
// rank, so each exchange is ONE all_to_all_single with equal splits over the whole buffer. The stages compute in the
// handle's own work area ([3][M]) and pack / unpack at the boundary. All three ENQUEUE on lane 0's stream and return
// (zkpoa_context_stream): a caller that runs its collectives on that stream needs no host synchronisation between
// stage and exchange; anyone else calls zkpoa_context_synchronize first.
void split_stage1(zkpoa_context* ctx, const zkpoa_zkey* zk, void* d_x) {
  hipStream_t st = ctx->dev.lanes[0].stream;
  const uint32_t M = zk->domain >> zk->split_log, kM = zk->power - zk->split_log, Q = M >> zk->split_log;
  char* A = zk->d_abc.as<char>();
  char* B = A + (size_t)M * 32;
  char* C = B + (size_t)M * 32;
  zk->h_ready = false;
  // buildABC for the constraint rows c = rank (mod G): a rank-local CSR is already renumbered
  hipLaunchKernelGGL(abc_rows_kernel, dim3((M + 255) / 256), dim3(256), 0, st, zk->d_row_ptr.as<const uint32_t>(),
                     zk->d_sig.as<const uint32_t>(), (const void*)zk->d_vals.get(), (const void*)zk->d_witness, M,
                     zk->csr_local ? 0u : zk->split_rank, zk->csr_local ? 1u : zk->split_world, (void*)A, (void*)B,
                     (void*)C);
  if (zk->n_long)   // a rank-local CSR lists its own rows; a full CSR lists all, the kernel keeps c = rank (mod G)
    hipLaunchKernelGGL(abc_long_rows_kernel, dim3((zk->n_long + 3) / 4), dim3(256), 0, st,
                       zk->d_row_ptr.as<const uint32_t>(), zk->d_sig.as<const uint32_t>(), (const void*)zk->d_vals.get(),
                       (const void*)zk->d_witness, zk->d_long.as<const uint32_t>(), zk->n_long,
                       zk->csr_local ? 0u : zk->split_log, zk->csr_local ? 0u : zk->split_rank, (void*)A, (void*)B,
                       (void*)C);
  ntt_dif(ctx, st, A, kM, true, 3, (size_t)M * 32);
  hipLaunchKernelGGL((split_pack_kernel<true>), dim3((uint32_t)(((uint64_t)6 * M + 255) / 256)), dim3(256), 0, st,
                     zk->d_abc.as<const uint4>(), (uint4*)d_x, M, Q);
  ZK_HIP(hipGetLastError());
}

void split_stage2(zkpoa_context* ctx, const zkpoa_zkey* zk, const void* d_in, void* d_out) {
  hipStream_t st = ctx->dev.lanes[0].stream;
  const size_t M = zk->domain >> zk->split_log, Q = M >> zk->split_log;
  for (int x = 0; x < 3; x++)   // polynomial x of every rank's block: offset x * Q, blocks 3 Q apart
    ntt_split_mid(ctx, st, reinterpret_cast<const char*>(d_in) + x * Q * 32, reinterpret_cast<char*>(d_out) + x * Q * 32,
                  zk->power, zk->split_world, zk->split_rank, (uint32_t)(3 * Q));
  ZK_HIP(hipGetLastError());
}

void split_stage3(zkpoa_context* ctx, const zkpoa_zkey* zk, const void* d_x) {
  hipStream_t st = ctx->dev.lanes[0].stream;
  const uint32_t M = zk->domain >> zk->split_log, kM = zk->power - zk->split_log, Q = M >> zk->split_log;
  char* A = zk->d_abc.as<char>();
  char* B = A + (size_t)M * 32;
  char* C = B + (size_t)M * 32;
  hipLaunchKernelGGL((split_pack_kernel<false>), dim3((uint32_t)(((uint64_t)6 * M + 255) / 256)), dim3(256), 0, st,
                     (const uint4*)d_x, zk->d_abc.as<uint4>(), M, Q);
  ntt_dit(ctx, st, A, kM, false, 3, (size_t)M * 32);
  hipLaunchKernelGGL(abc_join_kernel, dim3((M + 255) / 256), dim3(256), 0, st, (const void*)A, (const void*)B,
                     (const void*)C, M, zk->d_abc.get());
  ZK_HIP(hipGetLastError());
  zk->h_ready = true;   // in stream order: the H MSM of zkpoa_prove_partials_device runs on the same stream
}

HFr hfr_from_le(const uint8_t* le) { return HFr::from_bytes(le); }

// uniform on [0, r): 254 random bits, rejected while >= r (about one draw in four is), as Groth16's zero-knowledge
// argument assumes and as snarkjs' Fr.random() samples
void random_scalar(uint8_t out[32]) {
  for (;;) {
    if (const char* err = read_urandom(out, 32)) throw ProverError(PROVER_ERROR, err);
    out[31] &= 0x3f;   // 254 bits
    bool below = false;
    for (int i = 31; i >= 0; i--) {
      if (out[i] < kR[i]) { below = true; break; }
      if (out[i] > kR[i]) break;
    }
    if (below) break;
  }
}

bool parse_decimal_mod_r(const char* s, uint8_t out[32]) {
  if (!s || !*s) return false;
  HFr acc = HFr::zero(), ten = HFr::from_u64(10);
  for (const char* c = s; *c; c++) {
    if (*c < '0' || *c > '9') return false;
    acc = acc * ten + HFr::from_u64((uint64_t)(*c - '0'));
  }
  acc.from_mont().to_bytes(out);
  return true;
}

// Where a witness comes from: a complete .wtns image in memory (the rapidsnark-shaped entry points), or an open file
// (the `prover` executable, zkpoa_groth16_prover_files): then only the few header bytes are ever read through the CPU
// and the values go from the page cache straight into the uploader's pinned staging buffers (pread) -- mapping a 1.7 GB
// layer-three witness first costs ~25 ms of page-table work before the first byte moves, and as much again to unmap.
struct WtnsSrc {
  const uint8_t* buf = nullptr;
  uint64_t size = 0;
  int fd = -1;
};

struct WtnsView {
  const uint8_t* values = nullptr;   // memory form; null in file form
  uint32_t n = 0;
  int fd = -1;                       // file form: the values start at byte `off` of fd
  uint64_t off = 0;
  // values [first, first + count) -> out
  void read(uint64_t first, uint64_t count, uint8_t* out) const {
    if (fd < 0) {
      memcpy(out, values + first * 32, (size_t)count * 32);
      return;
    }
    size_t got = 0, want = (size_t)count * 32;
    while (got < want) {
      ssize_t r = pread(fd, out + got, want - got, (off_t)(off + first * 32 + got));
      if (r <= 0) throw ProverError(PROVER_ERROR, "wtns file: short read");
      got += (size_t)r;
    }
  }
  // the public signals w[1 .. n_public] (standard form), valid while `store` lives
  const uint8_t* publics(uint32_t n_public, std::vector<uint8_t>& store) const {
    if (fd < 0) return values + 32;
    store.resize((size_t)n_public * 32 + 1);
    if (n_public) read(1, n_public, store.data());
    return store.data();
  }
  // values [first, first + count) -> device memory at dst, on `st` (synchronised on return)
  void upload(zkpoa_context* ctx, void* dst, uint64_t first, uint64_t count, hipStream_t st) const {
    ctx->uploader.upload(dst, fd < 0 ? values + first * 32 : nullptr, (size_t)count * 32, ctx->dev.device, st, fd,
                         off + first * 32);
  }
};

WtnsView parse_wtns(const uint8_t* buf, uint64_t size) {
  Sections secs = parse_binfile(buf, size, "wtns", 2);
  const Section& s1 = need(secs, 1, "1 (wtns header)");
  if (s1.len < 40 || rd32(s1.p) != 32) throw ProverError(PROVER_ERROR, "wtns header: unsupported field size");
  if (memcmp(s1.p + 4, kR, 32) != 0)
    throw ProverError(PROVER_ERROR, "Curve of the witness does not match the curve of the proving key");
  WtnsView w;
  w.n = rd32(s1.p + 36);
  const Section& s2 = need(secs, 2, "2 (wtns values)");
  if (s2.len != (uint64_t)w.n * 32) throw ProverError(PROVER_ERROR, "wtns value section has the wrong size");
  w.values = s2.p;
  return w;
}

// the same on an open file: 12 bytes per section header are read, payloads are skipped
WtnsView parse_wtns_fd(int fd, uint64_t size) {
  auto rd = [&](uint64_t pos, void* out, size_t len) {
    size_t got = 0;
    while (got < len) {
      ssize_t r = pread(fd, static_cast<char*>(out) + got, len - got, (off_t)(pos + got));
      if (r <= 0) throw ProverError(PROVER_ERROR, "wtns file: short read");
      got += (size_t)r;
    }
  };
  std::map<uint32_t, Sec> secs;
  check_scan(bin_scan(rd, size, "wtns", 2, secs), "wtns");
  const bool have1 = secs.count(1), have2 = secs.count(2);
  const uint64_t off1 = secs[1].off, len1 = secs[1].len, off2 = secs[2].off, len2 = secs[2].len;
  if (!have1) throw ProverError(PROVER_ERROR, "missing section 1 (wtns header)");
  uint8_t h1[40];
  if (len1 < 40) throw ProverError(PROVER_ERROR, "wtns header: unsupported field size");
  rd(off1, h1, 40);
  if (rd32(h1) != 32) throw ProverError(PROVER_ERROR, "wtns header: unsupported field size");
  if (memcmp(h1 + 4, kR, 32) != 0)
    throw ProverError(PROVER_ERROR, "Curve of the witness does not match the curve of the proving key");
  WtnsView w;
  w.n = rd32(h1 + 36);
  if (!have2) throw ProverError(PROVER_ERROR, "missing section 2 (wtns values)");
  if (len2 != (uint64_t)w.n * 32) throw ProverError(PROVER_ERROR, "wtns value section has the wrong size");
  w.fd = fd;
  w.off = off2;
  return w;
}

WtnsView parse_wtns(const WtnsSrc& src) {
  return src.fd >= 0 ? parse_wtns_fd(src.fd, src.size) : parse_wtns(src.buf, src.size);
}

void check_witness_len(const WtnsView& w, const zkpoa_zkey* zk) {
  if (w.n != zk->nVars)
    throw ProverError(PROVER_INVALID_WITNESS_LENGTH, "Invalid witness length. Circuit: " + std::to_string(zk->nVars) +
                                                         ", witness: " + std::to_string(w.n));
}

// ---- what each of the five MSMs of a proof covers, for the handle as it is right now (stage = lane id) -------------
// The planner (lane_needs), the table builder (zkey_precompute) and the stages (prove_partials) all read this one view.
enum { kStageH = 0, kStageA = 1, kStageB1 = 2, kStageB2 = 3, kStageC = 4 };
struct StageView {
  uint64_t n = 0;                    // points
  const char* bases = nullptr;       // the first of them; null while a staged prove has not allocated the array
  uint64_t scalar_off = 0;           // H, C: index of the first scalar in d_abc resp. in the witness from wire nPublic + 1
  const MsmTable* table = nullptr;   // the fixed-base table whose array these n points cover exactly, else null (B1 and
  int table_c = 0;                   // B2: only as a pair, they share one sort); table_c: its window width
  // What a table for this stage is built from: the whole resident array, array_n points. The compacted queries record
  // their length; of sections 8 and 9 the handle knows its current range only, which is the whole array when it starts
  // at the array's first point. array_n == 0 means: no table can be built now (that, an absent or an empty array).
  const void* array = nullptr;
  uint64_t array_n = 0;
};
StageView stage_view(const zkpoa_zkey* zk, int stage) {
  StageView v;
  const MsmTable* t = nullptr;
  uint64_t first = 0;   // of these points, in bytes from the start of the array
  if (stage == kStageH && zk->split_world > 1) {   // the cyclic shard, all of it
    v.array = zk->dHs.get();
    v.n = v.array_n = zk->h_scalar_count();
    t = zk->tH_cyclic ? zk->tH.get() : nullptr;
  } else if (stage == kStageH) {
    v.array = zk->dH.get();
    v.n = zk->hcnt;
    first = (zk->hlo - zk->hbase) * 64;
    v.array_n = first ? 0 : v.n;
    v.scalar_off = zk->hlo;
    t = zk->tH_cyclic ? nullptr : zk->tH.get();
  } else if (stage == kStageC) {
    v.array = zk->dC.get();
    v.n = zk->ccnt;
    first = (zk->clo - zk->cbase) * 64;
    v.array_n = first ? 0 : v.n;
    v.scalar_off = zk->clo;
    t = zk->tC.get();
  } else {
    const CompactQuery& q = stage == kStageA ? zk->qA : zk->qB;
    v.array = stage == kStageB2 ? q.g2.get() : q.g1.get();
    v.n = q.cnt;
    v.array_n = q.res;
    first = q.lo * (stage == kStageB2 ? 128 : 64);
    t = stage == kStageA ? zk->tA.get() : !(zk->tB1 && zk->tB2) ? nullptr : stage == kStageB1 ? zk->tB1.get() : zk->tB2.get();
  }
  if (v.array) v.bases = reinterpret_cast<const char*>(v.array) + first;
  else v.array_n = 0;
  if (t && first == 0 && v.n == v.array_n) {
    uint64_t info[4];
    msm_table_info(t, info);
    if (info[0] == v.n) {
      v.table = t;
      v.table_c = (int)info[1];
    }
  }
  return v;
}

// The request (msm_plan.hpp) of a stage's MSM when it takes at most `limit` points at once. The budget (lane_needs) and
// the shared sort of the B query build theirs here; a stage whose MSM may run in chunks hands msm_run the same pieces --
// the view's table and `density` -- and msm_run makes each chunk's request from them with the same msm_request. A table
// is only of use to a whole MSM, and only where the caller allows one. Who passes which density (DESIGN.md "MSM plans"):
//   H (lane 0)                          none: uniform scalars
//   A (1), C (4)                        this proof's witness density (with_density)
//   B shared sort, B1's own MSM (2)     this proof's witness density
//   B2 over the shared sort (3)         nothing to plan: the sort's plan
//   B2's own MSM (3)                    none -- KNOWN MISMATCH: lane_needs sizes that lane with the density
//   lane_needs                          H none; A, B, C the handle's recorded density, if it has one
//   zkey_precompute (msm_table_c)       H table none; A / B / C widths the handle's recorded density, if it has one
static MsmRequest stage_request(const zkpoa_context* ctx, const StageView& v, uint64_t limit, const double* density,
                                bool for_g2, bool with_table = true) {
  return msm_request(ctx, std::min(v.n, limit), with_table && v.n <= limit ? v.table_c : 0, for_g2, density);
}

// Fixed-base tables for a resident key, most valuable first, while they fit the budget (bytes; 0 = half of the HBM
// that is free right now -- which leaves room for the per-lane sort / bucket workspaces). H and C first: the H MSM
// closes the critical path and section 8 is the largest G1 array; then the A query; the B query needs both its
// G1 and G2 table (they share one bucket sort). Returns the bytes allocated.
// max_new < 0: all of them at once, replacing what exists (zkpoa_zkey_precompute, the eager policy). max_new >= 0: keep
// what exists and build at most that many more -- the resident prover builds a key's tables one per idle moment, so that
// a request never waits for more than one of them (a whole set is 0.25 s at the layer-one shape, 3-7 s at layers two and
// three: more than twenty proofs' worth, which a workflow of two batches never earns back on the request path).
static size_t lane_workspace_total(const zkpoa_context* ctx, const zkpoa_zkey* zk, const uint64_t lim[5]);   // below
uint64_t zkey_precompute(zkpoa_context* ctx, zkpoa_zkey* zk, uint64_t budget, int max_new = -1) {
  const bool split = zk->split_world > 1;   // H table over the cyclic shard; A / B / C as for any shard
  ctx->dev.wait_lanes();
  ZK_HIP(hipDeviceSynchronize());
  const bool step = max_new >= 0;
  int built = 0;
  bool deferred = false;
  if (!step) zk->release_tables();
  if (step && zk->table_budget) budget = zk->table_budget;
  bool release_lanes = false;
  size_t held = 0;
  if (budget == 0) {
    // the lanes' grow-only workspaces are given back first (they regrow to what the fixed-base plans need) -- counted
    // as free here, released below once it is known that a table will be built at all
    for (auto& l : ctx->dev.lanes) held += l.ws.cap;
    release_lanes = true;
    size_t free_b = 0, total_b = 0;
    ZK_HIP(hipMemGetInfo(&free_b, &total_b));
    free_b += held;
    // ... but never the room the five lanes need for whole MSMs over this key (a chunked MSM cannot use its table, so
    // a table that pushes its own MSM into pieces is HBM spent to be slower): at the reference's shapes the half is the
    // smaller figure (2^26: ~100 GB of workspaces against 230 GB free); on a 2^27 key the workspaces come first
    uint64_t lim[5];
    for (int l = 0; l < 5; l++) lim[l] = ctx->msm_points_limit(l);
    const double room = (double)free_b - 1.1 * (double)lane_workspace_total(ctx, zk, lim);
    budget = (uint64_t)std::max(0.0, std::min(0.5 * (double)free_b, room)) + zk->table_bytes;
  }
  if (step) zk->table_budget = budget;
  const int force_c = ctx->opt_msm_c;
  auto fits = [&](uint64_t bytes) { return zk->table_bytes + bytes <= budget; };
  // One list of the tables this handle could have, most valuable first (B1 and B2 are one step). n = 0: nothing to
  // build from -- an empty or absent array, or a range of section 8 / 9 that is not the whole resident array.
  struct Candidate {
    MsmTablePtr* slot;
    bool g2;
    const void* bases;
    uint64_t n;
    int c;
    size_t bytes() const { return g2 ? msm_table_bytes_g2(n, c) : msm_table_bytes_g1(n, c); }
  };
  // a table that does not fit after all (allocation failure) ends the list; the ones built so far stay
  auto build = [&](const Candidate& t) -> bool {
    if (*t.slot) return true;                   // (step mode: built by an earlier step)
    if (step && built >= max_new) {             // this step's share is done: the rest waits for the next step
      deferred = true;
      return false;
    }
    built++;
    try {
      *t.slot = t.g2 ? msm_table_build_g2(ctx, t.bases, t.n, t.c) : msm_table_build_g1(ctx, t.bases, t.n, t.c);
      zk->table_bytes += t.bytes();
      return true;
    } catch (const HipError&) {
      (void)hipGetLastError();
      return false;
    }
  };
  // H scalars are uniform (its table: msm_table_build's own width); the A / B / C tables are sized for witness scalars
  // when a proof has measured some
  auto witness_c = [&](uint64_t n, bool g2) {
    if (const long c = opt_long(O_WITNESS_TABLE_C)) return (int)c;   // experiments only
    return (int)msm_table_c(n, force_c, g2, zk->have_density ? zk->witness_density : nullptr);
  };
  // (one window width for both B tables: the G2 model's -- shorter pieces -- as the shared sort is planned for G2)
  auto candidate = [&](MsmTablePtr* slot, int stage) {
    const StageView v = stage_view(zk, stage);
    const int c = stage == kStageH ? force_c : v.array_n ? witness_c(v.array_n, stage == kStageB1 || stage == kStageB2) : 0;
    return Candidate{slot, stage == kStageB2, v.array, v.array_n, c};
  };
  const Candidate tabs[5] = {candidate(&zk->tH, kStageH), candidate(&zk->tC, kStageC), candidate(&zk->tA, kStageA),
                             candidate(&zk->tB1, kStageB1), candidate(&zk->tB2, kStageB2)};
  const int kSingles = 3;   // H, C, A are one step each; the B pair behind them is one step
  const Candidate &tB1 = tabs[kSingles], &tB2 = tabs[kSingles + 1];
  if (release_lanes) {
    // Nothing to build (a 2^27 key: the lanes' workspaces come first): keep the workspaces. Giving back 150 GB and
    // taking it again costs seconds -- the driver wipes released memory before it hands it out (measured: 5 s per lane).
    bool any = !(zk->tB1 && zk->tB2) && tB1.n && fits(tB1.bytes() + tB2.bytes());
    for (int i = 0; i < kSingles; i++) any = any || (!*tabs[i].slot && tabs[i].n && fits(tabs[i].bytes()));
    if (!any) {
      zk->tables_settled = true;
      return zk->table_bytes;
    }
    for (auto& l : ctx->dev.lanes) l.ws.give_back();
  }
  bool more = true;
  // (a table that exists already counts as fitting: its bytes are in table_bytes)
  for (int i = 0; i < kSingles && more; i++) {
    if (!tabs[i].n || !(*tabs[i].slot || fits(tabs[i].bytes()))) continue;
    more = build(tabs[i]);
    if (tabs[i].slot == &zk->tH) zk->tH_cyclic = split && zk->tH;
  }
  if (more && tB1.n && !(zk->tB1 && zk->tB2)) {
    if (step && built >= max_new) {   // the pair is one step's work
      more = false;
      deferred = true;
    } else if (fits(tB1.bytes() + tB2.bytes())) {
      if (step) max_new = built + 2;              // ... and both halves belong to it
      more = build(tB1) && build(tB2);
      if (!more && zk->tB1) {   // the pair is only usable together
        zk->table_bytes -= tB1.bytes();
        zk->tB1.reset();
      }
    }
  }
  // settled: nothing is left for a later step (every wanted table exists, does not fit, or failed to build)
  zk->tables_settled = !deferred;
  return zk->table_bytes;
}

// ---- HBM budget of the five MSM lanes ---------------------------------------------------------------------------
// A lane's workspace is proportional to the points its MSM sorts at once (0.6-0.9 KB per point: 28 GB for the H MSM of a
// 2^26 domain). At the reference's shapes (<= 2^26, 52 M wires) five whole-MSM workspaces, the key and its tables fit in
// 288 GB with room to spare; a key of 2^27 constraints (layer three over four batches) or a card shared with another
// process does not leave that room. The workspaces the stages of the coming proof would reserve (from their plans) are
// therefore added up BEFORE a lane has to grow: if they do not fit in what is free (+ what the lanes hold now), the
// stage with the largest workspace takes its points in halves -- again and again until the sum fits -- and the lanes
// start from empty workspaces. A chunked MSM gives up its fixed-base table and the shared sort of the B query (each is
// indexed by the whole array), so only the stages that must are chunked. What this cannot foresee (a staged one-shot
// prove whose sizes arrive with the file, another process allocating meanwhile) is caught by the failed reservation
// itself: msm_run.
struct LaneNeeds {
  size_t bytes[5] = {0, 0, 0, 0, 0};
  size_t total() const { return bytes[0] + bytes[1] + bytes[2] + bytes[3] + bytes[4]; }
};
static LaneNeeds lane_needs(const zkpoa_context* ctx, const zkpoa_zkey* zk, const uint64_t lim[5], bool with_tables) {
  LaneNeeds w;
  const StageView v[5] = {stage_view(zk, 0), stage_view(zk, 1), stage_view(zk, 2), stage_view(zk, 3), stage_view(zk, 4)};
  const double* dens = zk->have_density ? zk->witness_density : nullptr;
  const bool guard = opt_flag(O_WS_GUARD);   // (tests) the lanes will carve guarded arenas: budget for them
  auto whole_g1 = [&](int l, const double* density) {   // a lane's own G1 MSM: sort and accumulation in one arena
    return msm_workspace(stage_request(ctx, v[l], lim[l], density, false, with_tables), kMsmSort | kMsmAccumG1, guard);
  };
  w.bytes[kStageH] = whole_g1(kStageH, nullptr);   // uniform scalars
  w.bytes[kStageA] = whole_g1(kStageA, dens);      // witness scalars
  w.bytes[kStageC] = whole_g1(kStageC, dens);
  // B (lanes 2 and 3): one sort for both when the whole query fits one
  const uint64_t nB = v[kStageB1].n, limB = std::min(lim[kStageB1], lim[kStageB2]);
  if (nB <= limB) {
    const MsmRequest shared = stage_request(ctx, v[kStageB1], limB, dens, true, with_tables);
    w.bytes[kStageB1] = msm_workspace(shared, kMsmSort | kMsmAccumG1, guard);
    w.bytes[kStageB2] = msm_workspace(shared, kMsmAccumG2, guard);
  } else {   // two chunked MSMs, no table
    w.bytes[kStageB1] = msm_workspace(stage_request(ctx, v[kStageB1], lim[kStageB1], dens, false, false), kMsmSort | kMsmAccumG1, guard);
    // KNOWN MISMATCH (DESIGN.md "MSM plans", follow-up): B2's own MSM runs with no density (prove_partials, tB2)
    w.bytes[kStageB2] = msm_workspace(stage_request(ctx, v[kStageB2], lim[kStageB2], dens, true, false), kMsmSort | kMsmAccumG2, guard);
  }
  return w;
}

static size_t lane_workspace_total(const zkpoa_context* ctx, const zkpoa_zkey* zk, const uint64_t lim[5]) {
  return lane_needs(ctx, zk, lim, false).total();   // classic form: what the lanes need if no table is built
}

static void budget_lane_workspaces(zkpoa_context* ctx, const zkpoa_zkey* zk) {
  uint64_t lim[5];
  for (int l = 0; l < 5; l++) lim[l] = ctx->msm_points_limit(l);
  LaneNeeds w = lane_needs(ctx, zk, lim, true);
  size_t held = 0, after = 0;
  bool grow = false, over_cap = false;
  for (int l = 0; l < 5; l++) {
    const Arena& a = ctx->dev.lanes[l].ws;
    held += a.cap;
    after += std::max(a.cap, w.bytes[l]);
    grow = grow || w.bytes[l] > a.cap;
    over_cap = over_cap || (a.limit && w.bytes[l] > a.cap && w.bytes[l] > a.limit);
  }
  if (!grow) return;   // (the steady state: nothing below runs, no driver call)
  size_t free_b = 0, total_b = 0;
  ZK_HIP(hipMemGetInfo(&free_b, &total_b));
  const double keep = 0.95;   // of what is free: the proof's own temporaries are small beside the workspaces
  if (!over_cap && (double)(after - held) <= keep * (double)free_b) return;
  const double avail = keep * ((double)free_b + (double)held);
  auto fits = [&](const LaneNeeds& x) {
    for (int l = 0; l < 5; l++)
      if (ctx->dev.lanes[l].ws.limit && x.bytes[l] > ctx->dev.lanes[l].ws.limit) return false;
    return (double)x.total() <= avail;
  };
  uint64_t n_of[5];
  for (int l = 0; l < 5; l++) n_of[l] = stage_view(zk, l).n;
  while (!fits(w)) {
    // the lane that is over its cap first, else the one with the largest workspace; its MSM takes half as many points
    int pick = -1;
    for (int l = 0; l < 5; l++)
      if (ctx->dev.lanes[l].ws.limit && w.bytes[l] > ctx->dev.lanes[l].ws.limit && (pick < 0 || w.bytes[l] > w.bytes[pick]))
        pick = l;
    if (pick < 0)
      for (int l = 0; l < 5; l++)
        if (std::min(n_of[l], lim[l]) > (1ull << 16) && (pick < 0 || w.bytes[l] > w.bytes[pick])) pick = l;
    if (pick < 0 || std::min(n_of[pick], lim[pick]) <= (1ull << 16)) break;   // nothing left to halve: the reservation will say so
    lim[pick] = zkpoa_context::below(std::min(n_of[pick], lim[pick]));
    w = lane_needs(ctx, zk, lim, true);
  }
  for (int l = 0; l < 5; l++)
    if (lim[l] < ctx->msm_points_limit(l)) ctx->oom_max_points[l] = lim[l];
  for (int l = 0; l < 5; l++) {   // every lane starts again from what it needs now (nothing is in flight: prove start)
    ZK_HIP(hipStreamSynchronize(ctx->dev.lanes[l].stream));
    ctx->dev.lanes[l].ws.give_back();
  }
  vlog("zkpoa:   HBM budget: %.1f GB free + %.1f GB held by the lanes; MSMs take at most H %llu, A %llu, B1 %llu, B2 %llu, "
       "C %llu points at once (workspaces %.1f GB)\n",
       free_b / 1e9, held / 1e9, (unsigned long long)lim[0], (unsigned long long)lim[1], (unsigned long long)lim[2],
       (unsigned long long)lim[3], (unsigned long long)lim[4], w.total() / 1e9);
}

// Partial MSM results of this handle's shard: A(64) B1(64) B2(128) C(64) H(64). The witness is already
// in zk->d_witness (device). The H-scalar chain runs in full on every rank (replicated).
// Hooks of a one-shot prove that overlaps the key upload with the compute (load_prove_staged): each stage of
// prove_partials first waits for the sections it needs and finishes their key-side preparation on its own lane.
struct Staging {
  std::function<void()> prep_chain, prep_H, prep_A, prep_B, prep_C;
  std::vector<void*> sinks[5];   // temporaries parked until the proof is done (freeing waits for the whole device)
};

void prove_partials(zkpoa_context* ctx, const zkpoa_zkey* zk, uint8_t out[384], Staging* stg = nullptr) {
  auto t0 = std::chrono::steady_clock::now();
  ctx->dev.wait_lanes();
  Lane& l0 = ctx->dev.lanes[0];
  uint8_t* outA = out;
  uint8_t* outB1 = out + 64;
  uint8_t* outB2 = out + 128;
  uint8_t* outC = out + 256;
  uint8_t* outH = out + 320;
  float msm_ms[5][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}};
  // A, B1 and B2 run over the compacted queries (points at infinity dropped at key load) and gathered scalars. Every
  // device pointer is read INSIDE its stage, after the stage's staging hook: a staged prove allocates and fills the
  // buffers while the stages are already waiting (a pointer taken here could still be null).
  const bool split = zk->split_world > 1;
  if (split && !zk->h_ready)
    throw ProverError(PROVER_ERROR, "split chain: run zkpoa_split_stage1/2/3 for this witness before zkpoa_prove_partials");
  if (ctx->ev_witness_set) {   // an asynchronous witness copy (zkpoa_split_stage1) must land before lanes 1-4 read it
    for (int l = 1; l < 5; l++) ZK_HIP(hipStreamWaitEvent(ctx->dev.lanes[l].stream, ctx->ev_witness, 0));
    ctx->ev_witness_set = false;
  }
  auto guarded = [&](int slot, std::function<void()> fn) {
    return SideTask([&, slot, fn] {
      ZK_HIP(hipSetDevice(ctx->dev.device));
      if (stg) deferred_free_sink() = &stg->sinks[slot];
      fn();
    });
  };
  // Witness MSMs on their own lanes (host threads: each MSM has one mid-way read-back). B1 and B2 use the
  // same scalars (the witness values of the wires that occur in the B matrix), so their bucket sort runs once
  // (lane 2) and both accumulations read it; A and C sort on their own lanes.
  std::unique_ptr<MsmSorted> sorted_b;   // owned here: freed after every stage has joined
  std::promise<const MsmSorted*> sorted_promise;
  std::shared_future<const MsmSorted*> sorted_ready = sorted_promise.get_future().share();
  // digit density of this proof's witness (non-zero digits per scalar for every window width), measured once by the
  // first witness stage that gets there, on its own lane; the classic-form witness MSMs size their windows with it
  std::once_flag density_once;
  auto with_density = [&](int lane_id) -> const double* {
    if (opt_flag(O_NO_DENSITY) || !zk->d_flag || !zk->d_witness) return nullptr;
    std::call_once(density_once, [&] {
      if (zk->have_density) return;
      msm_density(ctx->dev.lanes[lane_id].stream, zk->d_witness, zk->nVars, zk->witness_density,
                  zk->d_flag.as<char>() + 256);
      zk->have_density = true;
    });
    return zk->have_density ? zk->witness_density : nullptr;
  };
  // HBM budget of the lanes (a staged prove learns its sizes as the file arrives: msm_run's retry instead). A key's
  // first proof measures the witness's digit density first -- the witness MSMs are planned, and sized, with it
  if (!stg) {
    if (!zk->have_density) (void)with_density(1);
    budget_lane_workspaces(ctx, zk);
  }
  auto gather = [&](int lane_id, const CompactQuery& q) {
    if (q.cnt)
      hipLaunchKernelGGL(gather32_kernel, dim3((uint32_t)((q.cnt * 2 + 255) / 256)), dim3(256), 0,
                         ctx->dev.lanes[lane_id].stream, (const uint4*)zk->d_witness, q.wire.as<const uint32_t>() + q.lo,
                         q.cnt, q.scalars.as<uint4>());
  };
  // opt_prove_serial (measurement only): every stage runs alone, one after the other, so the per-stage device times
  // are solo times and their sum / the overlapped wall time says how much the five lanes gain (bench.py).
  const bool serial = ctx->opt_prove_serial != 0;
  SideTask tA = guarded(0, [&] {
    if (stg && stg->prep_A) stg->prep_A();
    const StageView vA = stage_view(zk, kStageA);
    if (!zk->d_witness || !zk->qA.g1 || !zk->qA.scalars) throw ProverError(PROVER_ERROR, "internal: A stage started before its inputs");
    const double* dens = with_density(1);
    gather(1, zk->qA);
    msm_run_g1(ctx, 1, vA.bases, zk->qA.scalars.get(), vA.n, outA, msm_ms[1], vA.table, dens);
  });
  if (serial) tA.wait();
  // (a B query beyond the 32-bit entry index of one sort cannot share it: two chunked MSMs instead)
  // (nor can one whose whole-query workspace did not fit in HBM on an earlier MSM of this context: msm_points_limit)
  const uint64_t sort_limit = std::min(ctx->msm_points_limit(2), ctx->msm_points_limit(3));
  bool share_b = false;      // set by the B1 stage, read by the B2 stage after the sort has been published
  int table_c_b = 0;
  float sort_b_ms = 0;   // the shared sort of the B query (host clock: the call returns with its stream synchronised)
  SideTask tB1 = guarded(1, [&] {
    StageView vB1;
    const double* dens = nullptr;
    try {
      if (stg && stg->prep_B) stg->prep_B();
      vB1 = stage_view(zk, kStageB1);
      share_b = vB1.n <= sort_limit;
      table_c_b = share_b ? vB1.table_c : 0;
      if (!zk->d_witness || !zk->qB.g1 || !zk->qB.g2 || !zk->qB.scalars)
        throw ProverError(PROVER_ERROR, "internal: B stage started before its inputs");
      dens = with_density(2);
      gather(2, zk->qB);
      auto ts0 = std::chrono::steady_clock::now();
      if (share_b) {
        try {
          sorted_b = msm_sort_run(ctx, 2, zk->qB.scalars.get(), stage_request(ctx, vB1, sort_limit, dens, true));
        } catch (const OomError& e) {   // no room for the whole query's sort: B1 and B2 each go through it in pieces
          if (!ctx->shrink_after_oom(2, zk->qB.cnt)) throw;
          vlog("zkpoa:   B query: %s; B1 and B2 sort their own pieces\n", e.what());
          share_b = false;
          table_c_b = 0;
        }
      }
      if (!share_b) ZK_HIP(hipStreamSynchronize(ctx->dev.lanes[2].stream));   // the gathered scalars are read on lane 3 too
      sort_b_ms = (float)ms_since(ts0);
      sorted_promise.set_value(sorted_b.get());
    } catch (...) {
      sorted_promise.set_exception(std::current_exception());
      throw;
    }
    if (share_b) msm_accum_g1(ctx, 2, sorted_b.get(), true, table_c_b ? msm_table_data(vB1.table) : vB1.bases, outB1, msm_ms[2]);
    else msm_run_g1(ctx, 2, vB1.bases, zk->qB.scalars.get(), vB1.n, outB1, msm_ms[2], nullptr, dens);
    if (share_b) msm_ms[2][0] += sort_b_ms;
  });
  if (serial) tB1.wait();
  SideTask tB2 = guarded(2, [&] {
    const MsmSorted* sr = sorted_ready.get();
    const StageView vB2 = stage_view(zk, kStageB2);
    bool shared = share_b;
    if (shared) {
      try {
        msm_accum_g2(ctx, 3, sr, false, table_c_b ? msm_table_data(vB2.table) : vB2.bases, outB2, msm_ms[3]);
      } catch (const OomError& e) {   // the G2 buckets of the whole query did not fit beside the rest: own sort, in pieces
        if (!ctx->shrink_after_oom(3, zk->qB.cnt)) throw;
        vlog("zkpoa:   B2: %s; sorting its own pieces\n", e.what());
        shared = false;
      }
    }
    // KNOWN MISMATCH (DESIGN.md "MSM plans", follow-up): no density here, while lane_needs sizes this lane with one
    if (!shared) msm_run_g2(ctx, 3, vB2.bases, zk->qB.scalars.get(), vB2.n, outB2, msm_ms[3], nullptr, nullptr);
  });
  if (serial) tB2.wait();
  SideTask tC = guarded(3, [&] {
    if (stg && stg->prep_C) stg->prep_C();
    const StageView vC = stage_view(zk, kStageC);
    const char* witC = reinterpret_cast<const char*>(zk->d_witness) + ((uint64_t)zk->nPublic + 1 + vC.scalar_off) * 32;
    if (!zk->d_witness || (vC.n && !vC.bases)) throw ProverError(PROVER_ERROR, "internal: C stage started before its inputs");
    if (zk->bc_log) {   // block-cyclic shard: the scalars of this rank's blocks, gathered in the order of its points
      if (zk->ccnt)
        hipLaunchKernelGGL(gather_bc32_kernel, dim3((uint32_t)((zk->ccnt * 2 + 255) / 256)), dim3(256), 0,
                           ctx->dev.lanes[4].stream,
                           reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(zk->d_witness) + ((uint64_t)zk->nPublic + 1) * 32),
                           zk->ccnt, zk->bc_log, zk->bc_rank, zk->bc_world, zk->d_cscal.as<uint4>());
      witC = zk->d_cscal.as<const char>();
    }
    msm_run_g1(ctx, 4, vC.bases, witC, vC.n, outC, msm_ms[4], vC.table, with_density(4));
  });
  if (serial) tC.wait();

  std::exception_ptr main_err;
  uint32_t witness_bad = 0;
  try {
    if (stg) deferred_free_sink() = &stg->sinks[4];
    if (stg && stg->prep_chain) stg->prep_chain();
    if (!zk->d_witness || !zk->d_flag || (!split && (!zk->d_abc || !zk->d_row_ptr)))
      throw ProverError(PROVER_ERROR, "internal: chain stage started before its inputs");
    // witness values must be canonical (< r): one streaming pass on the chain's lane, flag read with the H MSM's results
    ZK_HIP(hipMemsetAsync(zk->d_flag.get(), 0, 4, l0.stream));
    range_check<FrParams>(l0.stream, zk->d_witness, zk->nVars, zk->d_flag.as<uint32_t>());
    KernelTimer chain = KernelTimer::chain(ctx, l0.stream);
    chain.start();
    if (!split)
      h_chain(ctx, l0.stream, zk->d_row_ptr.as<uint32_t>(), zk->d_sig.as<uint32_t>(), zk->d_vals.get(),
              zk->d_long.as<uint32_t>(), zk->n_long, zk->d_witness, zk->domain, zk->power, zk->d_abc.get());
    chain.stop();
    if (stg && stg->prep_H) stg->prep_H();
    const StageView vH = stage_view(zk, kStageH);
    if (vH.n && !vH.bases) throw ProverError(PROVER_ERROR, "internal: H stage started before its inputs");
    // (a split handle: the three stages left this rank's H scalars, odd-coset indices = rank mod G, in d_abc[0 .. n/G))
    msm_run_g1(ctx, 0, vH.bases, zk->d_abc.as<const char>() + vH.scalar_off * 32, vH.n, outH, msm_ms[0],
               vH.table);
    if (split) zk->h_ready = false;
    chain.store(kMsChain);   // no wait of its own: the H MSM, later on the same stream, has returned
    msm_read_back(l0, zk->d_flag.get(), 4);   // lane 0 is idle (its MSM has returned): the flag through its pinned buffer
    witness_bad = *l0.pinned.as<const uint32_t>();
  } catch (...) {
    main_err = std::current_exception();
  }
  deferred_free_sink() = nullptr;
  for (SideTask* t : {&tA, &tB1, &tB2, &tC}) t->wait();
  sorted_b.reset();
  if (main_err) std::rethrow_exception(main_err);
  for (SideTask* t : {&tA, &tB1, &tB2, &tC}) t->get();
  if (witness_bad) throw ProverError(PROVER_ERROR, "witness value is not a field element (>= r)");
  auto t1 = std::chrono::steady_clock::now();
  ctx->ms[kMsMsmPhase] = std::chrono::duration<float, std::milli>(t1 - t0).count();
  ctx->ms[kMsMsm] = msm_ms[0][0];
  ctx->ms[kMsMsmAccum] = msm_ms[0][1];
  for (int l = 0; l < 5; l++) {   // per-lane MSM timings (H, A, B1, B2, C): zkpoa_last_ms_lane
    ctx->lane_ms[l][0] = msm_ms[l][0];
    ctx->lane_ms[l][1] = msm_ms[l][1];
  }
}

// header: alpha1(64) beta1(64) beta2(128) delta1(64) delta2(128); sums: A B1 B2 C H summed over all shards.
// Randomised assembly (groth16_prove.js tail). Host only.
void prove_assemble(const HeaderPoints& h, const uint8_t sums[384], const uint8_t* r_le, const uint8_t* s_le,
                    uint8_t proof_points[256]) {
  uint8_t rb[32], sb[32];
  if (r_le) memcpy(rb, r_le, 32); else random_scalar(rb);
  if (s_le) memcpy(sb, s_le, 32); else random_scalar(sb);
  uint64_t rk[4], sk[4], nrs[4];
  memcpy(rk, rb, 32);
  memcpy(sk, sb, 32);
  HFr rs = hfr_from_le(rb).to_mont() * hfr_from_le(sb).to_mont();
  rs.neg().from_mont().to_bytes(nrs);

  XYZZ<HFq> d1 = XYZZ<HFq>::from_affine(h.delta1);
  XYZZ<HFq2> d2 = XYZZ<HFq2>::from_affine(h.delta2);
  XYZZ<HFq> pi_a = XYZZ<HFq>::from_affine(h_affine_from_bytes<HFq>(sums));
  xyzz_add_affine(pi_a, h.alpha1, false);
  xyzz_add(pi_a, h_mul(d1, rk));
  XYZZ<HFq2> pi_b = XYZZ<HFq2>::from_affine(h_affine_from_bytes<HFq2>(sums + 128));
  xyzz_add_affine(pi_b, h.beta2, false);
  xyzz_add(pi_b, h_mul(d2, sk));
  XYZZ<HFq> pib1 = XYZZ<HFq>::from_affine(h_affine_from_bytes<HFq>(sums + 64));
  xyzz_add_affine(pib1, h.beta1, false);
  xyzz_add(pib1, h_mul(d1, sk));
  XYZZ<HFq> pi_c = XYZZ<HFq>::from_affine(h_affine_from_bytes<HFq>(sums + 256));
  xyzz_add_affine(pi_c, h_affine_from_bytes<HFq>(sums + 320), false);
  xyzz_add(pi_c, h_mul(pi_a, sk));
  xyzz_add(pi_c, h_mul(pib1, rk));
  xyzz_add(pi_c, h_mul(d1, nrs));

  h_affine_to_bytes<HFq>(h_to_affine(pi_a), proof_points);
  h_affine_to_bytes<HFq2>(h_to_affine(pi_b), proof_points + 64);
  h_affine_to_bytes<HFq>(h_to_affine(pi_c), proof_points + 192);
}

// the partial sums of a whole key -> proof points; ctx->ms[kMsProve] <- the prove time, counted from t0
void assemble_proof(zkpoa_context* ctx, const zkpoa_zkey* zk, const uint8_t parts[384], const uint8_t* r_le,
                    const uint8_t* s_le, std::chrono::steady_clock::time_point t0, uint8_t proof_points[256]) {
  prove_assemble(zk->hdr, parts, r_le, s_le, proof_points);
  ctx->ms[kMsProve] = (float)ms_since(t0);
}

// unsharded prove = partials of the whole key + assembly
void prove_core(zkpoa_context* ctx, const zkpoa_zkey* zk, const uint8_t* r_le, const uint8_t* s_le,
                uint8_t proof_points[256]) {
  auto t0 = std::chrono::steady_clock::now();
  if (!is_full_key(zk))
    throw ProverError(PROVER_ERROR, "this key handle is a shard: use zkpoa_prove_partials + zkpoa_prove_assemble");
  uint8_t parts[384];
  prove_partials(ctx, zk, parts);
  assemble_proof(ctx, zk, parts, r_le, s_le, t0, proof_points);
}

// Self-check (ZKPOA_SELFCHECK): the reference verifies every proof right after proving it
// (scripts/g16_verify.sh:213-216, full_workflow.sh:503-504); a zkey carries its own verification key, so the prover
// can run the same pairing check before anything is written. "0" = never, unset / "1" = the first proof of every key
// handle (a key whose conventions differ from SURVEY.md 8c fails on first contact, not downstream), "all" = every
// proof. Host only (csrc/verify.hip, ~7 ms). Keys without section 3 / assembled from device buffers are skipped.
int selfcheck_mode() {
  static const int kMode[] = {1, 0, 0, 2, 2};   // of the row's words: 1 | 0 | off | all | 2
  return kMode[opt_choice(O_SELFCHECK)];
}

struct SelfCheckFailed : ProverError {   // the proof was computed and does not verify (as opposed to "could not be checked")
  explicit SelfCheckFailed(const std::string& s) : ProverError(PROVER_ERROR, s) {}
};

// first_n: in the default mode the first that many proofs of a key are checked (1; the multi-GPU path checks 3: a stale
// exchange buffer can only show from the second proof on)
void selfcheck(zkpoa_context* ctx, const zkpoa_zkey* zk, const uint8_t proof_points[256], const uint8_t* public_le,
               uint64_t first_n = 1) {
  ctx->ms[kMsSelfCheck] = 0;
  const int mode = selfcheck_mode();
  if (mode == 0 || zk->vkey_points.empty() || (mode == 1 && zk->selfchecks_done >= first_n)) return;
  auto t0 = std::chrono::steady_clock::now();
  char msg[256] = {0};
  int rc = zkpoa_groth16_verify_points(zk->vkey_points.data(), (unsigned long)zk->vkey_points.size(), proof_points,
                                       public_le, zk->nPublic, msg, sizeof(msg));
  ctx->ms[kMsSelfCheck] = (float)ms_since(t0);
  if (rc == PROVER_OK) {
    zk->selfchecks_done++;
    vlog("zkpoa: self-check: proof verifies against the zkey's own verification key (%.1f ms)\n", ctx->ms[kMsSelfCheck]);
    return;
  }
  if (rc == ZKPOA_VERIFY_INVALID_PROOF)
    throw SelfCheckFailed(
                      "self-check failed: the proof does not verify against the verification key inside the zkey "
                      "(sections 2-3). Either the witness does not satisfy the circuit, or this zkey does not follow the "
                      "conventions the prover assumes: section 4 coefficients stored as coef*R^2 mod r; section 9 H points = "
                      "Lagrange basis of the odd coset of the 2n-th roots (no division by Z); section 8 C points starting at "
                      "wire nPublic+1; all points affine in Montgomery form. Set ZKPOA_SELFCHECK=0 to write the proof anyway.");
  throw ProverError(PROVER_ERROR, std::string("self-check could not run: ") + msg);
}

// witness (its length checked by the caller) -> the key's buffer on lane 0, then prove_core; io_ms <- the upload
void upload_and_prove(zkpoa_context* ctx, const zkpoa_zkey* zk, const WtnsView& w, const uint8_t* r_le,
                      const uint8_t* s_le, uint8_t proof_points[256]) {
  const auto tu = std::chrono::steady_clock::now();
  w.upload(ctx, zk->d_witness, 0, w.n, ctx->dev.lanes[0].stream);
  ctx->io_ms[0] = (float)ms_since(tu);
  ctx->io_ms[1] = (float)((double)w.n * 32 / 1e6);
  prove_core(ctx, zk, r_le, s_le, proof_points);
}

void prove_impl(zkpoa_context* ctx, const zkpoa_zkey* zk, const WtnsSrc& wsrc,
                const uint8_t* r_le, const uint8_t* s_le, uint8_t proof_points[256], uint8_t* public_le,
                uint64_t public_cap) {
  WtnsView w = parse_wtns(wsrc);
  check_witness_len(w, zk);
  if (public_cap < (uint64_t)zk->nPublic * 32) throw ProverError(PROVER_ERROR_SHORT_BUFFER, "public buffer too small");
  upload_and_prove(ctx, zk, w, r_le, s_le, proof_points);
  std::vector<uint8_t> pub_store;
  const uint8_t* pubs = w.publics(zk->nPublic, pub_store);
  memcpy(public_le, pubs, (size_t)zk->nPublic * 32);
  selfcheck(ctx, zk, proof_points, pubs);
}

// ---- one-shot prove with the key upload overlapped ------------------------------------------
// A one-shot `prover` run spends most of its time moving the key over PCIe (1 GB for layer one, 21 GB for layer
// three), and none of the compute needs the whole key: the H-scalar chain needs the witness and section 4, the H MSM
// section 9, the B MSMs sections 6 + 7, A section 5, C section 8. So the sections go up on a stream of their own in
// the order  witness, 4, 9, 6, 7, 5, 8  (the stage with the least work after its last byte arrives goes last) while
// every stage of prove_partials starts as soon as its own inputs are resident and does the key-side preparation of
// that section (CSR build, dropping the points at infinity, range checks) on its own lane. Wall time tends to
// max(upload, compute) + the C MSM instead of upload + compute. Returns the loaded key (complete, reusable: the cache
// keeps it) with `parts` = the five MSM results; nullptr when no copy stream could be created (caller: plain path).
// zkey_fd >= 0: the file `buf` maps; the sections are then read with pread instead of through the mapping.
//
// What is destroyed when, on the way out -- the one place where the order matters, so it is the declaration order: the
// handle `zk` is declared first and therefore goes LAST. Before it, in reverse order of declaration: `ending` cancels
// and joins the uploader (nobody writes into the handle's arrays any more), drains the device and frees the parked
// temporaries; then the staging hooks, the record and flag temporaries and the hold-back go; only then, on failure,
// the handle frees its arrays (on success it has been moved out to the caller).
KeyPtr load_prove_staged(zkpoa_context* ctx, const uint8_t* buf, uint64_t size, const WtnsView& w, uint8_t parts[384],
                         int zkey_fd = -1) {
  hipStream_t cs = ctx->dev.copy_stream_wait();
  if (!cs) return nullptr;
  ZkeySections zs;
  KeyPtr zk = zkey_parse(buf, size, zs);
  check_witness_len(w, zk.get());
  shard_init(zk.get(), 0, 1, false, 0);   // the whole key
  const uint64_t m = zk->nVars, n = zk->domain, nC = m - zk->nPublic - 1;
  {
    // What the overlapped form holds at its peak: the sections AND the compacted copies of the A / B queries (freeing
    // would wait for the whole device, so the originals are only given back after the proof), the coefficient records
    // AND their CSR form, the chain's work area, the witness -- plus the lanes' workspaces. A key for which that leaves
    // the lanes less than a quarter of the card (2^28: 247 of 309 GB; 2^27: 125) is loaded first and proved afterwards (the caller's
    // sequential path: temporaries freed as it goes, then the lanes' HBM budget of prove_partials).
    size_t free_b = 0, total_b = 0;
    ZK_HIP(hipMemGetInfo(&free_b, &total_b));
    const double peak = (double)n * 64 + (double)m * (64 + 128 + 64) + (double)nC * 64 + (double)m * 32 +
                        (double)zk->nCoefs * (44 + 36) + (double)n * (8 + 96) + (double)m * (108 + 236);
    if (peak > 0.72 * (double)total_b || peak > 0.8 * (double)free_b) {
      vlog("zkpoa: the overlapped load would hold %.0f GB at its peak (%.0f GB free of %.0f): loading the key first\n",
           peak / 1e9, free_b / 1e9, total_b / 1e9);
      return nullptr;
    }
  }
  // What of that is still to be allocated while the lanes already reserve their workspaces: every part is taken off as
  // it is allocated, and a lane that would eat into the rest halves its piece instead (Arena::reserve, msm_run).
  struct HoldBack {
    std::atomic<int64_t>& v;
    explicit HoldBack(std::atomic<int64_t>& x, double bytes) : v(x) { v = (int64_t)bytes; }
    void done(double bytes) {
      if (v.fetch_sub((int64_t)bytes) - (int64_t)bytes < 0) v = 0;
    }
    ~HoldBack() { v = 0; }
  } hold(ctx->key_hold_back, (double)n * 64 + (double)m * 256 + (double)nC * 64 + (double)zk->nCoefs * 36 +
                               (double)n * (8 + 96) + (double)m * (108 + 236));
  zkpoa_zkey* k = zk.get();
  k->device = ctx->dev.device;   // from here on the handle holds device memory
  DevMem d_recs, d_cflag;   // the coefficient records until the CSR exists; the flag word of the coordinate checks
  enum { S_WIT, S_COEF, S_H, S_B1, S_B2, S_A, S_C, S_COUNT };
  std::promise<void> ready[S_COUNT];
  std::shared_future<void> have[S_COUNT];
  for (int i = 0; i < S_COUNT; i++) have[i] = ready[i].get_future().share();
  std::atomic<bool> cancel{false};
  std::thread uploader;   // not a SideTask: cancel, join and drain the device are one unit (Ending), in that order
  Staging stg;
  const bool verbose = opt_verbose();
  const auto t_start = std::chrono::steady_clock::now();
  auto mark = [&, verbose](const char* what) {   // ZKPOA_VERBOSE: the timeline of an overlapped load + prove
    if (verbose)
      fprintf(stderr, "zkpoa: staged %7.1f ms  %s\n", ms_since(t_start), what);
  };
  auto cleanup_temps = [&] {
    (void)hipDeviceSynchronize();
    for (auto& v : stg.sinks) free_deferred(v);
  };
  struct Ending {   // however the function is left (the success path has done all of it already)
    std::atomic<bool>& cancel;
    std::thread& uploader;
    std::function<void()> cleanup;
    bool done = false;
    ~Ending() {
      if (done) return;
      cancel.store(true);
      if (uploader.joinable()) uploader.join();
      cleanup();
    }
  } ending{cancel, uploader, cleanup_temps};
  d_cflag.alloc(64);
  uint32_t* const cflag = d_cflag.as<uint32_t>();
  ZK_HIP(hipMemsetAsync(cflag, 0, 64, ctx->dev.lanes[0].stream));   // stream-ordered, then waited for: the range checks
  ZK_HIP(hipStreamSynchronize(ctx->dev.lanes[0].stream));            // that OR into it run on other (non-blocking) streams
  k->wbuf[0].alloc(m * 32);
  k->d_witness = k->wbuf[0].get();
  d_recs.alloc(zk->nCoefs * 44);
  k->d_flag.alloc(1024);
  // each buffer is allocated by the uploader right before its section moves (hipMalloc of GBs is milliseconds each)
  struct Item { int id; DevMem* dst; const uint8_t* src; uint64_t bytes; };
  const Item items[S_COUNT] = {
      {S_WIT, &k->wbuf[0], w.values /* null: from w.fd */, m * 32}, {S_COEF, &d_recs, zs.s4.p + 4, zk->nCoefs * 44},
      {S_H, &k->dH, zs.s9.p, n * 64},           {S_B1, &k->dB1, zs.s6.p, m * 64},
      {S_B2, &k->dB2, zs.s7.p, m * 128},        {S_A, &k->dA, zs.s5.p, m * 64},
      {S_C, &k->dC, zs.s8.p, nC * 64}};
  uploader = std::thread([&] {
    int i = 0;
    try {
      ZK_HIP(hipSetDevice(ctx->dev.device));
      for (; i < S_COUNT; i++) {
        if (cancel.load()) throw ProverError(PROVER_ERROR, "upload cancelled");
        const Item& it = items[i];
        if (!*it.dst) {
          it.dst->alloc(it.bytes);
          hold.done((double)it.bytes);
        }
        if (it.bytes) {
          if (it.id == S_WIT && w.fd >= 0) {   // file-backed witness: pread into the pinned staging buffers
            std::vector<uint8_t> small;
            if (it.bytes < (4u << 20)) {
              small.resize(it.bytes);
              w.read(0, w.n, small.data());
              ZK_HIP(hipMemcpyAsync(it.dst->get(), small.data(), it.bytes, hipMemcpyHostToDevice, cs));
              ZK_HIP(hipStreamSynchronize(cs));
            } else {
              ctx->uploader.upload(it.dst->get(), nullptr, it.bytes, ctx->dev.device, cs, w.fd, w.off);
            }
          } else if (it.bytes < (4u << 20)) {   // small: one asynchronous copy on the copy stream (no null-stream copy here)
            ZK_HIP(hipMemcpyAsync(it.dst->get(), it.src, it.bytes, hipMemcpyHostToDevice, cs));
            ZK_HIP(hipStreamSynchronize(cs));
          } else {
            const bool from_file = zkey_fd >= 0 && it.src >= buf && it.src < buf + size;
            ctx->uploader.upload(it.dst->get(), it.src, it.bytes, ctx->dev.device, cs, from_file ? zkey_fd : -1,
                                 from_file ? (uint64_t)(it.src - buf) : 0);
          }
        }
        ready[it.id].set_value();
        static const char* kNames[S_COUNT] = {"witness resident", "section 4 resident", "section 9 (H) resident",
                                              "section 6 (B1) resident", "section 7 (B2) resident",
                                              "section 5 (A) resident", "section 8 (C) resident"};
        mark(kNames[it.id]);
      }
    } catch (...) {
      for (; i < S_COUNT; i++) ready[items[i].id].set_exception(std::current_exception());
    }
  });
  ctx->dev.wait_lanes();   // the other lanes come up in the background while the first sections are already moving
  Lane* L = ctx->dev.lanes;
  // (every coordinate check runs on the lane of the stage that reads the section)
  stg.prep_chain = [&, k] {
    have[S_WIT].get();
    have[S_COEF].get();
    build_csr(ctx, k, d_recs.get(), false, L[0].stream);
    ntt_prepare(ctx, L[0].stream, k->power);
    hold.done((double)k->nCoefs * 36 + (double)n * (8 + 96));
    mark("CSR + NTT tables built, H-scalar chain starts");
  };
  stg.prep_H = [&, k] {
    mark("H-scalar chain enqueued");
    have[S_H].get();
    section_range_check(k, kSecH, L[0].stream, cflag);
  };
  stg.prep_A = [&, k] {
    have[S_WIT].get();
    have[S_A].get();
    section_range_check(k, kSecA, L[1].stream, cflag);
    query_compact(ctx, k, k->qA, k->dA.get(), nullptr, m, L[1].stream);
    hold.done((double)m * 108);
    mark("A query compacted, A MSM starts");
  };
  stg.prep_B = [&, k] {
    have[S_WIT].get();
    have[S_B1].get();
    have[S_B2].get();
    section_range_check(k, kSecB1, L[2].stream, cflag);
    section_range_check(k, kSecB2, L[2].stream, cflag);
    query_compact(ctx, k, k->qB, k->dB1.get(), k->dB2.get(), m, L[2].stream);
    hold.done((double)m * 236);
    mark("B query compacted, B MSMs start");
  };
  stg.prep_C = [&, k] {
    have[S_WIT].get();
    have[S_C].get();
    section_range_check(k, kSecC, L[4].stream, cflag);
  };
  mark("lanes up");
  prove_partials(ctx, k, parts, &stg);
  mark("all five MSMs done");
  uploader.join();
  uint32_t bad = 0;
  ZK_HIP(hipDeviceSynchronize());
  ZK_HIP(hipMemcpy(&bad, cflag, 4, hipMemcpyDeviceToHost));
  if (bad) throw ProverError(PROVER_ERROR, "zkey point coordinate is not a field element (>= q)");
  // the originals of the compacted queries are not read again: they go with the parked temporaries (take() + push_back,
  // the one way a member of the handle ever gets into a sink)
  for (DevMem* sec : {&k->dA, &k->dB1, &k->dB2}) stg.sinks[4].push_back(sec->take());
  cleanup_temps();
  ending.done = true;
  mark("temporaries freed");
  return zk;
}

#include "multi_device.hip.h"   // several GPUs: the device set of the process, sharded keys and their proof
#include "prove_request.hip.h"  // zkey + witness -> key cache -> proof -> self-check -> the two JSON texts

}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------
// The frame of an entry point that works on ctx's device: body() runs there; what it throws becomes the return code
// and ctx's last_error. Null arguments are the entry point's own business, before the call.
template <class Body>
static int abi_call(zkpoa_context* ctx, Body&& body) {
  try {
    ZK_HIP(hipSetDevice(ctx->dev.device));
    body();
  } catch (const std::exception& e) {
    ctx->last_error = e.what();
    const ProverError* pe = dynamic_cast<const ProverError*>(&e);
    return pe ? pe->code : PROVER_ERROR;
  }
  return PROVER_OK;
}

// what the four loaders from a zkey image share; `shard` = the entry point's own arguments to zkey_load_impl
template <class... Shard>
static int zkey_load_abi(zkpoa_context* ctx, const void* zkey_buffer, unsigned long zkey_size, zkpoa_zkey** out, Shard... shard) {
  if (!ctx || !out || !zkey_buffer) return PROVER_ERROR;
  *out = nullptr;
  return abi_call(ctx, [&] { *out = zkey_load_impl(ctx, static_cast<const uint8_t*>(zkey_buffer), zkey_size, shard...).release(); });
}

extern "C" int zkpoa_zkey_load(zkpoa_context* ctx, const void* zkey_buffer, unsigned long zkey_size, zkpoa_zkey** out) {
  return zkey_load_abi(ctx, zkey_buffer, zkey_size, out);
}

extern "C" int zkpoa_zkey_load_shard(zkpoa_context* ctx, const void* zkey_buffer, unsigned long zkey_size,
                                     uint64_t rank, uint64_t world, zkpoa_zkey** out) {
  return zkey_load_abi(ctx, zkey_buffer, zkey_size, out, rank, world);
}

extern "C" int zkpoa_zkey_load_shard_split(zkpoa_context* ctx, const void* zkey_buffer, unsigned long zkey_size,
                                           uint64_t rank, uint64_t world, zkpoa_zkey** out) {
  return zkey_load_abi(ctx, zkey_buffer, zkey_size, out, rank, world, true);
}

extern "C" int zkpoa_zkey_load_shard_ex(zkpoa_context* ctx, const void* zkey_buffer, unsigned long zkey_size,
                                        uint64_t rank, uint64_t world, int flags, zkpoa_zkey** out) {
  return zkey_load_abi(ctx, zkey_buffer, zkey_size, out, rank, world, (flags & ZKPOA_SHARD_SPLIT_CHAIN) != 0,
                       ZKPOA_SHARD_BLOCK_LOG(flags));
}

extern "C" int zkpoa_zkey_set_shard(zkpoa_zkey* zkey, uint64_t rank, uint64_t world) {
  if (!zkey || world == 0 || rank >= world) return PROVER_ERROR;
  if (!resident_unsharded(zkey)) return PROVER_ERROR;
  zkey->set_shard(rank, world);
  zkey->split_world = zkey->split_rank = zkey->split_log = 0;
  zkey->h_ready = false;
  try {
    queries_set_slice(zkey);
  } catch (const std::exception&) {
    return PROVER_ERROR;
  }
  return PROVER_OK;
}

extern "C" int zkpoa_zkey_set_shard_split(zkpoa_context* ctx, zkpoa_zkey* zkey, uint64_t rank, uint64_t world) {
  if (!ctx || !zkey) return PROVER_ERROR;
  return abi_call(ctx, [&] {
    if (!resident_unsharded(zkey)) throw ProverError(PROVER_ERROR, "only a fully resident key can be re-sharded");
    check_split(zkey, rank, world);
    hipStream_t st = ctx->dev.lanes[0].stream;
    const uint64_t cnt = zkpoa_zkey::split_h_count(zkey->domain, world);
    zkey->release_cyclic_h_table();
    zkey->dHs.alloc(cnt * 64);   // (the old shard is freed first)
    hipLaunchKernelGGL(strided_copy64_kernel, dim3((uint32_t)((cnt * 4 + 255) / 256)), dim3(256), 0, st,
                       zkey->dH.as<const uint4>(), zkey->dHs.as<uint4>(), cnt, (uint32_t)rank, (uint32_t)world);
    zkey->set_shard(rank, world);
    queries_set_slice(zkey);
    set_split(zkey, rank, world);
    ntt_prepare(ctx, st, zkey->power - zkey->split_log);
    finish(st);
  });
}

// A .wtns image in host memory, parsed and checked against the key and the caller's room for the public signals:
// what zkpoa_witness_load and zkpoa_prove_partials do before anything moves.
static WtnsView host_witness(const zkpoa_zkey* zk, const void* wtns_buffer, unsigned long wtns_size, const uint8_t* public_le,
                             unsigned long public_capacity) {
  WtnsView w = parse_wtns(reinterpret_cast<const uint8_t*>(wtns_buffer), wtns_size);
  check_witness_len(w, zk);
  if (public_le && public_capacity < (unsigned long)zk->nPublic * 32)
    throw ProverError(PROVER_ERROR_SHORT_BUFFER, "public buffer too small");
  return w;
}

extern "C" int zkpoa_witness_load(zkpoa_context* ctx, const zkpoa_zkey* zkey, const void* wtns_buffer,
                                  unsigned long wtns_size, uint8_t* public_le, unsigned long public_capacity) {
  if (!ctx || !zkey || !wtns_buffer) return PROVER_ERROR;
  return abi_call(ctx, [&] {
    const WtnsView w = host_witness(zkey, wtns_buffer, wtns_size, public_le, public_capacity);
    w.upload(ctx, zkey->d_witness, 0, w.n, ctx->dev.lanes[0].stream);
    zkey->h_ready = false;
    if (public_le) memcpy(public_le, w.values + 32, (size_t)zkey->nPublic * 32);
  });
}

extern "C" int zkpoa_split_stage1(zkpoa_context* ctx, const zkpoa_zkey* zkey, const void* d_witness, void* d_exchange) {
  if (!ctx || !zkey || !d_exchange) return PROVER_ERROR;
  return abi_call(ctx, [&] {
    if (zkey->split_world < 2) throw ProverError(PROVER_ERROR, "split chain: the key handle is not a split shard");
    hipStream_t st = ctx->dev.lanes[0].stream;
    if (d_witness && d_witness != zkey->d_witness) {
      ZK_HIP(hipMemcpyAsync(zkey->d_witness, d_witness, (size_t)zkey->nVars * 32, hipMemcpyDeviceToDevice, st));
      ctx->record_witness_event(st);   // the witness MSMs run on other lanes: they wait for this copy
    }
    split_stage1(ctx, zkey, d_exchange);
  });
}

extern "C" int zkpoa_split_stage2(zkpoa_context* ctx, const zkpoa_zkey* zkey, const void* d_received, void* d_exchange) {
  if (!ctx || !zkey || !d_received || !d_exchange || d_received == d_exchange) return PROVER_ERROR;
  return abi_call(ctx, [&] {
    if (zkey->split_world < 2) throw ProverError(PROVER_ERROR, "split chain: the key handle is not a split shard");
    split_stage2(ctx, zkey, d_received, d_exchange);
  });
}

extern "C" int zkpoa_split_stage3(zkpoa_context* ctx, const zkpoa_zkey* zkey, void* d_received) {
  if (!ctx || !zkey || !d_received) return PROVER_ERROR;
  return abi_call(ctx, [&] {
    if (zkey->split_world < 2) throw ProverError(PROVER_ERROR, "split chain: the key handle is not a split shard");
    split_stage3(ctx, zkey, d_received);
  });
}

extern "C" void* zkpoa_context_stream(zkpoa_context* ctx, int lane) {
  if (!ctx || lane < 0 || lane >= DeviceCtx::kLanes) return nullptr;
  try {
    if (lane) ctx->dev.wait_lanes();
    ctx->dev.ensure_lane(lane);   // lanes beyond the eager ones are created on first use: never hand out a null stream
  } catch (const std::exception&) {
    return nullptr;
  }
  return reinterpret_cast<void*>(ctx->dev.lanes[lane].stream.s);
}

extern "C" int zkpoa_context_synchronize(zkpoa_context* ctx) {
  if (!ctx) return PROVER_ERROR;
  return abi_call(ctx, [&] {
    finish(ctx->dev.lanes[0].stream);
  });
}

extern "C" int zkpoa_zkey_header(const zkpoa_zkey* zkey, uint8_t header_points[448]) {
  if (!zkey || !header_points) return PROVER_ERROR;
  zkey_header_bytes(zkey, header_points);
  return PROVER_OK;
}

extern "C" int zkpoa_prove_partials(zkpoa_context* ctx, const zkpoa_zkey* zkey, const void* wtns_buffer,
                                    unsigned long wtns_size, uint8_t partials[384], uint8_t* public_le,
                                    unsigned long public_capacity) {
  if (!ctx || !zkey || !wtns_buffer || !partials) return PROVER_ERROR;
  return abi_call(ctx, [&] {
    const WtnsView w = host_witness(zkey, wtns_buffer, wtns_size, public_le, public_capacity);
    if (zkey->split_world > 1)
      throw ProverError(PROVER_ERROR, "split chain: use zkpoa_witness_load, zkpoa_split_stage1/2/3, then "
                                      "zkpoa_prove_partials_device with a NULL witness");
    w.upload(ctx, zkey->d_witness, 0, w.n, ctx->dev.lanes[0].stream);
    prove_partials(ctx, zkey, partials);
    if (public_le) memcpy(public_le, w.values + 32, (size_t)zkey->nPublic * 32);
  });
}

extern "C" int zkpoa_prove_partials_device(zkpoa_context* ctx, const zkpoa_zkey* zkey, const void* d_witness,
                                           uint8_t partials[384]) {
  if (!ctx || !zkey || !partials) return PROVER_ERROR;
  return abi_call(ctx, [&] {
    hipStream_t st = ctx->dev.lanes[0].stream;
    if (d_witness && d_witness != zkey->d_witness) {
      ZK_HIP(hipMemcpyAsync(zkey->d_witness, d_witness, (size_t)zkey->nVars * 32, hipMemcpyDeviceToDevice, st));
      ZK_HIP(hipStreamSynchronize(st));
    }
    prove_partials(ctx, zkey, partials);
  });
}

extern "C" int zkpoa_prove_assemble(const uint8_t header_points[448], const uint8_t partial_sums[384],
                                    const uint8_t* r_le, const uint8_t* s_le, uint8_t proof_points[256]) {
  if (!header_points || !partial_sums || !proof_points) return PROVER_ERROR;
  try {
    prove_assemble(header_points_from_bytes(header_points), partial_sums, r_le, s_le, proof_points);
  } catch (const std::exception&) {
    return PROVER_ERROR;
  }
  return PROVER_OK;
}

extern "C" void zkpoa_zkey_free(zkpoa_context*, zkpoa_zkey* zkey) { KeyPtr dying(zkey); }

extern "C" int zkpoa_zkey_info(const zkpoa_zkey* zkey, uint64_t out[4]) {
  if (!zkey || !out) return PROVER_ERROR;
  out[0] = zkey->nVars;
  out[1] = zkey->nPublic;
  out[2] = zkey->domain;
  out[3] = zkey->nCoefs;
  return PROVER_OK;
}

extern "C" int zkpoa_prove(zkpoa_context* ctx, const zkpoa_zkey* zkey, const void* wtns_buffer, unsigned long wtns_size,
                           const uint8_t* r_le, const uint8_t* s_le, uint8_t proof_points[256], uint8_t* public_le,
                           unsigned long public_capacity) {
  if (!ctx || !zkey || !wtns_buffer || !proof_points) return PROVER_ERROR;
  return abi_call(ctx, [&] {
    uint8_t dummy[1];
    prove_impl(ctx, zkey, WtnsSrc{reinterpret_cast<const uint8_t*>(wtns_buffer), wtns_size, -1}, r_le, s_le, proof_points,
               public_le ? public_le : dummy, public_le ? public_capacity : (zkey->nPublic ? 0 : 1));
  });
}

// Key (or one rank's shard of it) from sections already in HBM. world == 1: the whole key. world > 1: the point
// buffers hold only this rank's index ranges (zkpoa_zkey::split: the ranges zkpoa_zkey_load_shard uploads); with
// `split`, d_H is the cyclic shard H[t * world + rank] and the records are those of the constraints
// c = rank (mod world) (records of other constraints are ignored).
extern "C" int zkpoa_zkey_load_device_shard(zkpoa_context* ctx, uint64_t n_vars, uint64_t n_public, unsigned log_domain,
                                            uint64_t rank, uint64_t world, int flags, const void* d_A,
                                            const void* d_B1, const void* d_B2, const void* d_C, const void* d_H,
                                            const void* d_coef_records, uint64_t n_coefs,
                                            const uint8_t header_points[448], zkpoa_zkey** out) {
  if (!ctx || !out || !header_points) return PROVER_ERROR;
  *out = nullptr;
  const bool split = (flags & ZKPOA_SHARD_SPLIT_CHAIN) != 0;
  return abi_call(ctx, [&] {
    KeyPtr zk(new zkpoa_zkey());
    if (log_domain > 28 || n_vars == 0 || n_vars > (1ull << 28) || n_public + 1 > n_vars || n_coefs > 0xffffffffull)
      throw ProverError(PROVER_ERROR, "zkey_load_device: size out of range");
    zk->nVars = (uint32_t)n_vars;
    zk->nPublic = (uint32_t)n_public;
    zk->power = log_domain;
    zk->domain = 1u << log_domain;
    zk->nCoefs = n_coefs;
    zk->dA = DevMem::lent(d_A);   // the caller's sections: read, never freed
    zk->dB1 = DevMem::lent(d_B1);
    zk->dB2 = DevMem::lent(d_B2);
    zk->dC = DevMem::lent(d_C);
    zk->hdr = header_points_from_bytes(header_points);
    shard_init(zk.get(), rank, world, split, ZKPOA_SHARD_BLOCK_LOG(flags));
    zk->device = ctx->dev.device;
    if (split) {
      // the cyclic H shard is always the handle's own (zkpoa_zkey_set_shard_split replaces it): a copy of the
      // caller's, device to device
      const size_t bytes = (size_t)zk->h_scalar_count() * 64;
      zk->dHs.alloc(bytes);
      ZK_HIP(hipMemcpy(zk->dHs.get(), d_H, bytes, hipMemcpyDeviceToDevice));
    } else {
      zk->dH = DevMem::lent(d_H);
    }
    finish_load(ctx, zk.get(), d_coef_records, /*recs_on_host=*/false, split, LoadPhases{/*verbose=*/false});
    *out = zk.release();
  });
}

extern "C" int zkpoa_zkey_load_device(zkpoa_context* ctx, uint64_t n_vars, uint64_t n_public, unsigned log_domain,
                                      const void* d_A, const void* d_B1, const void* d_B2, const void* d_C,
                                      const void* d_H, const void* d_coef_records, uint64_t n_coefs,
                                      const uint8_t header_points[448], zkpoa_zkey** out) {
  return zkpoa_zkey_load_device_shard(ctx, n_vars, n_public, log_domain, 0, 1, 0, d_A, d_B1, d_B2, d_C, d_H, d_coef_records,
                                      n_coefs, header_points, out);
}

extern "C" int zkpoa_prove_device(zkpoa_context* ctx, const zkpoa_zkey* zkey, const void* d_witness,
                                  const uint8_t* r_le, const uint8_t* s_le, uint8_t proof_points[256],
                                  uint8_t* public_le, unsigned long public_capacity) {
  if (!ctx || !zkey || !d_witness || !proof_points) return PROVER_ERROR;
  return abi_call(ctx, [&] {
    if (public_le && public_capacity < (unsigned long)zkey->nPublic * 32)
      throw ProverError(PROVER_ERROR_SHORT_BUFFER, "public buffer too small");
    hipStream_t st = ctx->dev.lanes[0].stream;
    if (d_witness != zkey->d_witness)
      ZK_HIP(hipMemcpyAsync(zkey->d_witness, d_witness, (size_t)zkey->nVars * 32, hipMemcpyDeviceToDevice, st));
    if (public_le && zkey->nPublic)
      ZK_HIP(hipMemcpyAsync(public_le, reinterpret_cast<const char*>(d_witness) + 32, (size_t)zkey->nPublic * 32,
                            hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    prove_core(ctx, zkey, r_le, s_le, proof_points);
    if (!zkey->vkey_points.empty() && selfcheck_mode()) {
      std::vector<uint8_t> pub((size_t)zkey->nPublic * 32 + 1);
      if (zkey->nPublic)
        ZK_HIP(hipMemcpy(pub.data(), reinterpret_cast<const char*>(zkey->d_witness) + 32, (size_t)zkey->nPublic * 32,
                         hipMemcpyDeviceToHost));
      selfcheck(ctx, zkey, proof_points, pub.data());
    }
  });
}

extern "C" int zkpoa_zkey_precompute(zkpoa_context* ctx, zkpoa_zkey* zkey, uint64_t budget_bytes, uint64_t* used_bytes) {
  if (!ctx || !zkey) return PROVER_ERROR;
  return abi_call(ctx, [&] {
    uint64_t used = zkey_precompute(ctx, zkey, budget_bytes);
    if (used_bytes) *used_bytes = used;
  });
}

extern "C" int zkpoa_zkey_read_h_scalars(zkpoa_context* ctx, const zkpoa_zkey* zkey, void* out, unsigned long capacity) {
  if (!ctx || !zkey || !out) return PROVER_ERROR;
  return abi_call(ctx, [&] {
    const uint64_t cnt = zkey->h_scalar_count();
    if (capacity < cnt * 32) throw ProverError(PROVER_ERROR_SHORT_BUFFER, "h-scalar buffer too small");
    if (!zkey->d_abc) throw ProverError(PROVER_ERROR, "no H scalars on this handle");
    ZK_HIP(hipDeviceSynchronize());
    ZK_HIP(hipMemcpy(out, zkey->d_abc.get(), cnt * 32, hipMemcpyDeviceToHost));
  });
}

extern "C" int zkpoa_zkey_vkey(const zkpoa_zkey* zkey, uint8_t* buffer, unsigned long* size) {
  if (!zkey || !size) return PROVER_ERROR;
  const unsigned long needed = (unsigned long)zkey->vkey_points.size();
  if (needed == 0) return PROVER_ERROR;   // the handle carries no verification key
  if (!buffer || *size < needed) {
    *size = needed;
    return PROVER_ERROR_SHORT_BUFFER;
  }
  memcpy(buffer, zkey->vkey_points.data(), needed);
  *size = needed;
  return PROVER_OK;
}

extern "C" int zkpoa_proof_to_json(const uint8_t proof_points[256], int style, char* buffer, unsigned long* size) {
  if (!proof_points) return PROVER_ERROR;
  return emit(proof_json(proof_points, style), buffer, size);
}

extern "C" int zkpoa_public_to_json(const uint8_t* public_le, unsigned long n_public, int style, char* buffer,
                                    unsigned long* size) {
  if (!public_le && n_public) return PROVER_ERROR;
  return emit(public_json(public_le, n_public, style), buffer, size);
}

extern "C" int zkpoa_h_scalars(zkpoa_context* ctx, const void* coeffs, unsigned long coeffs_size, const void* witness,
                               uint64_t n_vars, unsigned log_domain, void* out) {
  if (!ctx || !coeffs || !witness || !out) return PROVER_ERROR;
  return abi_call(ctx, [&] {
    if (log_domain > 28) throw ProverError(PROVER_ERROR, "h_scalars: log_domain > 28");
    const uint8_t* cb = reinterpret_cast<const uint8_t*>(coeffs);
    if (coeffs_size < 4) throw ProverError(PROVER_ERROR, "h_scalars: coefficient payload too short");
    uint64_t ncoef = rd32(cb);
    if (coeffs_size != 4 + ncoef * 44) throw ProverError(PROVER_ERROR, "h_scalars: coefficient payload has the wrong size");
    const uint32_t domain = 1u << log_domain;
    hipStream_t st = ctx->dev.lanes[0].stream;
    LaneIn recs(cb + 4, 44, ncoef), wit(witness, 32, n_vars);
    DevBuf abc((size_t)3 * domain * 32);
    AbcCsr csr;
    abc_build_csr(st, recs.at<void>(0), ncoef, domain, (uint32_t)n_vars, 0u, 0u, csr);
    if (csr.err) throw ProverError(PROVER_ERROR, "h_scalars: coefficient record out of range or value >= r");
    ntt_prepare(ctx, st, log_domain);
    timed(ctx, st, kMsChain, [&] {
      h_chain(ctx, st, csr.row_ptr.as<uint32_t>(), csr.sig.as<uint32_t>(), csr.vals.get(), csr.long_list.as<uint32_t>(), csr.n_long,
              wit.at<void>(0), domain, log_domain, abc.p);
    });
    ZK_HIP(hipMemcpy(out, abc.p, (size_t)domain * 32, hipMemcpyDeviceToHost));
  });
}

// Test hook (not in the header): the automatic GPU choice of the multi-GPU drop-in for a node of `count` GPUs of which
// those in busy_mask are locked by other provers. out <- the chosen devices; returns how many.
extern "C" int zkpoa_test_auto_pick_devices(int count, unsigned power, unsigned min_power, unsigned long pid,
                                            unsigned busy_mask, int out[8]) {
  if (count <= 0 || count > 32 || !out) return -1;
  unsigned taken = 0;
  std::vector<int> order;
  std::vector<int> ids = auto_pick_devices(count, power, min_power, pid, [&](int d, bool block) {
    if (!block && ((busy_mask | taken) >> d) & 1u) return false;
    taken |= 1u << d;
    order.push_back(d);
    return true;
  }, [&](size_t keep) {
    while (order.size() > keep) {
      taken &= ~(1u << order.back());
      order.pop_back();
    }
  });
  for (size_t i = 0; i < ids.size() && i < 8; i++) out[i] = ids[i];
  return (int)ids.size();
}

// test hook (no GPU): the block size the multi-GPU loader deals sections 5-8 out with (multi_block_log_default)
extern "C" unsigned zkpoa_test_multi_block_log(uint64_t n_vars, unsigned ranks) {
  return multi_block_log_default(n_vars, ranks);
}

extern "C" int groth16_prover(const void* zkey_buffer, unsigned long zkey_size, const void* wtns_buffer,
                              unsigned long wtns_size, char* proof_buffer, unsigned long* proof_size,
                              char* public_buffer, unsigned long* public_size, char* error_msg,
                              unsigned long error_msg_maxsize) {
  const ProveOut out{proof_buffer, proof_size, public_buffer, public_size, error_msg, error_msg_maxsize};
  if (!zkey_buffer || !wtns_buffer || !proof_size || !public_size) return out.fail(PROVER_ERROR, "null argument");
  return one_shot(reinterpret_cast<const uint8_t*>(zkey_buffer), zkey_size,
                  WtnsSrc{reinterpret_cast<const uint8_t*>(wtns_buffer), wtns_size, -1}, out);
}

extern "C" int groth16_prover_zkey_file(const char* zkey_file_path, const void* wtns_buffer, unsigned long wtns_size,
                                        char* proof_buffer, unsigned long* proof_size, char* public_buffer,
                                        unsigned long* public_size, char* error_msg, unsigned long error_msg_maxsize) {
  const ProveOut out{proof_buffer, proof_size, public_buffer, public_size, error_msg, error_msg_maxsize};
  if (!zkey_file_path || !wtns_buffer || !proof_size || !public_size) return out.fail(PROVER_ERROR, "null argument");
  return zkey_file_prove(zkey_file_path, WtnsSrc{reinterpret_cast<const uint8_t*>(wtns_buffer), wtns_size, -1}, out);
}

extern "C" int zkpoa_groth16_prover_files(const char* zkey_file_path, const char* wtns_file_path, char* proof_buffer,
                                          unsigned long* proof_size, char* public_buffer, unsigned long* public_size,
                                          char* error_msg, unsigned long error_msg_maxsize) {
  const ProveOut out{proof_buffer, proof_size, public_buffer, public_size, error_msg, error_msg_maxsize};
  if (!zkey_file_path || !wtns_file_path || !proof_size || !public_size) return out.fail(PROVER_ERROR, "null argument");
  const Fd wtns(open(wtns_file_path, O_RDONLY | O_CLOEXEC));
  struct stat wsb;
  if (wtns.fd < 0 || fstat(wtns.fd, &wsb) != 0 || !S_ISREG(wsb.st_mode))
    return out.fail(PROVER_ERROR, std::string("cannot read witness file ") + wtns_file_path);
  return zkey_file_prove(zkey_file_path, WtnsSrc{nullptr, (uint64_t)wsb.st_size, wtns.fd}, out);
}

extern "C" int zkpoa_set_thread_options(const char* r_dec, const char* s_dec, const char* json_style, int verbose) {
  OptOverlay& o = opt_overlay();
  o.active = true;
  o.r = r_dec ? r_dec : "";
  o.s = s_dec ? s_dec : "";
  o.json = json_style ? json_style : "";
  o.verbose = verbose ? "1" : "";
  return PROVER_OK;
}

extern "C" int zkpoa_clear_thread_options(void) {
  opt_overlay() = OptOverlay();
  return PROVER_OK;
}

// The host has nothing to do right now: the library may use the time. One step of background work per call -- today: the
// next fixed-base table of the most recently used resident key that has none yet (ZKPOA_PRECOMP policy "idle") -- so that
// a request arriving meanwhile waits for one table at most. Returns 1 when a step was done (call again while idle), 0
// when there is nothing to do, the policy says no, or a request is in flight (never blocks behind one).
extern "C" int zkpoa_idle_work(void) { return idle_work(); }
