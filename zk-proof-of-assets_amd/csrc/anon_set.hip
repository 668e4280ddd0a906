// The verifier's side (include/zkpoa_audit.h): the stable index of the published set's addresses and the exact duplicate
// check over it (anon_set_sort.hip.h), and zkpoa_assets_verify, which binds set, root, commitment and proof together.
// Also what queries that index (include/zkpoa_merkle_paths.h): zkpoa_anon_set_find_device, and the find over a tree's
// stored leaves that poseidon.hip's zkpoa_merkle_find hands over to.
//
// Why a sort. The layer-two circuit proves inclusion of H(address, balance), and the reference's ascending-order check
// keeps the prover from using one owned address twice; nothing keeps the prover from publishing a set that holds its
// own address on two rows, one with an inflated balance. Such a set cannot match the chain, so an auditor rejects it --
// exactly, on a file the prover chose: a fingerprint or hash table the prover can collide will not do.
#include "anon_set_sort.hip.h"
#include "pedersen_host.hpp"
#include "zkpoa_internal.hpp"

#include <memory>

using namespace zkpoa;

namespace {

struct AuditCounts {
  uint64_t dups, first[2];
  int ascending;
};

// keys on the device -> d_perm and the counts; the kernels' time into ms[kMsAnonIndex]
AuditCounts audit_device(zkpoa_context* ctx, const void* d_keys, uint64_t n, uint32_t* d_perm, bool compare) {
  AuditCounts out{0, {~0ull, ~0ull}, 1};
  ctx->ms[kMsAnonIndex] = 0;
  if (n == 0) return out;
  hipStream_t st = ctx->dev.lanes[0].stream;
  AnonSetWork wk(n);
  DevBuf res(24);
  timed(ctx, st, kMsAnonIndex, [&] {
    anon_set_index(st, wk, d_keys, n, d_perm);
    if (compare) anon_set_adjacent(st, d_keys, d_perm, n, res.p);
  });
  if (compare) {
    uint64_t r[3];
    ZK_HIP(hipMemcpy(r, res.p, 24, hipMemcpyDeviceToHost));
    out.dups = r[0];
    if (r[0]) {
      out.first[0] = r[1] & 0xffffffffull;
      out.first[1] = r[1] >> 32;
    }
    out.ascending = r[0] == 0 && r[2] == 0;
  }
  return out;
}

// the find kernel over device buffers, waited for; its time into ms[kMsAnonFind] (added to what is there when `add`: a
// first find's index build comes before it)
void find_device(zkpoa_context* ctx, const void* d_keys, uint64_t n, const uint32_t* d_perm, const void* d_queries, uint64_t m,
                 uint32_t* d_first, uint32_t* d_count, bool add) {
  if (!add) ctx->ms[kMsAnonFind] = 0;
  if (m == 0) return;
  hipStream_t st = ctx->dev.lanes[0].stream;
  timed(ctx, st, kMsAnonFind, [&] { anon_set_find(st, d_keys, n, d_perm, d_queries, m, d_first, d_count); }, add);
}

const uint64_t kFrOrder[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};

// the row of the first of n x 32 B values that is not below r, or n
uint64_t first_not_in_field(const void* values, uint64_t n) {
  const uint8_t* p = static_cast<const uint8_t*>(values);
  for (uint64_t i = 0; i < n; i++)
    if (!U256::from_le(p + 32 * i).below(kFrOrder)) return i;
  return n;
}

// public.json: an array of decimal strings (or bare numbers)
std::vector<U256> public_signals(const char* text) {
  std::vector<U256> out;
  Json js{text, text + strlen(text)};
  js.array([&](uint64_t) {
    const Span s = js.scalar();
    U256 v;
    if (!v.parse_dec(s.b, s.e)) throw std::runtime_error("public.json: a signal is not a decimal integer below 2^256");
    out.push_back(v);
  });
  js.end();
  return out;
}

}  // namespace

extern "C" int zkpoa_anon_set_index_device(zkpoa_context* ctx, const void* d_addresses, uint64_t n, uint32_t* d_perm) {
  ZK_API_BEGIN(ctx)
  if (n >> 32) throw HipError("anon set: at most 2^32 - 1 rows");
  if (n && (!d_addresses || !d_perm)) throw HipError("anon set: null pointer");
  (void)audit_device(ctx, d_addresses, n, d_perm, false);
  ZK_API_END(ctx)
}

extern "C" int zkpoa_anon_set_find_device(zkpoa_context* ctx, const void* d_keys, uint64_t n, const uint32_t* d_perm,
                                          const void* d_queries, uint64_t m, uint32_t* d_first, uint32_t* d_count) {
  ZK_API_BEGIN(ctx)
  if (n >> 32 || m >> 32) throw HipError("anon set: at most 2^32 - 1 rows and queries");
  if (m && (!d_queries || !d_first || !d_count || (n && (!d_keys || !d_perm)))) throw HipError("anon set: null pointer");
  find_device(ctx, d_keys, n, d_perm, d_queries, m, d_first, d_count, false);
  ZK_API_END(ctx)
}

void zkpoa::anon_set_find_indexed(zkpoa_context* ctx, const void* d_keys, uint64_t n, DevMem& perm, const void* queries,
                                  uint64_t m, uint32_t* first, uint32_t* count) {
  ctx->ms[kMsAnonFind] = 0;
  if (n >> 32 || m >> 32) throw HipError("anon set: at most 2^32 - 1 rows and queries");
  if (!perm && n) {   // the first find over these keys: their index, kept by the caller
    hipStream_t st = ctx->dev.lanes[0].stream;
    DevMem fresh;
    fresh.alloc(n * 4);
    AnonSetWork wk(n);
    timed(ctx, st, kMsAnonFind, [&] { anon_set_index(st, wk, d_keys, n, fresh.as<uint32_t>()); });
    perm = std::move(fresh);
  }
  if (m == 0) return;
  LaneIn q(queries, 32, m);
  LaneOut f(first, 4, m), c(count, 4, m);
  find_device(ctx, d_keys, n, perm.as<uint32_t>(), q.at<const void>(0), m, f.at<uint32_t>(0), c.at<uint32_t>(0), true);
  f.down();
  c.down();
}

extern "C" int zkpoa_anon_set_audit(zkpoa_context* ctx, const void* addresses, uint64_t n, uint64_t out[4]) {
  ZK_API_BEGIN(ctx)
  if (!out || (n && !addresses)) throw HipError("anon set: null pointer");
  if (n >> 32) throw HipError("anon set: at most 2^32 - 1 rows");
  DevBuf keys(n * 32), perm(n * 4);
  ctx->uploader.upload(keys.p, addresses, n * 32, ctx->dev.device, ctx->dev.lanes[0].stream);
  const AuditCounts c = audit_device(ctx, keys.p, n, static_cast<uint32_t*>(perm.p), true);
  out[0] = c.dups;
  out[1] = c.first[0];
  out[2] = c.first[1];
  out[3] = (uint64_t)c.ascending;
  ZK_API_END(ctx)
}

extern "C" int zkpoa_assets_verify(zkpoa_context* ctx, const void* addresses, const void* balances, uint64_t n,
                                   const char* vkey_json, const char* public_json, const char* proof_json,
                                   const uint8_t* expected_commitment32, uint32_t* failed_checks,
                                   zkpoa_assets_report* report) {
  if (failed_checks) *failed_checks = 0;
  ZK_API_BEGIN(ctx)
  if (!vkey_json || !public_json || !proof_json || !failed_checks || (n && (!addresses || !balances)))
    throw HipError("assets verify: null argument");
  if (n >> 30 && n != (1ull << 30)) throw HipError("assets verify: at most 2^30 rows");
  uint32_t failed = 0;
  zkpoa_assets_report rep;
  memset(&rep, 0, sizeof(rep));
  rep.rows = n;
  rep.first_dup[0] = rep.first_dup[1] = ~0ull;
  rep.ascending = 1;

  // malformed input first: nothing below throws for what the files or the set hold
  auto t0 = std::chrono::steady_clock::now();
  double t_check = 0, t_proof = 0, t_upload = 0, t_index = 0, t_tree = 0;
  auto lap = [&](double& into) {
    into = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
  };
  const std::vector<U256> pub = public_signals(public_json);
  uint64_t bad = first_not_in_field(addresses, n);
  if (bad < n) throw HipError("assets verify: the address of row " + std::to_string(bad) + " is not below the BN254 scalar modulus");
  bad = first_not_in_field(balances, n);
  if (bad < n) throw HipError("assets verify: the balance of row " + std::to_string(bad) + " is not below the BN254 scalar modulus");
  lap(t_check);
  char err[512] = {0};
  const int proof_rc = zkpoa_groth16_verify(vkey_json, public_json, proof_json, err, sizeof(err));
  if (proof_rc != PROVER_OK && proof_rc != ZKPOA_VERIFY_INVALID_PROOF) throw HipError(std::string("assets verify: ") + err);
  if (proof_rc != PROVER_OK) failed |= ZKPOA_ASSETS_PROOF;
  lap(t_proof);

  // the set: duplicates and root, both from one upload
  if (n == 0) {
    failed |= ZKPOA_ASSETS_SET | ZKPOA_ASSETS_ROOT;
  } else {
    DevBuf da(n * 32), db(n * 32), perm(n * 4);
    hipStream_t st = ctx->dev.lanes[0].stream;
    ctx->uploader.upload(da.p, addresses, n * 32, ctx->dev.device, st);
    ctx->uploader.upload(db.p, balances, n * 32, ctx->dev.device, st);
    lap(t_upload);
    const AuditCounts c = audit_device(ctx, da.p, n, static_cast<uint32_t*>(perm.p), true);
    lap(t_index);
    rep.duplicate_rows = c.dups;
    rep.first_dup[0] = c.first[0];
    rep.first_dup[1] = c.first[1];
    rep.ascending = c.ascending;
    if (c.dups) failed |= ZKPOA_ASSETS_SET;
    zkpoa_merkle* tree = nullptr;
    if (zkpoa_merkle_build_device(ctx, da.p, db.p, n, &tree) != PROVER_OK) throw HipError(ctx->last_error);
    const int rc = zkpoa_merkle_root(ctx, tree, rep.root_le);
    zkpoa_merkle_free(ctx, tree);
    if (rc != PROVER_OK) throw HipError(ctx->last_error);
    uint8_t claimed[32];
    if (pub.size() == 13) pub[12].to_le(claimed);
    if (pub.size() != 13 || memcmp(claimed, rep.root_le, 32) != 0) failed |= ZKPOA_ASSETS_ROOT;
    lap(t_tree);
  }
  if (opt_verbose())
    fprintf(stderr, "zkpoa: assets verify: %llu rows: range check %.1f ms, proof %.1f ms, upload %.1f ms, index %.1f ms (kernels %.2f), "
                    "tree %.1f ms (kernels %.2f)\n", (unsigned long long)n, t_check, t_proof, t_upload, t_index,
            ctx->ms[kMsAnonIndex], t_tree, ctx->ms[kMsMerkleBuild]);

  // the commitment the proof binds
  bool point = false;
  if (pub.size() >= 12) point = pedersen_decode(pub.data(), rep.commitment);
  if (!point || (expected_commitment32 && memcmp(expected_commitment32, rep.commitment, 32) != 0)) failed |= ZKPOA_ASSETS_COMMITMENT;

  *failed_checks = failed;
  if (report) *report = rep;
  ZK_API_END(ctx)
}
