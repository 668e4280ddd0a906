// The anonymity set against an Ethereum state root (include/zkpoa_state_proof.h): Merkle-Patricia proofs checked on the
// GPU. The arithmetic and the walk are csrc/mpt.hip.h; this file is the kernels, the layout check, the slab loop and the
// C ABI, and the whole check over a proofs file (csrc/state_proof_file.hpp) that `zkpoa-audit --state-proofs` runs.
#include "lane_batch.hip.h"
#include "mpt.hip.h"
#include "state_proof_file.hpp"

using namespace zkpoa;

namespace {

constexpr uint64_t kItemSlab = 1u << 20;   // items per walk launch (option state_proof_slab)
// the whole check: proofs and text bytes per slab of the file (a slab's blob is at most half its text, plus padding)
constexpr uint64_t kFileItems = 1u << 16;
constexpr uint64_t kFileText = 256ull << 20;

// one lane hashes one node: a longer one is refused with the layout (a branch node is 532 bytes)
constexpr uint32_t kMaxNodeBytes = 1u << 20;

struct Root {
  uint64_t w[4];
};

// One lane per node, nodes taken in `order` (bucketed by block count: a wave's lanes run the same number of
// permutations). The 24 rounds stay rolled (keccak.hip.h says why).
__global__ __launch_bounds__(256) void mpt_hash_kernel(const uint8_t* __restrict__ nodes, const uint64_t* __restrict__ node_offset,
                                                       const uint32_t* __restrict__ node_length, const uint32_t* __restrict__ order,
                                                       uint64_t count, uint64_t* __restrict__ digests) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= count) return;
  const uint32_t k = order[t];
  uint64_t d[4];
  mpt::keccak256_words(reinterpret_cast<const uint64_t*>(nodes + node_offset[k]), node_length[k], d);
#pragma unroll
  for (int i = 0; i < 4; i++) digests[4 * (uint64_t)k + i] = d[i];
}

// ZKPOA_MPT_ADDRESS20: the trie key of an address
__global__ __launch_bounds__(256) void mpt_address_key_kernel(const uint8_t* __restrict__ address20, uint64_t n, uint64_t* __restrict__ keys) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  uint64_t d[4];
  keccak::keccak256(address20 + 20 * t, 20, d);
#pragma unroll
  for (int i = 0; i < 4; i++) keys[4 * t + i] = d[i];
}

// One lane per item; every lane writes all of its outputs.
__global__ __launch_bounds__(256) void mpt_walk_kernel(const uint8_t* __restrict__ nodes, const uint64_t* __restrict__ node_offset,
                                                       const uint32_t* __restrict__ node_length, const uint64_t* __restrict__ first_node,
                                                       const uint64_t* __restrict__ digests, const uint8_t* __restrict__ keys32, Root root,
                                                       uint64_t n, uint8_t* __restrict__ out_status, uint32_t* __restrict__ out_where,
                                                       uint64_t* __restrict__ out_span) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  const mpt::Walked w = mpt::walk(nodes, node_offset, node_length, digests, first_node[t], first_node[t + 1], keys32 + 32 * t, root.w);
  out_status[t] = (uint8_t)w.status;
  out_where[t] = w.where;
  out_span[2 * t] = w.value_offset;
  out_span[2 * t + 1] = w.value_len;
}

// The account form: reads the walk's status and span, may turn a status 0 into ZKPOA_MPT_ACCOUNT. root / code: optional.
__global__ __launch_bounds__(256) void mpt_account_kernel(const uint8_t* __restrict__ nodes, const uint64_t* __restrict__ span, uint64_t n,
                                                          uint8_t* __restrict__ status, uint64_t* __restrict__ out_nonce,
                                                          uint8_t* __restrict__ out_balance, uint8_t* __restrict__ out_root,
                                                          uint8_t* __restrict__ out_code) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  mpt::Account acc;
  bool have = false;
  if (status[t] == mpt::kStatusPresent) {
    have = mpt::account(nodes + span[2 * t], (uint32_t)span[2 * t + 1], acc);
    if (!have) status[t] = (uint8_t)mpt::kStatusAccount;
  }
  out_nonce[t] = have ? acc.nonce : 0;
  for (int j = 0; j < 32; j++) {
    out_balance[32 * t + j] = have ? acc.balance[j] : 0;
    if (out_root) out_root[32 * t + j] = have ? acc.storage_root[j] : 0;
    if (out_code) out_code[32 * t + j] = have ? acc.code_hash[j] : 0;
  }
}

struct NodeArgs {
  const void* nodes;
  uint64_t nodes_bytes;
  const uint64_t* node_offset;
  const uint32_t* node_length;
  const uint64_t* first_node;
};

// The rules of include/zkpoa_state_proof.h, before anything is launched -> T
uint64_t checked_layout(const char* name, uint64_t n, const NodeArgs& a) {
  const std::string who = std::string(name) + ": ";
  if (n >> 32) throw HipError(who + "at most 2^32 - 1 items per call");
  if (!a.first_node) throw HipError(who + "null argument");
  if (a.first_node[0] != 0) throw HipError(who + "first_node[0] is not 0");
  for (uint64_t i = 0; i < n; i++)
    if (a.first_node[i + 1] < a.first_node[i]) throw HipError(who + "first_node descends at item " + std::to_string(i));
  const uint64_t T = a.first_node[n];
  if (T >> 32) throw HipError(who + "at most 2^32 - 1 nodes per call");
  if (T && (!a.node_offset || !a.node_length || (!a.nodes && a.nodes_bytes))) throw HipError(who + "null argument");
  for (uint64_t k = 0; k < T; k++) {
    if (a.node_offset[k] % 8) throw HipError(who + "the offset of node " + std::to_string(k) + " is not a multiple of 8");
    if (k && a.node_offset[k] < a.node_offset[k - 1]) throw HipError(who + "node_offset descends at node " + std::to_string(k));
    if (a.node_offset[k] > a.nodes_bytes || a.node_length[k] > a.nodes_bytes - a.node_offset[k])
      throw HipError(who + "node " + std::to_string(k) + " passes the end of the blob");
    if (a.node_length[k] > kMaxNodeBytes) throw HipError(who + "node " + std::to_string(k) + " is longer than 2^20 bytes");
  }
  return T;
}

struct AccountOut {
  uint64_t* nonce;
  void *balance, *storage_root, *code_hash;
};

// Both entry points, after the null checks. Layout checked, then: upload, per slab of items the hash of its nodes and
// the walk, the account kernel over all, down. The kernels' time -> ms[kMsLaneBatch].
void verify_run(const char* name, zkpoa_context* ctx, uint64_t n, const void* keys, int key_kind, const uint8_t* root32,
                const NodeArgs& a, uint8_t* out_status, uint32_t* out_where, uint64_t* out_span, const AccountOut* acct) {
  ctx->ms[kMsLaneBatch] = 0;
  const uint64_t T = checked_layout(name, n, a);
  if (n == 0) return;
  const uint64_t slab = ctx->opt_state_proof_slab ? (uint64_t)ctx->opt_state_proof_slab : kItemSlab;
  // node order, bucketed by block count within every slab's range of nodes (a counting sort)
  std::vector<uint32_t> order(T);
  for_slabs(n, slab, [&](uint64_t i0, uint64_t m) {
    const uint64_t lo = a.first_node[i0], hi = a.first_node[i0 + m];
    constexpr uint32_t kBuckets = 32;   // 1 .. 31 blocks each on their own, longer nodes together
    uint64_t at[kBuckets + 1] = {};
    auto bucket = [&](uint64_t k) { return std::min<uint32_t>(a.node_length[k] / keccak::kRate + 1, kBuckets); };
    for (uint64_t k = lo; k < hi; k++) at[bucket(k)]++;
    uint64_t sum = lo;
    for (uint32_t b = 0; b <= kBuckets; b++) {
      const uint64_t c = at[b];
      at[b] = sum;
      sum += c;
    }
    for (uint64_t k = lo; k < hi; k++) order[at[bucket(k)]++] = (uint32_t)k;
  });
  const uint64_t blob = (a.nodes_bytes + 7) & ~7ull;   // the hash kernel reads whole words
  DevBuf dnodes(blob);
  ZK_HIP(hipMemset(dnodes.p, 0, blob));
  dnodes.up(a.nodes, a.nodes_bytes);
  LaneIn doff(a.node_offset, 8, T), dlen(a.node_length, 4, T), dorder(order.data(), 4, T), dfirst(a.first_node, 8, n + 1);
  LaneIn dkeys(keys, key_kind == ZKPOA_MPT_ADDRESS20 ? 20 : 32, n);
  DevBuf ddig(32 * T), dhashed(key_kind == ZKPOA_MPT_ADDRESS20 ? 32 * n : 0);
  LaneOut ost(out_status, 1, n), owh(out_where, 4, n);
  DevBuf dspan(16 * n);
  Root root;
  memcpy(root.w, root32, 32);   // little-endian host: the 32 bytes in order, as the digests are stored
  hipStream_t st = ctx->dev.lanes[0].stream;
  const uint8_t* dn = static_cast<const uint8_t*>(dnodes.p);
  const bool roots = acct && acct->storage_root, codes = acct && acct->code_hash;
  LaneOut ono(acct ? acct->nonce : nullptr, 8, acct ? n : 0), oba(acct ? acct->balance : nullptr, 32, acct ? n : 0);
  LaneOut oro(roots ? acct->storage_root : nullptr, 32, roots ? n : 0), oco(codes ? acct->code_hash : nullptr, 32, codes ? n : 0);
  timed(ctx, st, kMsLaneBatch, [&] {
    const uint8_t* k32 = dkeys.at<const uint8_t>(0);
    if (key_kind == ZKPOA_MPT_ADDRESS20) {
      hipLaunchKernelGGL(mpt_address_key_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, dkeys.at<const uint8_t>(0), n,
                         static_cast<uint64_t*>(dhashed.p));
      k32 = static_cast<const uint8_t*>(dhashed.p);
    }
    for_slabs(n, slab, [&](uint64_t i0, uint64_t m) {
      const uint64_t lo = a.first_node[i0], hi = a.first_node[i0 + m];
      if (hi > lo)
        hipLaunchKernelGGL(mpt_hash_kernel, dim3(blocks_of(hi - lo, 256)), dim3(256), 0, st, dn, doff.at<const uint64_t>(0),
                           dlen.at<const uint32_t>(0), dorder.at<const uint32_t>(lo), hi - lo, static_cast<uint64_t*>(ddig.p));
      hipLaunchKernelGGL(mpt_walk_kernel, dim3(blocks_of(m, 256)), dim3(256), 0, st, dn, doff.at<const uint64_t>(0),
                         dlen.at<const uint32_t>(0), dfirst.at<const uint64_t>(i0), static_cast<const uint64_t*>(ddig.p), k32 + 32 * i0,
                         root, m, ost.at<uint8_t>(i0), owh.at<uint32_t>(i0), static_cast<uint64_t*>(dspan.p) + 2 * i0);
    });
    if (acct)
      hipLaunchKernelGGL(mpt_account_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, dn, static_cast<const uint64_t*>(dspan.p), n,
                         ost.at<uint8_t>(0), ono.at<uint64_t>(0), oba.at<uint8_t>(0), roots ? oro.at<uint8_t>(0) : nullptr,
                         codes ? oco.at<uint8_t>(0) : nullptr);
  });
  ost.down();
  owh.down();
  if (out_span) ZK_HIP(hipMemcpy(out_span, dspan.p, 16 * n, hipMemcpyDeviceToHost));
  if (acct) {
    ono.down();
    oba.down();
    if (roots) oro.down();
    if (codes) oco.down();
  }
}

// x / d for a 256-bit x (limbs least significant first)
U256 div_u64(const U256& x, uint64_t d) {
  U256 q;
  unsigned __int128 rem = 0;
  for (int k = 3; k >= 0; k--) {
    const unsigned __int128 cur = (rem << 64) | x.v[k];
    q.v[k] = (uint64_t)(cur / d);
    rem = cur % d;
  }
  return q;
}

}  // namespace

extern "C" int zkpoa_mpt_verify(zkpoa_context* ctx, uint64_t n, const void* keys, int key_kind, const uint8_t* root32,
                                const void* nodes, uint64_t nodes_bytes, const uint64_t* node_offset, const uint32_t* node_length,
                                const uint64_t* first_node, uint8_t* out_status, uint32_t* out_where, uint64_t* out_value_span) {
  ZK_API_BEGIN(ctx)
  if (key_kind != ZKPOA_MPT_KEY32 && key_kind != ZKPOA_MPT_ADDRESS20) throw HipError("mpt_verify: key_kind is 0 (32-byte keys) or 1 (addresses)");
  if (n && (!keys || !root32 || !out_status || !out_where || !out_value_span)) throw HipError("mpt_verify: null argument");
  verify_run("mpt_verify", ctx, n, keys, key_kind, root32, NodeArgs{nodes, nodes_bytes, node_offset, node_length, first_node},
             out_status, out_where, out_value_span, nullptr);
  ZK_API_END(ctx)
}

extern "C" int zkpoa_eth_account_proofs(zkpoa_context* ctx, uint64_t n, const void* address20, const uint8_t* root32,
                                        const void* nodes, uint64_t nodes_bytes, const uint64_t* node_offset,
                                        const uint32_t* node_length, const uint64_t* first_node, uint8_t* out_status,
                                        uint32_t* out_where, uint64_t* out_nonce, void* out_balance32, void* out_storage_root32,
                                        void* out_code_hash32) {
  ZK_API_BEGIN(ctx)
  if (n && (!address20 || !root32 || !out_status || !out_where || !out_nonce || !out_balance32))
    throw HipError("eth_account_proofs: null argument");
  const AccountOut acct{out_nonce, out_balance32, out_storage_root32, out_code_hash32};
  verify_run("eth_account_proofs", ctx, n, address20, ZKPOA_MPT_ADDRESS20, root32,
             NodeArgs{nodes, nodes_bytes, node_offset, node_length, first_node}, out_status, out_where, nullptr, &acct);
  ZK_API_END(ctx)
}

extern "C" int zkpoa_eth_block_header(const uint8_t* rlp, uint64_t len, uint8_t* hash32, uint8_t* state_root32, uint64_t* number) {
  if (!rlp || !hash32 || !state_root32 || !number || len == 0 || len >> 24) return PROVER_ERROR;   // a header is a few hundred bytes
  const mpt::Item top = mpt::rlp_item(rlp, 0, (uint32_t)len);
  if (!top.ok || !top.list || top.next != len) return PROVER_ERROR;
  static const uint32_t exact[7] = {32, 32, 20, 32, 32, 32, 256};
  uint32_t p = top.payload;
  uint64_t num = 0;
  const uint8_t* root = nullptr;
  for (uint32_t i = 0; i < 9; i++) {
    const mpt::Item it = mpt::rlp_item(rlp, p, top.next);
    if (!it.ok || it.list) return PROVER_ERROR;
    if (i < 7 ? it.len != exact[i] : it.len > (i == 7 ? 32u : 8u)) return PROVER_ERROR;
    if (i == 3) root = rlp + it.payload;
    if (i == 8)
      for (uint32_t j = 0; j < it.len; j++) num = (num << 8) | rlp[it.payload + j];
    p = it.next;
  }
  while (p < top.next) {   // what later forks appended: any items, but well-formed
    const mpt::Item it = mpt::rlp_item(rlp, p, top.next);
    if (!it.ok) return PROVER_ERROR;
    p = it.next;
  }
  // the byte-wise Keccak: the header lies wherever the caller has it
  uint64_t d[4];
  keccak::keccak256(rlp, (uint32_t)len, d);
  memcpy(hash32, d, 32);
  memcpy(state_root32, root, 32);
  *number = num;
  return PROVER_OK;
}

extern "C" int zkpoa_anon_set_state_check_file(zkpoa_context* ctx, const void* addresses, const void* balances, uint64_t n,
                                               const char* proofs_path, const uint8_t* root32, uint64_t unit_divisor,
                                               zkpoa_state_report* report) {
  ZK_API_BEGIN(ctx)
  if (!proofs_path || !root32 || !report || (n && (!addresses || !balances))) throw HipError("state check: null argument");
  if (n >> 32) throw HipError("state check: at most 2^32 - 1 rows");
  if (unit_divisor != 1 && unit_divisor != 1000000000ull && unit_divisor != 1000000000000000000ull)
    throw HipError("state check: unit_divisor is 1, 10^9 or 10^18");
  zkpoa_state_report rep;
  memset(&rep, 0, sizeof(rep));
  rep.rows = n;
  rep.first_bad_row = rep.first_diff_row = ~0ull;
  const auto t_begin = std::chrono::steady_clock::now();
  double t_read = 0, t_device = 0;

  // the set's addresses on the device; their index is built by the first lookup and kept for the others
  DevBuf keys(n * 32);
  ctx->uploader.upload(keys.p, addresses, n * 32, ctx->dev.device, ctx->dev.lanes[0].stream);
  DevMem perm;
  // per row: what its proofs gave so far
  enum : uint8_t { kNone = 0, kFailed = 1, kDiffers = 2, kPresent = 3, kAbsent = 4 };
  std::vector<uint8_t> state(n, kNone), fail_status(n, 0);
  std::vector<uint32_t> fail_where(n, 0);
  const uint8_t* bal = static_cast<const uint8_t*>(balances);

  ProofFile file(proofs_path);
  ProofSlab slab;
  std::vector<uint8_t> queries, status, balance;
  std::vector<uint32_t> first, count, where;
  std::vector<uint64_t> nonce;
  for (;;) {
    auto t0 = std::chrono::steady_clock::now();
    if (!file.next(slab, kFileItems, kFileText)) break;
    t_read += ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    const uint64_t m = slab.items;
    rep.proofs_read += m;
    queries.assign(32 * m, 0);
    for (uint64_t i = 0; i < m; i++)   // the address as the csv's integer, little-endian
      for (int j = 0; j < 20; j++) queries[32 * i + j] = slab.address20[20 * i + 19 - j];
    first.assign(m, 0xffffffffu);
    count.assign(m, 0);
    if (n) anon_set_find_indexed(ctx, keys.p, n, perm, queries.data(), m, first.data(), count.data());
    status.assign(m, 0);
    where.assign(m, 0);
    nonce.assign(m, 0);
    balance.assign(32 * m, 0);
    const AccountOut acct{nonce.data(), balance.data(), nullptr, nullptr};
    verify_run("state check", ctx, m, slab.address20.data(), ZKPOA_MPT_ADDRESS20, root32,
               NodeArgs{slab.nodes.data(), slab.nodes.size(), slab.node_offset.data(), slab.node_length.data(), slab.first_node.data()},
               status.data(), where.data(), nullptr, &acct);
    rep.kernel_ms += ctx->ms[kMsLaneBatch];
    t_device += ms_since(t0);
    for (uint64_t i = 0; i < m; i++) {
      if (!n || count[i] == 0) {
        rep.proofs_not_in_set++;
        continue;
      }
      const uint64_t row = first[i];
      if (state[row] >= kDiffers) continue;   // a valid proof has spoken: proofs under one root agree
      if (status[i] > mpt::kStatusAbsent) {
        if (state[row] == kNone) {
          state[row] = kFailed;
          fail_status[row] = status[i];
          fail_where[row] = where[i];
        }
        continue;
      }
      const U256 chain = U256::from_be(balance.data() + 32 * i), csv = U256::from_le(bal + 32 * row);
      const U256 units = div_u64(chain, unit_divisor);
      const bool absent = status[i] == mpt::kStatusAbsent;
      const bool equal = absent ? !(csv.v[0] | csv.v[1] | csv.v[2] | csv.v[3]) : memcmp(units.v, csv.v, 32) == 0;
      state[row] = equal ? (absent ? kAbsent : kPresent) : kDiffers;
      if (!equal && row < rep.first_diff_row) {
        rep.first_diff_row = row;
        rep.first_diff_absent = absent;
        memcpy(rep.first_diff_chain_balance32, balance.data() + 32 * i, 32);
      }
    }
  }
  for (uint64_t row = 0; row < n; row++) {
    const uint8_t s = state[row];
    if (s == kPresent) rep.proven_present++;
    else if (s == kAbsent) rep.proven_absent++;
    else {
      if (s == kNone) rep.rows_without_proof++;
      else if (s == kFailed) rep.rows_failed++;
      else rep.rows_differ++;
      if (rep.first_bad_row == ~0ull) {
        rep.first_bad_row = row;
        rep.first_bad_kind = s == kNone ? ZKPOA_STATE_BAD_NO_PROOF : s == kFailed ? ZKPOA_STATE_BAD_PROOFS : ZKPOA_STATE_BAD_BALANCE;
        rep.first_bad_status = s == kFailed ? fail_status[row] : 0;
        rep.first_bad_where = s == kFailed ? fail_where[row] : 0;
      }
    }
  }
  ctx->ms[kMsLaneBatch] = rep.kernel_ms;
  if (opt_verbose())
    fprintf(stderr, "zkpoa: state check: %llu rows, %llu proofs: read %.1f ms, lookup + upload + kernels %.1f ms (kernels %.2f), "
                    "all %.1f ms\n", (unsigned long long)n, (unsigned long long)rep.proofs_read, t_read, t_device, rep.kernel_ms,
            ms_since(t_begin));
  *report = rep;
  ZK_API_END(ctx)
}
