// ECDSA signing on the GPU, one key per lane: what the reference's tests/generate_ecdsa_signatures.ts does per key with
// noble-secp256k1 (RFC 6979 nonce, signature, low s) and ethers (the address), plus the pieces that stand on their own:
// batched SHA-256, public keys, the nonce candidates, and the derived keys of `ecdsa-sigs-parser sign --generate-keys`.
// The arithmetic is csrc/secp256k1.hip.h and csrc/sha256.hip.h; this file is the kernels and the C ABI
// (include/zkpoa_ecdsa_sign.h). Not hardened against side channels: see the header.
#include "lane_batch.hip.h"
#include "secp256k1.hip.h"

#include <mutex>

using namespace zkpoa;
using namespace zkpoa::secp;

namespace {

constexpr uint32_t kSignThreads = 64;          // one wave per workgroup, as the recovery kernel
constexpr uint64_t kSignLanesMax = 1u << 20;   // keys per launch

// Every lane writes all of its outputs, with vector stores. hash_words: 0 (one hash for all lanes) or 8.
__global__ __launch_bounds__(kSignThreads) void ecdsa_sign_kernel(const void* __restrict__ seckeys, const uint32_t* __restrict__ msghash,
                                                                  uint32_t hash_words, const AffineK* __restrict__ ftab, uint64_t n,
                                                                  void* __restrict__ out_r, void* __restrict__ out_s,
                                                                  uint8_t* __restrict__ out_v, void* __restrict__ out_pubkey,
                                                                  uint32_t* __restrict__ out_address, uint8_t* __restrict__ out_status) {
  const uint64_t t = (uint64_t)blockIdx.x * kSignThreads + threadIdx.x;
  if (t >= n) return;
  uint32_t d[8], z[8];
  load_be32(seckeys, t, d);
  load_be32(msghash + (uint64_t)hash_words * t, 0, z);
  const Signed res = sign_one(d, z, ftab);
  store_be32(out_r, t, res.r.l);
  store_be32(out_s, t, res.s.l);
  out_v[t] = (uint8_t)res.v;
  store_key_outputs(t, res.q, res.addr, res.status, out_pubkey, out_address, out_status);
}

__global__ __launch_bounds__(kSignThreads) void pubkey_kernel(const void* __restrict__ seckeys, const AffineK* __restrict__ ftab, uint64_t n,
                                                              void* __restrict__ out_pubkey, uint32_t* __restrict__ out_address,
                                                              uint8_t* __restrict__ out_status) {
  const uint64_t t = (uint64_t)blockIdx.x * kSignThreads + threadIdx.x;
  if (t >= n) return;
  uint32_t d[8];
  load_be32(seckeys, t, d);
  const PublicKey res = public_key(d, ftab);
  store_key_outputs(t, res.q, res.addr, res.status, out_pubkey, out_address, out_status);
}

__global__ __launch_bounds__(kSignThreads) void rfc6979_nonce_kernel(const void* __restrict__ seckeys, const void* __restrict__ msghash,
                                                                     int skip, uint64_t n, void* __restrict__ out_k) {
  const uint64_t t = (uint64_t)blockIdx.x * kSignThreads + threadIdx.x;
  if (t >= n) return;
  uint32_t d[8], z[8], k[8];
  load_be32(seckeys, t, d);
  load_be32(msghash, t, z);
  rfc6979_candidate(d, z, skip, k);
  store_be32(out_k, t, k);
}

// digest words are big-endian words: stored byte-swapped, the 32 bytes stand in order
__global__ __launch_bounds__(256) void sha256_kernel(const uint8_t* __restrict__ messages, uint32_t len, uint64_t n,
                                                     uint32_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  uint32_t h[8];
  sha256::digest(messages + t * len, len, h);
#pragma unroll
  for (int i = 0; i < 8; i++) out[8 * t + i] = bswap32(h[i]);
}

// key first + t = (SHA-256(seed || be64(first + t)) mod (n - 1)) + 1
__global__ __launch_bounds__(256) void derive_keys_kernel(const uint8_t* __restrict__ seed, uint32_t seed_len, uint64_t first, uint64_t n,
                                                          void* __restrict__ out_keys) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  store_be32(out_keys, t, derive_key(seed, seed_len, first + t).l);
}

}  // namespace

// the table of fixed_mul: computed once per process on the host (512 additions), copied to the device by each call
const AffineK* zkpoa::secp::fixed_table_host() {
  static AffineK tab[kFixedEntries];
  static std::once_flag once;
  std::call_once(once, [] { fixed_base_table(tab); });
  return tab;
}

extern "C" int zkpoa_sha256_batch(zkpoa_context* ctx, const void* messages, uint64_t message_len, uint64_t n, void* out32) {
  ZK_API_BEGIN(ctx)
  if (message_len > 4096) throw HipError("sha256: messages of at most 4096 bytes");
  if (!batch_wanted("sha256", "messages", n, (messages || !message_len) && out32)) return PROVER_OK;
  LaneIn dm(messages, message_len, n);
  LaneOut dout(out32, 32, n);
  hipStream_t st = ctx->dev.lanes[0].stream;
  hipLaunchKernelGGL(sha256_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, dm.at<const uint8_t>(0), (uint32_t)message_len, n,
                     dout.at<uint32_t>(0));
  finish(st);
  dout.down();
  ZK_API_END(ctx)
}

extern "C" int zkpoa_secp256k1_derive_keys(zkpoa_context* ctx, const void* seed, uint64_t seed_len, uint64_t first, uint64_t n,
                                           void* out_seckeys) {
  ZK_API_BEGIN(ctx)
  if (seed_len > 4096) throw HipError("derive_keys: a seed of at most 4096 bytes");
  if (!batch_wanted("derive_keys", "keys", n, (seed || !seed_len) && out_seckeys)) return PROVER_OK;
  hipStream_t st = ctx->dev.lanes[0].stream;
  LaneIn ds(seed, seed_len, 1);
  LaneOut<SecretBuf> dk(out_seckeys, 32, n, st);
  hipLaunchKernelGGL(derive_keys_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, ds.at<const uint8_t>(0), (uint32_t)seed_len, first, n,
                     dk.at<void>(0));
  finish(st);
  dk.down();
  ZK_API_END(ctx)
}

extern "C" int zkpoa_secp256k1_pubkey(zkpoa_context* ctx, uint64_t n, const void* seckeys, void* out_pubkey_xy, void* out_address20,
                                      uint8_t* out_status) {
  ZK_API_BEGIN(ctx)
  if (!batch_wanted("secp256k1_pubkey", "keys", n, seckeys && out_pubkey_xy && out_address20 && out_status)) return PROVER_OK;
  hipStream_t st = ctx->dev.lanes[0].stream;
  LaneIn dtab(fixed_table_host(), sizeof(AffineK), kFixedEntries);
  LaneOut opk(out_pubkey_xy, 64, n), oad(out_address20, 20, n), ost(out_status, 1, n);
  LaneIn<SecretBuf> dk(seckeys, 32, n, st);
  for_slabs(n, kSignLanesMax, [&](uint64_t i0, uint64_t m) {
    hipLaunchKernelGGL(pubkey_kernel, dim3(blocks_of(m, kSignThreads)), dim3(kSignThreads), 0, st, dk.at<const void>(i0),
                       dtab.at<const AffineK>(0), m, opk.at<void>(i0), oad.at<uint32_t>(i0), ost.at<uint8_t>(i0));
  });
  finish(st);
  for (const auto* o : {&opk, &oad, &ost}) o->down();
  ZK_API_END(ctx)
}

extern "C" int zkpoa_rfc6979_nonce(zkpoa_context* ctx, uint64_t n, const void* seckeys, const void* msghash, uint32_t skip, void* out_k) {
  ZK_API_BEGIN(ctx)
  if (skip > 64) throw HipError("rfc6979_nonce: skip is at most 64");
  if (!batch_wanted("rfc6979_nonce", "keys", n, seckeys && msghash && out_k)) return PROVER_OK;
  hipStream_t st = ctx->dev.lanes[0].stream;
  LaneIn dz(msghash, 32, n);
  LaneIn<SecretBuf> dk(seckeys, 32, n, st);
  LaneOut<SecretBuf> ok(out_k, 32, n, st);
  hipLaunchKernelGGL(rfc6979_nonce_kernel, dim3(blocks_of(n, kSignThreads)), dim3(kSignThreads), 0, st, dk.at<const void>(0),
                     dz.at<const void>(0), (int)skip, n, ok.at<void>(0));
  finish(st);
  ok.down();
  ZK_API_END(ctx)
}

extern "C" int zkpoa_ecdsa_sign(zkpoa_context* ctx, uint64_t n, const void* seckeys, const void* msghash, uint64_t msghash_stride,
                                void* out_r, void* out_s, uint8_t* out_v, void* out_pubkey_xy, void* out_address20, uint8_t* out_status) {
  ZK_API_BEGIN(ctx)
  ctx->ms[kMsLaneBatch] = 0;
  if (msghash_stride != 0 && msghash_stride != 32) throw HipError("ecdsa_sign: msghash_stride is 0 (one hash) or 32 (one per key)");
  if (!batch_wanted("ecdsa_sign", "keys", n, seckeys && msghash && out_r && out_s && out_v && out_pubkey_xy && out_address20 && out_status))
    return PROVER_OK;
  hipStream_t st = ctx->dev.lanes[0].stream;
  LaneIn dtab(fixed_table_host(), sizeof(AffineK), kFixedEntries), dz(msghash, 32, msghash_stride ? n : 1);
  LaneOut orr(out_r, 32, n), os(out_s, 32, n), ov(out_v, 1, n), opk(out_pubkey_xy, 64, n), oad(out_address20, 20, n), ost(out_status, 1, n);
  LaneIn<SecretBuf> dk(seckeys, 32, n, st);
  timed(ctx, st, kMsLaneBatch, [&] {
    for_slabs(n, kSignLanesMax, [&](uint64_t i0, uint64_t m) {
      hipLaunchKernelGGL(ecdsa_sign_kernel, dim3(blocks_of(m, kSignThreads)), dim3(kSignThreads), 0, st, dk.at<const void>(i0),
                         dz.at<const uint32_t>(msghash_stride ? i0 : 0), msghash_stride ? 8u : 0u, dtab.at<const AffineK>(0), m,
                         orr.at<void>(i0), os.at<void>(i0), ov.at<uint8_t>(i0), opk.at<void>(i0), oad.at<uint32_t>(i0), ost.at<uint8_t>(i0));
    });
  });
  for (const auto* o : {&orr, &os, &ov, &opk, &oad, &ost}) o->down();
  ZK_API_END(ctx)
}
