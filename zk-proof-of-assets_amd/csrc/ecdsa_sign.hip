// ECDSA signing on the GPU, one key per lane: what the reference's tests/generate_ecdsa_signatures.ts does per key with
// noble-secp256k1 (RFC 6979 nonce, signature, low s) and ethers (the address), plus the pieces that stand on their own:
// batched SHA-256, public keys, the nonce candidates, and the derived keys of `ecdsa-sigs-parser sign --generate-keys`.
// The arithmetic is csrc/secp256k1.hip.h and csrc/sha256.hip.h; this file is the kernels and the C ABI
// (include/zkpoa_ecdsa_sign.h). Not hardened against side channels: see the header.
#include "secp256k1.hip.h"
#include "zkpoa_internal.hpp"

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
  store_be32(out_pubkey, 2 * t, res.q.x.l);
  store_be32(out_pubkey, 2 * t + 1, res.q.y.l);
#pragma unroll
  for (int i = 0; i < 5; i++) out_address[5 * t + i] = res.addr[i];
  out_status[t] = (uint8_t)res.status;
}

__global__ __launch_bounds__(kSignThreads) void pubkey_kernel(const void* __restrict__ seckeys, const AffineK* __restrict__ ftab, uint64_t n,
                                                              void* __restrict__ out_pubkey, uint32_t* __restrict__ out_address,
                                                              uint8_t* __restrict__ out_status) {
  const uint64_t t = (uint64_t)blockIdx.x * kSignThreads + threadIdx.x;
  if (t >= n) return;
  uint32_t d[8];
  load_be32(seckeys, t, d);
  const PublicKey res = public_key(d, ftab);
  store_be32(out_pubkey, 2 * t, res.q.x.l);
  store_be32(out_pubkey, 2 * t + 1, res.q.y.l);
#pragma unroll
  for (int i = 0; i < 5; i++) out_address[5 * t + i] = res.addr[i];
  out_status[t] = (uint8_t)res.status;
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

// the table of fixed_mul: computed once per process on the host (512 additions), copied to the device by each call
const AffineK* fixed_table_host() {
  static AffineK tab[kFixedEntries];
  static std::once_flag once;
  std::call_once(once, [] { fixed_base_table(tab); });
  return tab;
}

// A call's device memory that held keys or nonces: overwritten on the stream before it is given back.
struct SecretBuf {
  DevBuf buf;
  size_t bytes;
  hipStream_t st;
  SecretBuf(size_t n, hipStream_t s) : buf(n), bytes(n), st(s) {}
  ~SecretBuf() {
    if (bytes) (void)hipMemsetAsync(buf.p, 0, bytes, st);
    (void)hipStreamSynchronize(st);
  }
};

uint32_t blocks_of(uint64_t lanes, uint32_t threads) { return (uint32_t)((lanes + threads - 1) / threads); }

void finish(hipStream_t st) {
  ZK_HIP(hipStreamSynchronize(st));
  ZK_HIP(hipGetLastError());
}

}  // namespace

extern "C" int zkpoa_sha256_batch(zkpoa_context* ctx, const void* messages, uint64_t message_len, uint64_t n, void* out32) {
  ZK_API_BEGIN(ctx)
  if (message_len > 4096) throw HipError("sha256: messages of at most 4096 bytes");
  if (n == 0) return PROVER_OK;
  if (n > (1ull << 32)) throw HipError("sha256: at most 2^32 messages per call");
  if ((!messages && message_len) || !out32) throw HipError("sha256: null argument");
  DevBuf dm(message_len * n), dout(32 * n);
  dm.up(messages, message_len * n);
  hipStream_t st = ctx->dev.lanes[0].stream;
  hipLaunchKernelGGL(sha256_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, static_cast<const uint8_t*>(dm.p), (uint32_t)message_len, n,
                     static_cast<uint32_t*>(dout.p));
  finish(st);
  ZK_HIP(hipMemcpy(out32, dout.p, 32 * n, hipMemcpyDeviceToHost));
  ZK_API_END(ctx)
}

extern "C" int zkpoa_secp256k1_derive_keys(zkpoa_context* ctx, const void* seed, uint64_t seed_len, uint64_t first, uint64_t n,
                                           void* out_seckeys) {
  ZK_API_BEGIN(ctx)
  if (seed_len > 4096) throw HipError("derive_keys: a seed of at most 4096 bytes");
  if (n == 0) return PROVER_OK;
  if (n > (1ull << 32)) throw HipError("derive_keys: at most 2^32 keys per call");
  if ((!seed && seed_len) || !out_seckeys) throw HipError("derive_keys: null argument");
  hipStream_t st = ctx->dev.lanes[0].stream;
  DevBuf ds(seed_len);
  ds.up(seed, seed_len);
  SecretBuf dk(32 * n, st);
  hipLaunchKernelGGL(derive_keys_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, static_cast<const uint8_t*>(ds.p), (uint32_t)seed_len,
                     first, n, dk.buf.p);
  finish(st);
  ZK_HIP(hipMemcpy(out_seckeys, dk.buf.p, 32 * n, hipMemcpyDeviceToHost));
  ZK_API_END(ctx)
}

extern "C" int zkpoa_secp256k1_pubkey(zkpoa_context* ctx, uint64_t n, const void* seckeys, void* out_pubkey_xy, void* out_address20,
                                      uint8_t* out_status) {
  ZK_API_BEGIN(ctx)
  if (n == 0) return PROVER_OK;
  if (n > (1ull << 32)) throw HipError("secp256k1_pubkey: at most 2^32 keys per call");
  if (!seckeys || !out_pubkey_xy || !out_address20 || !out_status) throw HipError("secp256k1_pubkey: null argument");
  hipStream_t st = ctx->dev.lanes[0].stream;
  DevBuf dtab(kFixedEntries * sizeof(AffineK)), opk(64 * n), oad(20 * n), ost(n);
  dtab.up(fixed_table_host(), kFixedEntries * sizeof(AffineK));
  SecretBuf dk(32 * n, st);
  dk.buf.up(seckeys, 32 * n);
  for (uint64_t i0 = 0; i0 < n; i0 += kSignLanesMax) {
    const uint64_t m = std::min(kSignLanesMax, n - i0);
    hipLaunchKernelGGL(pubkey_kernel, dim3(blocks_of(m, kSignThreads)), dim3(kSignThreads), 0, st,
                       static_cast<const char*>(dk.buf.p) + 32 * i0, static_cast<const AffineK*>(dtab.p), m,
                       static_cast<char*>(opk.p) + 64 * i0, static_cast<uint32_t*>(oad.p) + 5 * i0, static_cast<uint8_t*>(ost.p) + i0);
  }
  finish(st);
  ZK_HIP(hipMemcpy(out_pubkey_xy, opk.p, 64 * n, hipMemcpyDeviceToHost));
  ZK_HIP(hipMemcpy(out_address20, oad.p, 20 * n, hipMemcpyDeviceToHost));
  ZK_HIP(hipMemcpy(out_status, ost.p, n, hipMemcpyDeviceToHost));
  ZK_API_END(ctx)
}

extern "C" int zkpoa_rfc6979_nonce(zkpoa_context* ctx, uint64_t n, const void* seckeys, const void* msghash, uint32_t skip, void* out_k) {
  ZK_API_BEGIN(ctx)
  if (skip > 64) throw HipError("rfc6979_nonce: skip is at most 64");
  if (n == 0) return PROVER_OK;
  if (n > (1ull << 32)) throw HipError("rfc6979_nonce: at most 2^32 keys per call");
  if (!seckeys || !msghash || !out_k) throw HipError("rfc6979_nonce: null argument");
  hipStream_t st = ctx->dev.lanes[0].stream;
  DevBuf dz(32 * n);
  dz.up(msghash, 32 * n);
  SecretBuf dk(32 * n, st), ok(32 * n, st);
  dk.buf.up(seckeys, 32 * n);
  hipLaunchKernelGGL(rfc6979_nonce_kernel, dim3(blocks_of(n, kSignThreads)), dim3(kSignThreads), 0, st, dk.buf.p, dz.p, (int)skip, n,
                     ok.buf.p);
  finish(st);
  ZK_HIP(hipMemcpy(out_k, ok.buf.p, 32 * n, hipMemcpyDeviceToHost));
  ZK_API_END(ctx)
}

extern "C" int zkpoa_ecdsa_sign(zkpoa_context* ctx, uint64_t n, const void* seckeys, const void* msghash, uint64_t msghash_stride,
                                void* out_r, void* out_s, uint8_t* out_v, void* out_pubkey_xy, void* out_address20, uint8_t* out_status) {
  ZK_API_BEGIN(ctx)
  ctx->ms[8] = 0;
  if (msghash_stride != 0 && msghash_stride != 32) throw HipError("ecdsa_sign: msghash_stride is 0 (one hash) or 32 (one per key)");
  if (n == 0) return PROVER_OK;
  if (n > (1ull << 32)) throw HipError("ecdsa_sign: at most 2^32 keys per call");
  if (!seckeys || !msghash || !out_r || !out_s || !out_v || !out_pubkey_xy || !out_address20 || !out_status)
    throw HipError("ecdsa_sign: null argument");
  hipStream_t st = ctx->dev.lanes[0].stream;
  const uint64_t hashes = msghash_stride ? n : 1;
  const uint32_t hash_words = msghash_stride ? 8u : 0u;
  DevBuf dtab(kFixedEntries * sizeof(AffineK)), dz(32 * hashes);
  DevBuf orr(32 * n), os(32 * n), ov(n), opk(64 * n), oad(20 * n), ost(n);
  dtab.up(fixed_table_host(), kFixedEntries * sizeof(AffineK));
  dz.up(msghash, 32 * hashes);
  SecretBuf dk(32 * n, st);
  dk.buf.up(seckeys, 32 * n);
  ZK_HIP(hipEventRecord(ctx->ev_a[0], st));
  for (uint64_t i0 = 0; i0 < n; i0 += kSignLanesMax) {
    const uint64_t m = std::min(kSignLanesMax, n - i0);
    hipLaunchKernelGGL(ecdsa_sign_kernel, dim3(blocks_of(m, kSignThreads)), dim3(kSignThreads), 0, st,
                       static_cast<const char*>(dk.buf.p) + 32 * i0, static_cast<const uint32_t*>(dz.p) + hash_words * i0, hash_words,
                       static_cast<const AffineK*>(dtab.p), m, static_cast<char*>(orr.p) + 32 * i0, static_cast<char*>(os.p) + 32 * i0,
                       static_cast<uint8_t*>(ov.p) + i0, static_cast<char*>(opk.p) + 64 * i0, static_cast<uint32_t*>(oad.p) + 5 * i0,
                       static_cast<uint8_t*>(ost.p) + i0);
  }
  ZK_HIP(hipEventRecord(ctx->ev_b[0], st));
  finish(st);
  ZK_HIP(hipEventElapsedTime(&ctx->ms[8], ctx->ev_a[0], ctx->ev_b[0]));
  ZK_HIP(hipMemcpy(out_r, orr.p, 32 * n, hipMemcpyDeviceToHost));
  ZK_HIP(hipMemcpy(out_s, os.p, 32 * n, hipMemcpyDeviceToHost));
  ZK_HIP(hipMemcpy(out_v, ov.p, n, hipMemcpyDeviceToHost));
  ZK_HIP(hipMemcpy(out_pubkey_xy, opk.p, 64 * n, hipMemcpyDeviceToHost));
  ZK_HIP(hipMemcpy(out_address20, oad.p, 20 * n, hipMemcpyDeviceToHost));
  ZK_HIP(hipMemcpy(out_status, ost.p, n, hipMemcpyDeviceToHost));
  ZK_API_END(ctx)
}
