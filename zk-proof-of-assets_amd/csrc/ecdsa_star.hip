// ECDSA -> ECDSA* on the GPU: what scripts/ecdsa_sigs_parser.ts does per signature with ethers and noble-secp256k1
// (recover the public key, build r', derive the Ethereum address and compare it), one signature per lane, plus the two
// pieces of it that stand on their own: batched Keccak-256 and ethers.computeAddress. The arithmetic is
// csrc/secp256k1.hip.h and csrc/keccak.hip.h; this file is the kernels and the C ABI (include/zkpoa_prover.h).
#include "secp256k1.hip.h"
#include "zkpoa_internal.hpp"

using namespace zkpoa;
using namespace zkpoa::secp;

namespace {

constexpr uint32_t kSigThreads = 64;          // one wave per workgroup
constexpr uint64_t kSigLanesMax = 1u << 18;   // signatures per launch: bounds the lanes' tables at 256 MiB
constexpr uint64_t kTableBytesPerLane = 8 * 32 * 4;

// Every lane writes all of its outputs, with vector stores.
__global__ __launch_bounds__(kSigThreads) void ecdsa_star_kernel(const void* __restrict__ r, const void* __restrict__ s,
                                                                 const void* __restrict__ msghash, const uint8_t* __restrict__ v,
                                                                 const uint32_t* __restrict__ address, const AffineK* __restrict__ gtab,
                                                                 uint32_t* __restrict__ tables, uint64_t stride, uint64_t n,
                                                                 void* __restrict__ out_rprime, void* __restrict__ out_pubkey,
                                                                 uint32_t* __restrict__ out_address, uint8_t* __restrict__ out_status) {
  const uint64_t t = (uint64_t)blockIdx.x * kSigThreads + threadIdx.x;
  if (t >= n) return;   // whole tail of the last wave: stride >= the launch's lanes, so t < stride below
  uint32_t rl[8], sl[8], zl[8], given[5];
  load_be32(r, t, rl);
  load_be32(s, t, sl);
  load_be32(msghash, t, zl);
#pragma unroll
  for (int i = 0; i < 5; i++) given[i] = address[5 * t + i];
  const LaneTable lt{tables + t, stride};
  const Recovered res = recover_one(rl, sl, zl, v[t], given, gtab, lt);
  store_be32(out_rprime, t, res.r_prime.l);
  store_be32(out_pubkey, 2 * t, res.q.x.l);
  store_be32(out_pubkey, 2 * t + 1, res.q.y.l);
#pragma unroll
  for (int i = 0; i < 5; i++) out_address[5 * t + i] = res.addr[i];
  out_status[t] = (uint8_t)res.status;
}

__global__ __launch_bounds__(256) void keccak256_kernel(const uint8_t* __restrict__ messages, uint32_t len, uint64_t n,
                                                        uint64_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  uint64_t d[4];
  keccak::keccak256(messages + t * len, len, d);
#pragma unroll
  for (int i = 0; i < 4; i++) out[4 * t + i] = d[i];
}

__global__ __launch_bounds__(256) void eth_address_kernel(const void* __restrict__ pubkeys, uint64_t n, uint32_t* __restrict__ out_address,
                                                          uint8_t* __restrict__ out_text) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  AffineK q;
  load_be32(pubkeys, 2 * t, q.x.l);
  load_be32(pubkeys, 2 * t + 1, q.y.l);
  uint32_t addr[5];
  eth_address_words(q, addr);
#pragma unroll
  for (int i = 0; i < 5; i++) out_address[5 * t + i] = addr[i];
  uint8_t text[42];
  eip55_text(addr, text);
  // 42 t is even: two characters per store
  uint16_t* dst = reinterpret_cast<uint16_t*>(out_text + 42 * t);
#pragma unroll
  for (int i = 0; i < 21; i++) dst[i] = (uint16_t)(text[2 * i] | (text[2 * i + 1] << 8));
}

// 1G .. 8G in affine form, the same for every lane: computed here (seven additions) rather than spelt out
void generator_table(AffineK (&tab)[8]) {
  const AffineK g = generator();
  XyzzK e = XyzzK::from_affine(g);
  tab[0] = g;
  for (int m = 1; m < 8; m++) {
    xyzz_add_affine(e, g, false);
    tab[m] = to_affine(e);
  }
}

}  // namespace

extern "C" int zkpoa_ecdsa_star(zkpoa_context* ctx, uint64_t n, const void* r, const void* s, const void* msghash, const uint8_t* v,
                                const void* address20, void* out_rprime, void* out_pubkey_xy, void* out_address20,
                                uint8_t* out_status) {
  ZK_API_BEGIN(ctx)
  ctx->ms[8] = 0;
  if (n == 0) return PROVER_OK;
  if (n > (1ull << 32)) throw HipError("ecdsa_star: at most 2^32 signatures per call");
  if (!r || !s || !msghash || !v || !address20 || !out_rprime || !out_pubkey_xy || !out_address20 || !out_status)
    throw HipError("ecdsa_star: null argument");
  const uint64_t lanes = std::min<uint64_t>((n + kSigThreads - 1) / kSigThreads * kSigThreads, kSigLanesMax);
  AffineK gt[8];
  generator_table(gt);
  DevBuf dr(32 * n), ds(32 * n), dz(32 * n), dv(n), da(20 * n), dg(sizeof(gt)), dtab(lanes * kTableBytesPerLane);
  DevBuf orp(32 * n), opk(64 * n), oad(20 * n), ost(n);
  dr.up(r, 32 * n);
  ds.up(s, 32 * n);
  dz.up(msghash, 32 * n);
  dv.up(v, n);
  da.up(address20, 20 * n);
  dg.up(gt, sizeof(gt));
  hipStream_t st = ctx->dev.lanes[0].stream;
  ZK_HIP(hipEventRecord(ctx->ev_a[0], st));
  for (uint64_t i0 = 0; i0 < n; i0 += lanes) {
    const uint64_t m = std::min(lanes, n - i0);
    hipLaunchKernelGGL(ecdsa_star_kernel, dim3((uint32_t)((m + kSigThreads - 1) / kSigThreads)), dim3(kSigThreads), 0, st,
                       static_cast<const char*>(dr.p) + 32 * i0, static_cast<const char*>(ds.p) + 32 * i0,
                       static_cast<const char*>(dz.p) + 32 * i0, static_cast<const uint8_t*>(dv.p) + i0,
                       static_cast<const uint32_t*>(da.p) + 5 * i0, static_cast<const AffineK*>(dg.p),
                       static_cast<uint32_t*>(dtab.p), lanes, m, static_cast<char*>(orp.p) + 32 * i0,
                       static_cast<char*>(opk.p) + 64 * i0, static_cast<uint32_t*>(oad.p) + 5 * i0,
                       static_cast<uint8_t*>(ost.p) + i0);
  }
  ZK_HIP(hipEventRecord(ctx->ev_b[0], st));
  ZK_HIP(hipStreamSynchronize(st));
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipEventElapsedTime(&ctx->ms[8], ctx->ev_a[0], ctx->ev_b[0]));
  ZK_HIP(hipMemcpy(out_rprime, orp.p, 32 * n, hipMemcpyDeviceToHost));
  ZK_HIP(hipMemcpy(out_pubkey_xy, opk.p, 64 * n, hipMemcpyDeviceToHost));
  ZK_HIP(hipMemcpy(out_address20, oad.p, 20 * n, hipMemcpyDeviceToHost));
  ZK_HIP(hipMemcpy(out_status, ost.p, n, hipMemcpyDeviceToHost));
  ZK_API_END(ctx)
}

extern "C" int zkpoa_keccak256(zkpoa_context* ctx, const void* messages, uint64_t message_len, uint64_t n, void* out32) {
  ZK_API_BEGIN(ctx)
  if (message_len > 4096) throw HipError("keccak256: messages of at most 4096 bytes");
  if (n == 0) return PROVER_OK;
  if (n > (1ull << 32)) throw HipError("keccak256: at most 2^32 messages per call");
  if ((!messages && message_len) || !out32) throw HipError("keccak256: null argument");
  DevBuf dm(message_len * n), dout(32 * n);
  dm.up(messages, message_len * n);
  hipStream_t st = ctx->dev.lanes[0].stream;
  hipLaunchKernelGGL(keccak256_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, static_cast<const uint8_t*>(dm.p),
                     (uint32_t)message_len, n, static_cast<uint64_t*>(dout.p));
  ZK_HIP(hipStreamSynchronize(st));
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipMemcpy(out32, dout.p, 32 * n, hipMemcpyDeviceToHost));
  ZK_API_END(ctx)
}

extern "C" int zkpoa_eth_address(zkpoa_context* ctx, const void* pubkey_xy, uint64_t n, void* out_address20, void* out_checksum42) {
  ZK_API_BEGIN(ctx)
  if (n == 0) return PROVER_OK;
  if (n > (1ull << 32)) throw HipError("eth_address: at most 2^32 keys per call");
  if (!pubkey_xy || !out_address20 || !out_checksum42) throw HipError("eth_address: null argument");
  DevBuf dk(64 * n), da(20 * n), dt(42 * n);
  dk.up(pubkey_xy, 64 * n);
  hipStream_t st = ctx->dev.lanes[0].stream;
  hipLaunchKernelGGL(eth_address_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, dk.p, n, static_cast<uint32_t*>(da.p),
                     static_cast<uint8_t*>(dt.p));
  ZK_HIP(hipStreamSynchronize(st));
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipMemcpy(out_address20, da.p, 20 * n, hipMemcpyDeviceToHost));
  ZK_HIP(hipMemcpy(out_checksum42, dt.p, 42 * n, hipMemcpyDeviceToHost));
  ZK_API_END(ctx)
}
