// ECDSA -> ECDSA* on the GPU: what scripts/ecdsa_sigs_parser.ts does per signature with ethers and noble-secp256k1
// (recover the public key, build r', derive the Ethereum address and compare it), one signature per lane, plus the two
// pieces of it that stand on their own: batched Keccak-256 and ethers.computeAddress. The arithmetic is
// csrc/secp256k1.hip.h and csrc/keccak.hip.h; this file is the kernels and the C ABI (include/zkpoa_prover.h).
#include "lane_batch.hip.h"
#include "secp256k1.hip.h"

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
  store_key_outputs(t, res.q, res.addr, res.status, out_pubkey, out_address, out_status);
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

}  // namespace

extern "C" int zkpoa_ecdsa_star(zkpoa_context* ctx, uint64_t n, const void* r, const void* s, const void* msghash, const uint8_t* v,
                                const void* address20, void* out_rprime, void* out_pubkey_xy, void* out_address20,
                                uint8_t* out_status) {
  ZK_API_BEGIN(ctx)
  ctx->ms[kMsLaneBatch] = 0;
  if (!batch_wanted("ecdsa_star", "signatures", n,
                    r && s && msghash && v && address20 && out_rprime && out_pubkey_xy && out_address20 && out_status))
    return PROVER_OK;
  const uint64_t lanes = std::min<uint64_t>((n + kSigThreads - 1) / kSigThreads * kSigThreads, kSigLanesMax);
  AffineK gt[8];
  generator_table(gt);
  LaneIn dr(r, 32, n), ds(s, 32, n), dz(msghash, 32, n), dv(v, 1, n), da(address20, 20, n), dg(gt, sizeof(gt), 1);
  DevBuf dtab(lanes * kTableBytesPerLane);
  LaneOut orp(out_rprime, 32, n), opk(out_pubkey_xy, 64, n), oad(out_address20, 20, n), ost(out_status, 1, n);
  hipStream_t st = ctx->dev.lanes[0].stream;
  timed(ctx, st, kMsLaneBatch, [&] {
    for_slabs(n, lanes, [&](uint64_t i0, uint64_t m) {
      hipLaunchKernelGGL(ecdsa_star_kernel, dim3(blocks_of(m, kSigThreads)), dim3(kSigThreads), 0, st, dr.at<const void>(i0),
                         ds.at<const void>(i0), dz.at<const void>(i0), dv.at<const uint8_t>(i0), da.at<const uint32_t>(i0),
                         dg.at<const AffineK>(0), static_cast<uint32_t*>(dtab.p), lanes, m, orp.at<void>(i0), opk.at<void>(i0),
                         oad.at<uint32_t>(i0), ost.at<uint8_t>(i0));
    });
  });
  for (const auto* o : {&orp, &opk, &oad, &ost}) o->down();
  ZK_API_END(ctx)
}

extern "C" int zkpoa_keccak256(zkpoa_context* ctx, const void* messages, uint64_t message_len, uint64_t n, void* out32) {
  ZK_API_BEGIN(ctx)
  if (message_len > 4096) throw HipError("keccak256: messages of at most 4096 bytes");
  if (!batch_wanted("keccak256", "messages", n, (messages || !message_len) && out32)) return PROVER_OK;
  LaneIn dm(messages, message_len, n);
  LaneOut dout(out32, 32, n);
  hipStream_t st = ctx->dev.lanes[0].stream;
  hipLaunchKernelGGL(keccak256_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, dm.at<const uint8_t>(0), (uint32_t)message_len, n,
                     dout.at<uint64_t>(0));
  finish(st);
  dout.down();
  ZK_API_END(ctx)
}

extern "C" int zkpoa_eth_address(zkpoa_context* ctx, const void* pubkey_xy, uint64_t n, void* out_address20, void* out_checksum42) {
  ZK_API_BEGIN(ctx)
  if (!batch_wanted("eth_address", "keys", n, pubkey_xy && out_address20 && out_checksum42)) return PROVER_OK;
  LaneIn dk(pubkey_xy, 64, n);
  LaneOut da(out_address20, 20, n), dt(out_checksum42, 42, n);
  hipStream_t st = ctx->dev.lanes[0].stream;
  hipLaunchKernelGGL(eth_address_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, dk.at<const void>(0), n, da.at<uint32_t>(0),
                     dt.at<uint8_t>(0));
  finish(st);
  da.down();
  dt.down();
  ZK_API_END(ctx)
}
