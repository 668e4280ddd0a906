// zkpoa_secp_prim (include/zkpoa_secp_prim.h): the functions of csrc/secp256k1.hip.h one by one, one record per lane, on
// raw 8-word values -- the test hook that lets tests/test_gpu_secp_prim.py feed Fp, Sc, the recoding and the two ladders
// the operands at which their last corrections act. The arithmetic is the header's; this file only moves words.
#include "lane_batch.hip.h"
#include "secp256k1.hip.h"

using namespace zkpoa;
using namespace zkpoa::secp;

namespace {

constexpr uint32_t kPrimThreads = 64;          // one wave per workgroup, as the recovery kernel
constexpr uint64_t kPrimRecordsMax = 1u << 16;
constexpr uint64_t kTableWordsPerLane = 8 * 32;

// 8-word operand arrays in, 8-word result arrays out, then `tail` extra words per record
struct SecpArity {
  int in, out, tail;
};
SecpArity secp_prim_arity(int op) {
  static constexpr SecpArity k[] = {{2, 1, 0}, {1, 1, 0}, {2, 1, 0}, {2, 1, 0}, {1, 1, 0}, {1, 1, 0}, {1, 1, 0}, {1, 1, 0}, {1, 0, 1},
                                    {2, 1, 0}, {2, 1, 0}, {1, 1, 0}, {1, 1, 0}, {1, 1, 0}, {1, 1, 0}, {1, 0, 1}, {1, 0, 1},
                                    {1, 1, 2}, {4, 2, 0}, {1, 4, 0}, {4, 4, 1}};
  if (op < 0 || op >= (int)(sizeof(k) / sizeof(k[0]))) return {0, 0, 0};
  return k[op];
}

// Every lane below n reads operand j at in[(j n + i) 8 ..] and writes result j at out[(j n + i) 8 ..], the extra words at
// out[8 n out8 + i tail ..]: all inside the buffers zkpoa_secp_prim sized by the same arity. Vector stores only.
__global__ __launch_bounds__(kPrimThreads) void secp_prim_kernel(int op, const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                                 uint64_t n, uint32_t out8, uint32_t tail,
                                                                 const AffineK* __restrict__ gtab, const AffineK* __restrict__ ftab,
                                                                 uint32_t* __restrict__ tables, uint64_t stride) {
  const uint64_t i = (uint64_t)blockIdx.x * kPrimThreads + threadIdx.x;
  if (i >= n) return;   // i < n <= stride below
  auto fp = [&](int j) {
    secp::Fp r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.l[k] = in[((uint64_t)j * n + i) * 8 + k];
    return r;
  };
  auto sc = [&](int j) {
    secp::Sc r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.l[k] = in[((uint64_t)j * n + i) * 8 + k];
    return r;
  };
  auto put = [&](int j, const uint32_t (&l)[8]) {
#pragma unroll
    for (int k = 0; k < 8; k++) out[((uint64_t)j * n + i) * 8 + k] = l[k];
  };
  uint32_t* extra = out + (uint64_t)8 * n * out8 + i * tail;
  auto put_xyzz = [&](const XyzzK& p) {
    put(0, p.x.l);
    put(1, p.y.l);
    put(2, p.zz.l);
    put(3, p.zzz.l);
  };
  switch (op) {
    case 0: put(0, (fp(0) * fp(1)).l); break;
    case 1: put(0, fp(0).sqr().l); break;
    case 2: put(0, (fp(0) + fp(1)).l); break;
    case 3: put(0, (fp(0) - fp(1)).l); break;
    case 4: put(0, fp(0).neg().l); break;
    case 5: put(0, fp(0).dbl().l); break;
    case 6: put(0, fp(0).inv().l); break;
    case 7: put(0, fp(0).sqrt_candidate().l); break;
    case 8: extra[0] = fp(0).ge_p() ? 1u : 0u; break;
    case 9: put(0, (sc(0) * sc(1)).l); break;
    case 10: put(0, sc_add(sc(0), sc(1)).l); break;
    case 11: put(0, sc(0).neg().l); break;
    case 12: put(0, sc(0).inv().l); break;
    case 13: put(0, sc(0).reduce_once().l); break;
    case 14: put(0, key_from_hash(sc(0).l).l); break;
    case 15: extra[0] = sc(0).ge_n() ? 1u : 0u; break;
    case 16: extra[0] = sc(0).is_high() ? 1u : 0u; break;
    case 17: {
      uint32_t mag[8];
      uint64_t sgn;
      recode_signed4(sc(0).l, mag, sgn);
      put(0, mag);
      extra[0] = (uint32_t)sgn;
      extra[1] = (uint32_t)(sgn >> 32);
      break;
    }
    case 18: {
      const AffineK a = to_affine(XyzzK{fp(0), fp(1), fp(2), fp(3)});
      put(0, a.x.l);
      put(1, a.y.l);
      break;
    }
    case 19: put_xyzz(fixed_mul(sc(0), ftab)); break;
    default: {   // 20
      const LaneTable lt{tables + i, stride};
      const XyzzK q = double_mul(AffineK{fp(0), fp(1)}, sc(2), sc(3), gtab, lt);
      put_xyzz(q);
      extra[0] = q.is_inf() ? 1u : 0u;
      break;
    }
  }
}

}  // namespace

extern "C" int zkpoa_secp_prim(zkpoa_context* ctx, int op, const void* in, void* out, uint64_t n) {
  ZK_API_BEGIN(ctx)
  const SecpArity ar = secp_prim_arity(op);
  if (ar.in == 0) throw HipError("secp_prim: bad op");
  if (n > kPrimRecordsMax) throw HipError("secp_prim: at most 2^16 records per call");
  if (!batch_wanted("secp_prim", "records", n, in && out)) return PROVER_OK;
  const uint64_t lanes = (n + kPrimThreads - 1) / kPrimThreads * kPrimThreads;
  AffineK gt[8];
  generator_table(gt);
  LaneIn din(in, (size_t)32 * ar.in, n), dg(gt, sizeof(gt), 1), df(fixed_table_host(), sizeof(AffineK), kFixedEntries);
  LaneOut dout(out, (size_t)32 * ar.out + 4 * ar.tail, n);
  DevBuf dtab(op == 20 ? lanes * kTableWordsPerLane * 4 : 0);
  hipStream_t st = ctx->dev.lanes[0].stream;
  hipLaunchKernelGGL(secp_prim_kernel, dim3(blocks_of(n, kPrimThreads)), dim3(kPrimThreads), 0, st, op, din.at<const uint32_t>(0),
                     dout.at<uint32_t>(0), n, (uint32_t)ar.out, (uint32_t)ar.tail, dg.at<const AffineK>(0), df.at<const AffineK>(0),
                     static_cast<uint32_t*>(dtab.p), lanes);
  finish(st);
  dout.down();
  ZK_API_END(ctx)
}
