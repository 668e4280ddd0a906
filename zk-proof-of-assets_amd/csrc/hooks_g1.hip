// G1 / Fq / Fr instantiations of the element-wise hooks and the synthetic base generator.
#include "hooks.hip.h"

namespace zkpoa {
template <>
Affine<HFq> host_generator<HFq>() {
  return {HFq::from_u64(1), HFq::from_u64(2)};
}
void group_add_run_g1(zkpoa_context* ctx, const void* a, const void* b, void* out, uint64_t n) {
  group_add_run<Fq>(ctx, a, b, out, n);
}
void field_prim_run_g1(zkpoa_context* ctx, int field, int op, const void* in, void* out, uint64_t n, int raw) {
  if (field == 0) field_prim_run<Fq>(ctx, field, op, in, out, n, raw);
  else field_prim_run<Fr>(ctx, field, op, in, out, n, raw);
}
void curve_prim_run_g1(zkpoa_context* ctx, int op, const void* a, const void* b, const uint32_t* k, void* out,
                       uint64_t n) {
  curve_prim_run<Fq>(ctx, op, a, b, k, out, n);
}

// ---- zkpoa_fq29_prim: the 9 x 29-bit field (fq29.hip.h) and the G1 sums built on it ------------------------------
// words per element (in, out) of each op; ops 0-3 and 7 take 9-limb vectors as given when raw, 8-word values
// (re-limbed on load) otherwise, and always return 9 limbs as computed
struct Fq29Arity {
  int in_raw, in_words, out;
};
static Fq29Arity fq29_prim_arity(int op) {
  static constexpr Fq29Arity k[] = {{18, 16, 9}, {9, 8, 9}, {36, 32, 9}, {18, 16, 9}, {8, 8, 17}, {49, 49, 32}, {64, 64, 32}, {18, 16, 9}, {136, 136, 32},
                                    {0, 0, 0}, {64, 64, 36}, {136, 136, 36}, {32, 32, 32}};
  if (op < 0 || op >= (int)(sizeof(k) / sizeof(k[0]))) return {0, 0, 0};
  return k[op];
}
// acc += b in the 29-bit-limb form, all cases: infinity operands here, acc = +-b by redoing the exact addition
ZK_DEV void xyzz_add29(XYZZ<Fq>& acc, const XYZZ<Fq>& b) {
  if (b.is_inf()) return;
  if (acc.is_inf()) {
    acc = b;
    return;
  }
  Xyzz29S x, y;
  xyzz29s_from_wire(x, fq29_from_words(acc.x.l), fq29_from_words(acc.y.l), fq29_from_words(acc.zz.l), fq29_from_words(acc.zzz.l));
  xyzz29s_from_wire(y, fq29_from_words(b.x.l), fq29_from_words(b.y.l), fq29_from_words(b.zz.l), fq29_from_words(b.zzz.l));
  xyzz29s_add(x, y);
  Fq29 o[4];
  xyzz29s_to_wire(x, o[0], o[1], o[2], o[3]);
  uint32_t w[32];
#pragma unroll
  for (int c = 0; c < 4; c++) fq29_to_words(o[c], w + 8 * c);
  const XYZZ<Fq> r = xyzz_from_words_3q(w);
  if (r.zz.is_zero()) xyzz_add(acc, b);
  else acc = r;
}
static __global__ __launch_bounds__(256) void fq29_prim_kernel(int op, const uint32_t* in, uint32_t* out, uint64_t n,
                                                               int raw, uint32_t in_words, uint32_t out_words) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t* src = in + i * in_words;
  uint32_t* dst = out + i * out_words;
  auto arg = [&](int j) {
    Fq29 r;
    if (raw) {
#pragma unroll
      for (int k = 0; k < 9; k++) r.l[k] = src[9 * j + k];
    } else {
      uint32_t w[8];
#pragma unroll
      for (int k = 0; k < 8; k++) w[k] = src[8 * j + k];
      r = fq29_from_words(w);
    }
    return r;
  };
  auto put = [&](const Fq29& r) {
#pragma unroll
    for (int k = 0; k < 9; k++) dst[k] = r.l[k];
  };
  auto fq = [&](int off) {
    Fq r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.l[k] = src[off + k];
    return r;
  };
  switch (op) {
    case 0: put(fq29_mul(arg(0), arg(1))); break;
    case 1: put(fq29_sqr(arg(0))); break;
    case 2: put(fq29_dot2(arg(0), arg(1), arg(2), arg(3))); break;
    case 3: put(fq29_norm(fq29_sub<Fq29C4>(arg(0), arg(1)))); break;
    case 7: put(fq29_norm(fq29_sub<Fq29C14>(arg(0), arg(1)))); break;
    case 4: {   // 8 words -> 9 limbs -> 8 words
      uint32_t w[8];
#pragma unroll
      for (int k = 0; k < 8; k++) w[k] = src[k];
      const Fq29 r = fq29_from_words(w);
      put(r);
      fq29_to_words(r, w);
#pragma unroll
      for (int k = 0; k < 8; k++) dst[9 + k] = w[k];
      break;
    }
    case 5: {   // wire XYZZ + (negate ? -base : base) as the accumulation kernel adds: 32 + 16 + 1 words -> canonical XYZZ
      XYZZ<Fq> acc = {fq(0), fq(8), fq(16), fq(24)};
      const Affine<Fq> p = {fq(32), fq(40)};
      const bool neg = src[48] != 0;
      G1Piece29 s;
      s.a = {};
      s.empty = acc.is_inf();
      if (!s.empty)
        xyzz29_from_wire(s.a, fq29_from_words(acc.x.l), fq29_from_words(acc.y.l), fq29_from_words(acc.zz.l),
                         fq29_from_words(acc.zzz.l));
      g1piece29_add(s, p.x.l, p.y.l, neg);
      XYZZ<Fq> r;
      if (g1piece29_result(s, r)) acc = r;
      else xyzz_add_affine(acc, p, neg);
      store_xyzz(dst, 0, acc);
      break;
    }
    case 8: {   // a piece of 8 bases (16 words + negate flag each), summed as msm_accum0_kernel does -> canonical XYZZ
      G1Piece29 s;
      s.a = {};
      s.empty = true;
      for (int k = 0; k < 8; k++) {
        const Affine<Fq> p = {fq(17 * k), fq(17 * k + 8)};
        g1piece29_add(s, p.x.l, p.y.l, src[17 * k + 16] != 0);
      }
      XYZZ<Fq> acc;
      if (!g1piece29_result(s, acc)) {
        acc = XYZZ<Fq>::inf();
        for (int k = 0; k < 8; k++) xyzz_add_affine(acc, Affine<Fq>{fq(17 * k), fq(17 * k + 8)}, src[17 * k + 16] != 0);
      }
      store_xyzz(dst, 0, acc);
      break;
    }
    case 10: {   // packed + packed -> packed as the partial-sum kernels add; word 32 = 1 when the exact addition redid it
      const G1Sum29 a = g1sum29_load(src, 0), b = g1sum29_load(src, 1);
      G1Sum29 acc = a;
      RedPacked29::add(acc, b);
      const bool redo = RedPacked29::poisoned(acc);
      if (redo) {
        XYZZ<Fq> e = g1sum29_to_wire(a);
        xyzz_add(e, g1sum29_to_wire(b));
        RedExact29::store<false>(dst, 0, e);
      } else {
        RedPacked29::store<false>(dst, 0, acc);
      }
      dst[32] = redo ? 1u : 0u;
      dst[33] = dst[34] = dst[35] = 0;
      break;
    }
    case 11: {   // a piece of 8 bases as msm_accum0_kernel closes it -> packed; word 32 as above
      G1Piece29 s;
      s.a = {};
      s.empty = true;
      for (int k = 0; k < 8; k++) {
        const Affine<Fq> p = {fq(17 * k), fq(17 * k + 8)};
        g1piece29_add(s, p.x.l, p.y.l, src[17 * k + 16] != 0);
      }
      G1Sum29 sum = RedPacked29::inf();
      sum.inf = s.empty;
      const bool redo = !s.empty && !g1piece29_close(s, sum.p);
      if (redo) {
        XYZZ<Fq> acc = XYZZ<Fq>::inf();
        for (int k = 0; k < 8; k++) xyzz_add_affine(acc, Affine<Fq>{fq(17 * k), fq(17 * k + 8)}, src[17 * k + 16] != 0);
        sum = g1sum29_from_wire(acc);
      }
      g1sum29_store(dst, 0, sum);
      dst[32] = redo ? 1u : 0u;
      dst[33] = dst[34] = dst[35] = 0;
      break;
    }
    case 12:   // packed -> canonical wire XYZZ, as the last kernel of the reduction stores it
      RedPacked29::store<true>(dst, 0, g1sum29_load(src, 0));
      break;
    default: {   // 6: wire XYZZ + wire XYZZ -> canonical XYZZ
      XYZZ<Fq> acc = {fq(0), fq(8), fq(16), fq(24)};
      xyzz_add29(acc, XYZZ<Fq>{fq(32), fq(40), fq(48), fq(56)});
      store_xyzz(dst, 0, acc);
      break;
    }
  }
}
void fq29_prim_run(zkpoa_context* ctx, int op, const void* in, void* out, uint64_t n, int raw) {
  const Fq29Arity ar = fq29_prim_arity(op);
  if (ar.out == 0) throw HipError("fq29_prim: bad op");
  if (n == 0) return;
  const uint32_t in_words = raw ? ar.in_raw : ar.in_words;
  LaneIn din(in, (size_t)in_words * 4, n);
  LaneOut dout(out, (size_t)ar.out * 4, n);
  hipStream_t st = ctx->dev.lanes[0].stream;
  hipLaunchKernelGGL(fq29_prim_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, op, din.at<const uint32_t>(0),
                     dout.at<uint32_t>(0), n, raw ? 1 : 0, in_words, (uint32_t)ar.out);
  finish(st);
  dout.down();
}
void gen_bases_g1(zkpoa_context* ctx, const uint8_t a_le[32], const uint8_t b_le[32], uint64_t i0, uint64_t n, void* d_out) {
  gen_bases<Fq, HFq>(ctx, a_le, b_le, i0, n, d_out);
}
}  // namespace zkpoa
using namespace zkpoa;

extern "C" int zkpoa_field_op(zkpoa_context* ctx, int field, int op, const void* a, const void* b, void* out,
                              uint64_t n) {
  ZK_API_BEGIN(ctx)
  if (field < 0 || field > 1 || op < 0 || op > 5) throw HipError("field_op: bad field/op");
  if (n == 0) return PROVER_OK;
  LaneIn da(a, 32, n), db(b, 32, b ? n : 0);
  LaneOut dout(out, 32, n);
  hipStream_t st = ctx->dev.lanes[0].stream;
  dim3 grid(blocks_of(n, 256));
  const void *ap = da.at<const void>(0), *bp = b ? db.at<const void>(0) : nullptr;   // no b: the kernel takes zero for it
  if (field == 0) hipLaunchKernelGGL((zkpoa::field_op_kernel<Fq>), grid, dim3(256), 0, st, op, ap, bp, dout.at<void>(0), n);
  else hipLaunchKernelGGL((zkpoa::field_op_kernel<Fr>), grid, dim3(256), 0, st, op, ap, bp, dout.at<void>(0), n);
  finish(st);
  dout.down();
  ZK_API_END(ctx)
}

extern "C" int zkpoa_fq29_prim(zkpoa_context* ctx, int op, const void* in, void* out, uint64_t n, int raw) {
  ZK_API_BEGIN(ctx)
  fq29_prim_run(ctx, op, in, out, n, raw);
  ZK_API_END(ctx)
}
