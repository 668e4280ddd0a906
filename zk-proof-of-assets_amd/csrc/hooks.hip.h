// Element-wise device hooks (parity tests) and synthetic base generation, generic over the group.
#pragma once
#include "msm.hip.h"
#include "zkpoa_internal.hpp"

namespace zkpoa {

// ---------------------------------------------------------------------------------------------
// element-wise test kernels
// ---------------------------------------------------------------------------------------------
template <class F>
__global__ __launch_bounds__(256) void field_op_kernel(int op, const void* a, const void* b, void* out, uint64_t n) {
  uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  F x = load_field<F>(reinterpret_cast<const char*>(a) + 32 * i);
  F y = F::zero();
  if (b) y = load_field<F>(reinterpret_cast<const char*>(b) + 32 * i);
  F r;
  switch (op) {
    case 0: r = x * y; break;
    case 1: r = x + y; break;
    case 2: r = x - y; break;
    case 3: r = x.inv(); break;
    case 4: r = x.to_mont(); break;
    default: r = x.from_mont(); break;
  }
  store_field(reinterpret_cast<char*>(out) + 32 * i, r);
}

template <class F>
__global__ __launch_bounds__(256) void group_add_kernel(const void* a, const void* b, void* out_xyzz, uint64_t n) {
  uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  Affine<F> pa = load_affine<F>(a, i), pb = load_affine<F>(b, i);
  XYZZ<F> acc = XYZZ<F>::from_affine(pa);
  xyzz_add_affine(acc, pb, false);
  store_xyzz(out_xyzz, i, acc);
}

// XYZZ -> affine on the device (one Fermat inversion per point; setup/test use only)
template <class F>
__global__ __launch_bounds__(256) void xyzz_to_affine_kernel(const void* in_xyzz, void* out_affine, uint64_t n) {
  uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  XYZZ<F> p = load_xyzz<F>(in_xyzz, i);
  constexpr int FB = FieldBytes<F>::N;
  char* o = reinterpret_cast<char*>(out_affine) + i * (2 * FB);
  if (p.is_inf()) {
    store_field(o, F::zero());
    store_field(o + FB, F::zero());
    return;
  }
  F i3 = p.zzz.inv();
  F i2 = (p.zz * i3).sqr();
  store_field(o, p.x * i2);
  store_field(o + FB, p.y * i3);
}

// P_i = (a + i*b) * G for i in [i0 + t*CH, +CH): one double-and-add per thread, then CH-1 mixed
// additions of B = b*G. Output XYZZ into scratch (converted by xyzz_to_affine_kernel).
template <class F>
__global__ __launch_bounds__(256) void gen_bases_kernel(Affine<F> G, Affine<F> Bstep, Fr a_m, Fr b_m, uint64_t i0,
                                                        uint64_t n, uint32_t CH, void* out_xyzz) {
  uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  uint64_t first = t * CH;
  if (first >= n) return;
  // s = a + (i0 + first) * b  (Montgomery), then to standard form for the bit scan
  uint64_t idx = i0 + first;
  Fr im = Fr::zero();
  im.l[0] = (uint32_t)idx;
  im.l[1] = (uint32_t)(idx >> 32);
  im = im.to_mont();
  Fr s = (a_m + b_m * im).from_mont().canon();  // canonical: the bits are scanned below
  XYZZ<F> acc = XYZZ<F>::inf();
  for (int limb = 7; limb >= 0; limb--) {
    uint32_t w = s.l[limb];
    for (int bit = 31; bit >= 0; bit--) {
      acc = xyzz_dbl(acc);
      if ((w >> bit) & 1u) xyzz_add_affine(acc, G, false);
    }
  }
  uint64_t last = first + CH < n ? first + CH : n;
  for (uint64_t k = first; k < last; k++) {
    store_xyzz(out_xyzz, k, acc);
    xyzz_add_affine(acc, Bstep, false);
  }
}


// group generator (affine, Montgomery); specialised in hooks_g1.hip / hooks_g2.hip
template <class HF>
Affine<HF> host_generator();

template <class F, class HF>
void gen_bases(zkpoa_context* ctx, const uint8_t a_le[32], const uint8_t b_le[32], uint64_t i0, uint64_t n,
               void* d_out) {
  if (n == 0) return;
  Lane& lane = ctx->dev.lanes[0];
  Affine<HF> G = host_generator<HF>();
  uint64_t bk[4];
  memcpy(bk, b_le, 32);
  Affine<HF> Bs = h_to_affine(h_mul(XYZZ<HF>::from_affine(G), bk));
  Affine<F> dG, dB;
  static_assert(sizeof(Affine<F>) == sizeof(Affine<HF>), "layout");
  memcpy(&dG, &G, sizeof(dG));
  memcpy(&dB, &Bs, sizeof(dB));
  Fr am, bm;
  HFr ha = HFr::from_bytes(a_le).to_mont(), hb = HFr::from_bytes(b_le).to_mont();
  memcpy(&am, &ha, 32);
  memcpy(&bm, &hb, 32);
  const uint32_t CH = 32;
  // scratch: XYZZ for every point, processed in slabs to bound memory
  const uint64_t slab = 1ull << 22;
  DevBuf scratch((n < slab ? n : slab) * MsmSizes<F>::kXyzz);
  for (uint64_t off = 0; off < n; off += slab) {
    uint64_t cnt = n - off < slab ? n - off : slab;
    uint64_t threads = (cnt + CH - 1) / CH;
    hipLaunchKernelGGL((gen_bases_kernel<F>), dim3(blocks_of(threads, 256)), dim3(256), 0, lane.stream, dG,
                       dB, am, bm, i0 + off, cnt, CH, scratch.p);
    hipLaunchKernelGGL((xyzz_to_affine_kernel<F>), dim3(blocks_of(cnt, 256)), dim3(256), 0, lane.stream,
                       (const void*)scratch.p, (void*)(reinterpret_cast<char*>(d_out) + off * MsmSizes<F>::kAffine),
                       cnt);
  }
  finish(lane.stream);
}


template <class F>
inline void group_add_run(zkpoa_context* ctx, const void* a, const void* b, void* out, uint64_t n) {
  constexpr size_t A = MsmSizes<F>::kAffine;
  LaneIn da(a, A, n), db(b, A, n);
  DevBuf dx(n * MsmSizes<F>::kXyzz);
  LaneOut dout(out, A, n);
  hipStream_t st = ctx->dev.lanes[0].stream;
  dim3 grid(blocks_of(n, 256));
  hipLaunchKernelGGL((group_add_kernel<F>), grid, dim3(256), 0, st, da.template at<const void>(0),
                     db.template at<const void>(0), dx.p, n);
  hipLaunchKernelGGL((xyzz_to_affine_kernel<F>), grid, dim3(256), 0, st, (const void*)dx.p, dout.template at<void>(0), n);
  finish(st);
  dout.down();
}

// ---------------------------------------------------------------------------------------------
// primitive-level test kernels (zkpoa_field_prim / zkpoa_curve_prim): the field and curve layer's own functions on
// raw lazy values, results stored as computed (or canonical) so the tests can assert each function's output range
// ---------------------------------------------------------------------------------------------
// operand / result counts per op (include/zkpoa_prover.h); {0, 0} = no such op
struct PrimArity {
  int in, out;
};
inline PrimArity field_prim_arity(int field, int op) {
  static constexpr PrimArity kFp[] = {{2, 1}, {1, 1}, {2, 1}, {2, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1},
                                      {1, 1}, {4, 1}, {6, 1}, {4, 2}, {2, 2}, {8, 2}, {1, 1}, {2, 1}};
  static constexpr PrimArity kFq2[] = {{2, 1}, {1, 1}, {2, 1}, {2, 1}, {1, 1}, {1, 1}};
  if ((field == 0 || field == 1) && op >= 0 && op < (int)(sizeof(kFp) / sizeof(kFp[0]))) return kFp[op];
  if (field == 2 && op >= 0 && op < (int)(sizeof(kFq2) / sizeof(kFq2[0]))) return kFq2[op];
  return {0, 0};
}

template <class PRM>
ZK_DEV void store_prim(void* p, const Fp<PRM>& v, int raw) {
  if (!raw) {
    store_fp<PRM>(p, v);
    return;
  }
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}
ZK_DEV void store_prim(void* p, const Fq2& v, int raw) {
  store_prim(p, v.c0, raw);
  store_prim(reinterpret_cast<char*>(p) + 32, v.c1, raw);
}

// in: the op's operand arrays (n elements each) back to back; out: its result arrays, likewise. F = Fq, Fr or Fq2.
template <class F>
__global__ __launch_bounds__(256) void field_prim_kernel(int op, const void* in, void* out, uint64_t n, int raw) {
  uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  constexpr int B = FieldBytes<F>::N;
  const char* src = reinterpret_cast<const char*>(in);
  char* dst = reinterpret_cast<char*>(out);
  auto arg = [&](int j) { return load_field<F>(src + (j * n + i) * B); };
  auto put = [&](int j, const F& v) { store_prim(dst + (j * n + i) * B, v, raw); };
  if constexpr (std::is_same<F, Fq2>::value) {   // Fq2: mul, sqr, add, sub, neg, inv
    F r;
    switch (op) {
      case 0: r = arg(0) * arg(1); break;
      case 1: r = arg(0).sqr(); break;
      case 2: r = arg(0) + arg(1); break;
      case 3: r = arg(0) - arg(1); break;
      case 4: r = arg(0).neg(); break;
      default: r = arg(0).inv(); break;
    }
    put(0, r);
    return;
  } else {
    auto flag = [&](bool b) {
      F r = F::zero();
      r.l[0] = b ? 1u : 0u;
      put(0, r);
    };
    F r0, r1;
    switch (op) {
      case 0: put(0, arg(0) * arg(1)); break;
      case 1: put(0, arg(0).sqr()); break;
      case 2: put(0, arg(0) + arg(1)); break;
      case 3: put(0, arg(0) - arg(1)); break;
      case 4: put(0, arg(0).neg()); break;
      case 5: put(0, arg(0).neg_2p()); break;
      case 6: put(0, arg(0).dbl()); break;
      case 7: put(0, arg(0).canon()); break;
      case 8: put(0, F::reduce_2p(arg(0))); break;
      case 9: put(0, arg(0).inv()); break;
      case 10: put(0, F::dot2(arg(0), arg(1), arg(2), arg(3))); break;
      case 11: put(0, F::dot3(arg(0), arg(1), arg(2), arg(3), arg(4), arg(5))); break;
      case 12:
        F::mul_pair(arg(0), arg(1), arg(2), arg(3), r0, r1);
        put(0, r0);
        put(1, r1);
        break;
      case 13:
        F::sqr_pair(arg(0), arg(1), r0, r1);
        put(0, r0);
        put(1, r1);
        break;
      case 14:
        F::dot2_pair(arg(0), arg(1), arg(2), arg(3), arg(4), arg(5), arg(6), arg(7), r0, r1);
        put(0, r0);
        put(1, r1);
        break;
      case 15: flag(arg(0).is_zero()); break;
      default: flag(arg(0) == arg(1)); break;
    }
  }
}

// F = Fq, Fr or Fq2
template <class F>
inline void field_prim_run(zkpoa_context* ctx, int field, int op, const void* in, void* out, uint64_t n, int raw) {
  const PrimArity ar = field_prim_arity(field, op);
  if (ar.in == 0) throw HipError("field_prim: bad field/op");
  if (n == 0) return;
  constexpr size_t B = FieldBytes<F>::N;
  LaneIn din(in, ar.in * B, n);
  LaneOut dout(out, ar.out * B, n);
  hipStream_t st = ctx->dev.lanes[0].stream;
  hipLaunchKernelGGL((field_prim_kernel<F>), dim3(blocks_of(n, 256)), dim3(256), 0, st, op, din.template at<const void>(0),
                     dout.template at<void>(0), n, raw);
  finish(st);
  dout.down();
}

// curve op: 0 = xyzz_add(a, b XYZZ), 1 = xyzz_add_affine(a, b affine, negate k != 0), 2 = xyzz_dbl(a),
// 3 = xyzz_dbl_affine(b affine), 4 = xyzz_mul_small(a, k). Results stored as computed (coordinates in [0, 2p)).
constexpr int kCurvePrimOps = 5;

template <class F>
__global__ __launch_bounds__(256) void curve_prim_kernel(int op, const void* a, const void* b, const uint32_t* k,
                                                         void* out, uint64_t n) {
  uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  XYZZ<F> r;
  switch (op) {
    case 0:
      r = load_xyzz<F>(a, i);
      xyzz_add(r, load_xyzz<F>(b, i));
      break;
    case 1:
      r = load_xyzz<F>(a, i);
      xyzz_add_affine(r, load_affine<F>(b, i), k[i] != 0);
      break;
    case 2: r = xyzz_dbl(load_xyzz<F>(a, i)); break;
    case 3: r = xyzz_dbl_affine(load_affine<F>(b, i)); break;
    default: r = xyzz_mul_small(load_xyzz<F>(a, i), k[i]); break;
  }
  constexpr int FB = FieldBytes<F>::N;
  char* o = reinterpret_cast<char*>(out) + i * (4 * FB);
  store_prim(o, r.x, 1);
  store_prim(o + FB, r.y, 1);
  store_prim(o + 2 * FB, r.zz, 1);
  store_prim(o + 3 * FB, r.zzz, 1);
}

template <class F>
inline void curve_prim_run(zkpoa_context* ctx, int op, const void* a, const void* b, const uint32_t* k, void* out,
                           uint64_t n) {
  if (op < 0 || op >= kCurvePrimOps) throw HipError("curve_prim: bad op");
  if (n == 0) return;
  constexpr size_t X = MsmSizes<F>::kXyzz;
  const bool use_a = op != 3, use_b = op <= 1 || op == 3, use_k = op == 1 || op == 4;
  const size_t bsz = op == 0 ? X : MsmSizes<F>::kAffine;
  // an operand the op does not use: no items, so nothing is read from the caller's pointer
  LaneIn da(a, X, use_a ? n : 0), db(b, bsz, use_b ? n : 0), dk(k, 4, use_k ? n : 0);
  LaneOut dout(out, X, n);
  hipStream_t st = ctx->dev.lanes[0].stream;
  hipLaunchKernelGGL((curve_prim_kernel<F>), dim3(blocks_of(n, 256)), dim3(256), 0, st, op, da.template at<const void>(0),
                     db.template at<const void>(0), dk.template at<const uint32_t>(0), dout.template at<void>(0), n);
  finish(st);
  dout.down();
}

}  // namespace zkpoa
