// Inverse NTT whose elements are curve points (ffjavascript's G.ifft / lagrangeEvaluations): what `snarkjs powersoftau
// prepare phase2` runs per level to turn the powers tau^i X into the Lagrange form L_j(tau) X (csrc/ptau_prepare.hip).
//   out[j] = sum_i (w_n^(-i j) / n) in[i],   n = 2^k,  w_n from the root-of-unity table of ntt.hip.h
// Generic over the coordinate field (F = Fq: G1, 64 B per point; F = Fq2: G2, 128 B), instantiated in ec_ntt_g1.hip and
// ec_ntt_g2.hip. Wire format in and out (affine, Montgomery, canonical, infinity all-zero); XYZZ<F> in between.
//
// Shape: radix-2 decimation in time over one global XYZZ work buffer, one kernel launch per stage, one butterfly per
// thread, every size on the same path (n / 2 threads in workgroups of 64: 2^8 points are already two workgroups).
//   load    W[p] = in[bitrev_k(p)]                                            (the only pass that reads `in`)
//   stage s, s < k: (a, b) = (W[i], W[i + 2^s]) -> (a + [t] b, a - [t] b),    t = w_{2^(s+1)}^(-j),  j = i mod 2^s
//   store   XYZZ -> affine, one field inversion per run of 16 points (Montgomery's trick), wire format into `out`
// The factor 1/n costs two scalar multiplications per transform instead of n: W[0] and W[1] are scaled at load, and
// in block 0 of every stage (i < 2^s) `a` is then already scaled while `b` is not, so that butterfly's twiddle is
// t / n. After stage s the first 2^(s+1) points carry the factor, after the last stage all of them.
// Twiddles: stage 0 has none (every t is 1), and j = 0 outside block 0 is 1 as well: those lanes skip the multiplier.
// Threads are numbered j-major (thread = j * blocks + block), so in the early stages, where a few distinct twiddles
// serve many blocks, whole waves share one twiddle: the waves of j = 0 do no multiplication at all, the others run
// without divergence; in the late stages consecutive lanes take consecutive points. -1 never occurs as a twiddle of
// this form (j < 2^s), and a twiddle above r / 2 is replaced by r - t on the negated point (scalar_normalize).
//
// The multiplication [t] Q, t a full-width element of Fr that differs per lane: fixed window, signed 4-bit digits.
// Bit-serial double-and-add would take the addition branch on nearly every bit (some lane of the wave has the bit set):
// 253 doublings + ~250 additions per wave. Here every lane runs 64 windows of 4 doublings + 1 addition from a table
// 1Q .. 8Q (7 additions to build; the table is a per-lane array indexed by the digit, which the compiler keeps in
// scratch memory: 1 KiB per lane for G1, 2 KiB for G2, read 64 times per multiplication). Per butterfly with a
// non-trivial twiddle: 256 doublings + 71 additions + the 2 additions of the butterfly itself; a digit is zero in one
// window of 17, which skips that addition for the lane. All additions are xyzz_add / xyzz_dbl of bn254_ec.hip.h,
// complete for P + P, P - P and infinity on either side.
#pragma once
#include "bn254_ec.hip.h"
#include "msm.hip.h"
#include "ntt.hip.h"
#include "zkpoa_internal.hpp"

namespace zkpoa {

constexpr uint32_t kEcNttThreads = 64;   // butterflies per workgroup
constexpr uint32_t kEcNttRun = 16;       // points per inversion in the store pass

// [k] q for k in standard form, canonical (below r); k is used up
template <class F>
ZK_DEV XYZZ<F> ec_mul_windowed(const XYZZ<F>& q, uint32_t (&k)[8]) {
  if (q.is_inf()) return q;
  const bool neg = scalar_normalize(k);   // k <= (r - 1) / 2 < 2^253
  // signed digits d_i in [-7, 8], k = sum d_i 16^i: magnitudes packed as nibbles, signs as a bit mask
  uint32_t mag[8];
  uint64_t sgn = 0;
  uint32_t carry = 0;
#pragma unroll
  for (int w = 0; w < 8; w++) {
    uint32_t out = 0;
#pragma unroll
    for (int d = 0; d < 8; d++) {
      uint32_t v = ((k[w] >> (4 * d)) & 15u) + carry;
      carry = v > 8u;
      if (carry) {
        v = 16u - v;
        sgn |= 1ull << (8 * w + d);
      }
      out |= v << (4 * d);
    }
    mag[w] = out;
  }
  XYZZ<F> tab[8];   // (m + 1) * (+-q)
  tab[0] = neg ? xyzz_neg(q) : q;
#pragma unroll 1
  for (int m = 1; m < 8; m++) {
    XYZZ<F> e = tab[m - 1];
    xyzz_add(e, tab[0]);
    tab[m] = e;
  }
  XYZZ<F> acc = XYZZ<F>::inf();
#pragma unroll 1
  for (int i = 0; i < 64; i++) {   // most significant digit first
#pragma unroll 1
    for (int d = 0; d < 4; d++) acc = xyzz_dbl(acc);
    const uint32_t m = mag[7] >> 28;
    const bool minus = (sgn >> 63) != 0;
#pragma unroll
    for (int w = 7; w > 0; w--) mag[w] = (mag[w] << 4) | (mag[w - 1] >> 28);
    mag[0] <<= 4;
    sgn <<= 1;
    if (m) {
      XYZZ<F> e = tab[m - 1];
      if (minus) e.y = e.y.neg();
      xyzz_add(acc, e);
    }
  }
  return acc;
}

// [t] q for t in Montgomery form (any element of Fr)
template <class F>
ZK_DEV XYZZ<F> ec_ntt_mul(const XYZZ<F>& q, const Fr& t_mont) {
  const Fr t = t_mont.from_mont().canon();
  uint32_t k[8];
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = t.l[i];
  return ec_mul_windowed(q, k);
}

// W[p] = in[bitrev_k(p)] as XYZZ; W[0] and W[1] times 1 / n (k > 0)
template <class F>
static __global__ __launch_bounds__(kEcNttThreads) void ec_ntt_load_kernel(const void* __restrict__ in, uint32_t k,
                                                                           Fr inv_n, void* __restrict__ W) {
  const uint64_t p = (uint64_t)blockIdx.x * kEcNttThreads + threadIdx.x;
  if (p >> k) return;
  const uint32_t src = k ? __brev((uint32_t)p) >> (32u - k) : 0u;
  XYZZ<F> a = XYZZ<F>::from_affine(load_affine<F>(in, src));
  if (k && p < 2) a = ec_ntt_mul(a, inv_n);
  store_xyzz(W, p, a);
}

// stage s of k (see the header comment); tw[e] = w_{2^log_tw}^(-e), e < 2^(log_tw - 1), Montgomery form, log_tw >= k
template <class F>
static __global__ __launch_bounds__(kEcNttThreads) void ec_ntt_stage_kernel(void* __restrict__ W, uint32_t k, uint32_t s,
                                                                            const void* __restrict__ tw, uint32_t log_tw,
                                                                            Fr inv_n) {
  const uint64_t t = (uint64_t)blockIdx.x * kEcNttThreads + threadIdx.x;
  if (t >> (k - 1u)) return;
  const uint32_t log_blocks = k - 1u - s;
  const uint64_t j = t >> log_blocks, blk = t & ((1ull << log_blocks) - 1u);
  const uint64_t i = (blk << (s + 1u)) + j;
  XYZZ<F> b = load_xyzz<F>(W, i + (1ull << s));
  if (s && (j || !blk)) {
    Fr w = load_field<Fr>(reinterpret_cast<const char*>(tw) + 32 * (j << (log_tw - 1u - s)));
    if (!blk) w = w * inv_n;
    b = ec_ntt_mul(b, w);
  }
  const XYZZ<F> a = load_xyzz<F>(W, i);   // after the multiplication: not live across it
#pragma unroll 1
  for (int h = 0; h < 2; h++) {
    XYZZ<F> r = a;
    xyzz_add(r, h ? xyzz_neg(b) : b);
    store_xyzz(W, i + ((uint64_t)h << s), r);
  }
}

// out[e] = W[e] in wire format, e < n. One inversion per run of kEcNttRun points: the prefix products of the ZZZ
// coordinates (1 for a point at infinity) go through the points' own slots in `out`.
template <class F>
static __global__ __launch_bounds__(256) void ec_ntt_store_kernel(const void* __restrict__ W, uint64_t n,
                                                                  void* __restrict__ out) {
  const uint64_t e0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * kEcNttRun;
  if (e0 >= n) return;
  const uint32_t m = (uint32_t)(n - e0 < kEcNttRun ? n - e0 : kEcNttRun);
  constexpr int FB = FieldBytes<F>::N;
  const char* w = reinterpret_cast<const char*>(W) + e0 * (4 * FB);
  char* o = reinterpret_cast<char*>(out) + e0 * (2 * FB);
  F acc = F::one();
  for (uint32_t e = 0; e < m; e++) {
    const F zzz = load_field<F>(w + e * (4 * FB) + 3 * FB);
    store_field(o + e * (2 * FB), acc);
    if (!zzz.is_zero()) acc = acc * zzz;
  }
  F inv = acc.inv();
  for (int e = (int)m - 1; e >= 0; e--) {
    const XYZZ<F> p = load_xyzz<F>(w, (size_t)e);
    char* oe = o + e * (2 * FB);
    if (p.is_inf() || p.zzz.is_zero()) {
      store_field(oe, F::zero());
      store_field(oe + FB, F::zero());
      continue;
    }
    const F i3 = inv * load_field<F>(oe);   // 1 / ZZZ
    inv = inv * p.zzz;
    const F i2 = (p.zz * i3).sqr();         // 1 / ZZ
    store_field(oe, p.x * i2);
    store_field(oe + FB, p.y * i3);
  }
}

// w_{2^log_max}^(-e), e < 2^(log_max - 1): serves every transform of up to 2^log_max points (ec_intt_run's log_tw)
inline void ec_intt_twiddles(hipStream_t st, uint32_t log_max, void* tw) {
  if (log_max < 2) return;   // stage 0 has no twiddles
  build_pow_table(st, hfr_root_of_unity(log_max).inv(), HFr::one(), 1u << (log_max - 1), tw);
}

// Enqueues the transform of 2^k points on st. d_out may be d_in: `in` is read by the load pass only.
template <class F>
void ec_intt_run(hipStream_t st, EcNttWork& wk, const void* d_in, uint32_t k, void* d_out) {
  if (k > wk.log_max) throw HipError("ec_intt: more points than the work buffer holds");
  HFr n_inv = HFr::one();
  {
    const HFr half = HFr::from_u64(2).inv();
    for (uint32_t i = 0; i < k; i++) n_inv = n_inv * half;
  }
  const Fr inv_n = to_dev(n_inv);
  const uint64_t n = 1ull << k;
  hipLaunchKernelGGL((ec_ntt_load_kernel<F>), dim3((uint32_t)((n + kEcNttThreads - 1) / kEcNttThreads)),
                     dim3(kEcNttThreads), 0, st, d_in, k, inv_n, wk.work.p);
  if (k) {
    const dim3 grid((uint32_t)((n / 2 + kEcNttThreads - 1) / kEcNttThreads));
    for (uint32_t s = 0; s < k; s++)
      hipLaunchKernelGGL((ec_ntt_stage_kernel<F>), grid, dim3(kEcNttThreads), 0, st, wk.work.p, k, s, (const void*)wk.tw.p,
                         wk.log_max, inv_n);
  }
  hipLaunchKernelGGL((ec_ntt_store_kernel<F>), dim3((uint32_t)((n + 256 * kEcNttRun - 1) / (256 * kEcNttRun))), dim3(256),
                     0, st, (const void*)wk.work.p, n, d_out);
  ZK_HIP(hipGetLastError());
}

template <class F>
EcNttWork* ec_intt_work(zkpoa_context* ctx, uint32_t log_max) {
  if (log_max > 28) throw HipError("ec_intt: more than 2^28 points (BN254's Fr has no root of unity of that order)");
  EcNttWork* wk = new EcNttWork(log_max, MsmSizes<F>::kXyzz << log_max, log_max ? (size_t)32 << (log_max - 1) : 32);
  try {
    ec_intt_twiddles(ctx->dev.lanes[0].stream, log_max, wk->tw.p);
    ZK_HIP(hipGetLastError());
  } catch (...) {
    delete wk;
    throw;
  }
  return wk;
}

}  // namespace zkpoa
