// out[i] = k_i * P_i: the multiplication of `powersoftau contribute` (csrc/ptau_contribute.hip), where every point of
// sections 2-5 meets its own full-width scalar tau^i, alpha tau^i or beta tau^i. Generic over the coordinate field,
// instantiated in ptau_mul_g1.hip and ptau_mul_g2.hip.
//
// Neither multiplication kernel of csrc/setup.hip fits: setup_scale_kernel has one scalar for all lanes, and
// setup_mul_kernel is bit-serial over coefficients that are mostly short. Here every scalar has 254 bits and every
// lane's bits differ, which is the case ec_mul_windowed (csrc/ec_ntt.hip.h, the EC NTT's multiplier) was written for: 64 windows of signed 4-bit
// digits, 4 doublings and one table addition per window in every lane, whatever the scalar -- the lanes of a wave stay
// converged but for the one window in 17 whose digit is zero. Per point: 256 doublings + 7 (table) + ~60 additions,
// all xyzz_dbl / xyzz_add of bn254_ec.hip.h (complete: P + P, P - P, infinity on either side). k = 0 and P = O give
// infinity; k above r / 2 runs as (r - k) on -P.
// The XYZZ results go through a scratch buffer and come out affine by ec_ntt_store_kernel: one field inversion per run
// of 16 points (Montgomery's trick), canonical coordinates, infinity all-zero.
#pragma once
#include "ec_ntt.hip.h"

namespace zkpoa {

constexpr uint32_t kMulEachThreads = 64;   // as the butterflies of ec_ntt.hip.h: the window table lives in scratch

template <class F>
static __global__ __launch_bounds__(kMulEachThreads) void scalar_mul_each_kernel(const void* __restrict__ points,
                                                                                 const void* __restrict__ scalars,
                                                                                 uint64_t i0, uint32_t cnt,
                                                                                 void* __restrict__ out_xyzz,
                                                                                 uint32_t* __restrict__ flags) {
  const uint32_t t = blockIdx.x * kMulEachThreads + threadIdx.x;
  if (t >= cnt) return;
  uint32_t k[8];
  load_scalar(reinterpret_cast<const char*>(scalars) + 32 * i0, t, k);
  uint32_t bw = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) (void)subb(k[i], FrParams::P[i], bw);
  if (!bw) {   // k >= r
    atomicOr(flags, 1u);
    store_xyzz(out_xyzz, t, XYZZ<F>::inf());
    return;
  }
  const XYZZ<F> q = XYZZ<F>::from_affine(load_affine<F>(points, i0 + t));
#ifdef ZKPOA_PTAU_MUL_BITSERIAL
  // tools/ptau_mul_ab.hip only (A/B measurement): plain double-and-add of the setup_mul_kernel form, MSB first, one
  // doubling site and one addition site; the lanes of a wave take the addition whenever any of them has the bit set
  const bool neg = scalar_normalize(k);
  const Affine<F> p = load_affine<F>(points, i0 + t);
  XYZZ<F> acc = XYZZ<F>::inf();
  for (int bit = 253; bit >= 0; bit--) {
    acc = xyzz_dbl(acc);
    if ((k[bit >> 5] >> (bit & 31)) & 1u) xyzz_add_affine(acc, p, neg);
  }
  (void)q;
  store_xyzz(out_xyzz, t, acc);
#else
  store_xyzz(out_xyzz, t, ec_mul_windowed(q, k));
#endif
}

// XYZZ scratch of a slab (at most kMulEachSlab points at a time go through it)
constexpr uint64_t kMulEachSlab = 1ull << 20;
template <class F>
size_t scalar_mul_each_scratch_bytes(uint64_t n, uint64_t slab) {
  return (size_t)(n < slab ? n : slab) * MsmSizes<F>::kXyzz;
}
// enqueued on st, not synchronised; d_out may be d_points (a slab's points are read before its results are stored).
// d_scratch: scalar_mul_each_scratch_bytes(n, slab) of device memory, the caller's (one allocation per command).
template <class F>
void scalar_mul_each(hipStream_t st, const void* d_points, const void* d_scalars, uint64_t n, void* d_out, uint32_t* d_flags,
                     void* d_scratch, uint64_t slab) {
  if (n == 0) return;
  if (n >> 32) throw HipError("scalar_mul_each: 2^32 points or more in one call");
  if (!slab) slab = kMulEachSlab;
  for (uint64_t off = 0; off < n; off += slab) {
    const uint32_t cnt = (uint32_t)(n - off < slab ? n - off : slab);
    hipLaunchKernelGGL((scalar_mul_each_kernel<F>), dim3((cnt + kMulEachThreads - 1) / kMulEachThreads), dim3(kMulEachThreads),
                       0, st, d_points, d_scalars, off, cnt, d_scratch, d_flags);
    hipLaunchKernelGGL((ec_ntt_store_kernel<F>), dim3((uint32_t)((cnt + 256 * kEcNttRun - 1) / (256 * kEcNttRun))), dim3(256),
                       0, st, (const void*)d_scratch, (uint64_t)cnt,
                       (void*)(reinterpret_cast<char*>(d_out) + off * MsmSizes<F>::kAffine));
  }
  ZK_HIP(hipGetLastError());
}

}  // namespace zkpoa
