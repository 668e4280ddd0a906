// A/B of the per-point scalar multiplication of `powersoftau contribute` (csrc/ptau_contribute.hip.h), compile-time:
//   A  hipcc --offload-arch=gfx950 -O3 -std=c++17 -I zk-proof-of-assets_amd/csrc tools/ptau_mul_ab.hip -o tools/ptau_mul_ab
//      the product's kernel: 64 signed 4-bit windows per lane (ec_mul_windowed)
//   B  ... -DZKPOA_PTAU_MUL_BITSERIAL ... -o tools/ptau_mul_ab_bitserial
//      plain MSB-first double-and-add of the setup_mul_kernel form (one doubling site, one addition site)
// Both run scalar_mul_each<F> as the product does (multiplication kernel, then the batched-inversion store kernel) over
// 2^log_n points (default 20) with a full-width scalar of its own per lane, for G1 and for G2: one warm run, then five
// timed with device events; the median is reported. One JSON line.
// The operands are pseudo-random field elements, not points of BN254: the group formulas (a = 0) never use b, so every
// (x, y) is a point of SOME curve y^2 = x^3 + b' and the arithmetic, its exceptional branches and its timing are those of
// real points. Results are not checked here (tests/test_gpu_ptau_contribute.py checks the product's kernel).
#include "ptau_contribute.hip.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

using namespace zkpoa;

// 32-byte little-endian values below 0x30644e72 * 2^224 (< r < q): full width, every lane its own
static __global__ void fill_kernel(uint32_t* out, uint64_t words32, uint64_t seed) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= words32) return;
  uint64_t z = seed + 0x9e3779b97f4a7c15ull * (i + 1);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  uint32_t v = (uint32_t)(z ^ (z >> 31));
  if ((i & 7u) == 7u) v %= 0x30644e72u;
  out[i] = v;
}

template <class F>
static double run(hipStream_t st, uint64_t n, double runs[5]) {
  constexpr size_t A = MsmSizes<F>::kAffine;
  DevBuf pts(n * A), ks(n * 32), out(n * A), flag(64), scratch(scalar_mul_each_scratch_bytes<F>(n, kMulEachSlab));
  auto fill = [&](void* p, uint64_t bytes, uint64_t seed) {
    const uint64_t w = bytes / 4;
    hipLaunchKernelGGL(fill_kernel, dim3((uint32_t)((w + 255) / 256)), dim3(256), 0, st, (uint32_t*)p, w, seed);
  };
  fill(pts.p, n * A, 1);
  fill(ks.p, n * 32, 2);
  ZK_HIP(hipMemsetAsync(flag.p, 0, 64, st));
  hipEvent_t e0, e1;
  ZK_HIP(hipEventCreate(&e0));
  ZK_HIP(hipEventCreate(&e1));
  for (int it = 0; it < 6; it++) {
    ZK_HIP(hipEventRecord(e0, st));
    scalar_mul_each<F>(st, pts.p, ks.p, n, out.p, (uint32_t*)flag.p, scratch.p, kMulEachSlab);
    ZK_HIP(hipEventRecord(e1, st));
    ZK_HIP(hipEventSynchronize(e1));
    float ms = 0;
    ZK_HIP(hipEventElapsedTime(&ms, e0, e1));
    if (it) runs[it - 1] = ms;
  }
  uint32_t bad = 0;
  ZK_HIP(hipMemcpy(&bad, flag.p, 4, hipMemcpyDeviceToHost));
  if (bad) throw HipError("a scalar was not below r");
  double sorted[5];
  std::copy(runs, runs + 5, sorted);
  std::sort(sorted, sorted + 5);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return sorted[2];
}

int main(int argc, char** argv) {
  const int log_n = argc > 1 ? atoi(argv[1]) : 20;
  if (log_n < 1 || log_n > 24) {
    fprintf(stderr, "usage: ptau_mul_ab [log_n in 1..24]\n");
    return 2;
  }
  const uint64_t n = 1ull << log_n;
  try {
    hipStream_t st;
    ZK_HIP(hipStreamCreate(&st));
    double r1[5], r2[5];
    const double g1 = run<Fq>(st, n, r1), g2 = run<Fq2>(st, n, r2);
#ifdef ZKPOA_PTAU_MUL_BITSERIAL
    const char* variant = "bit-serial double-and-add";
#else
    const char* variant = "signed 4-bit windows";
#endif
    printf("{\"variant\": \"%s\", \"log_n\": %d, \"g1_ms_median\": %.3f, \"g1_mul_per_s\": %.0f, \"g1_ms_runs\": [%.3f, %.3f, %.3f, %.3f, %.3f], "
           "\"g2_ms_median\": %.3f, \"g2_mul_per_s\": %.0f, \"g2_ms_runs\": [%.3f, %.3f, %.3f, %.3f, %.3f]}\n",
           variant, log_n, g1, n / g1 * 1e3, r1[0], r1[1], r1[2], r1[3], r1[4], g2, n / g2 * 1e3, r2[0], r2[1], r2[2], r2[3], r2[4]);
    (void)hipStreamDestroy(st);
  } catch (const std::exception& e) {
    fprintf(stderr, "ptau_mul_ab: %s\n", e.what());
    return 1;
  }
  return 0;
}
