// Does the 9 x 29-bit field (csrc/fq29.hip.h) beat the 8 x 32-bit one (csrc/bn254_field.hip.h) where the G1 bucket
// accumulation uses it? Register-only loops of product, square, dot2 and the mixed addition in both forms, by waves
// per SIMD, and the issue cost of the two 64-bit shift instructions the compiler builds the column shift from.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I zk-proof-of-assets_amd/csrc tools/microbench_limb29.hip -o tools/microbench_limb29
#include "bn254_ec.hip.h"
#include "fq29.hip.h"
#include <stdio.h>
#include <algorithm>
#include <vector>
using namespace zkpoa;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)

ZK_DEV Fq29 ld29(const uint4* in, int t) {   // a canonical element (< q), re-limbed
  const Fq a = load_field<Fq>(in + 2 * (t & 1023));
  return fq29_from_words(a.l);
}
ZK_DEV void st29(uint4* out, int t, const Fq29& a) {
  uint32_t s = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) s ^= a.l[i];
  reinterpret_cast<uint32_t*>(out)[t] = s;
}

// op 0 product, 1 square, 2 dot2; each result feeds the next operation
template <int OP>
__global__ __launch_bounds__(256) void k_f32(const uint4* in, uint4* out, int iters) {
  int t = blockIdx.x * 256 + threadIdx.x;
  Fq x = load_field<Fq>(in + 2 * (t & 1023)), y = load_field<Fq>(in + 2 * ((t + 1) & 1023));
  Fq z = load_field<Fq>(in + 2 * ((t + 2) & 1023));
  Fq w = load_field<Fq>(in + 2 * ((t + 3) & 1023));
  for (int i = 0; i < iters; i++) {   // dot2: four different operands every time (z, w trail x by one and two steps)
    const Fq n = OP == 0 ? x * y : (OP == 1 ? x.sqr() : Fq::dot2(x, y, z, w));
    w = z;
    z = x;
    x = n;
  }
  store_field(out + 2 * t, x + z + w);
}
template <int OP>
__global__ __launch_bounds__(256) void k_f29(const uint4* in, uint4* out, int iters) {
  int t = blockIdx.x * 256 + threadIdx.x;
  Fq29 x = ld29(in, t), y = ld29(in, t + 1), z = ld29(in, t + 2);
  Fq29 w = ld29(in, t + 3);
  for (int i = 0; i < iters; i++) {
    const Fq29 n = OP == 0 ? fq29_mul(x, y) : (OP == 1 ? fq29_sqr(x) : fq29_dot2(x, y, z, w));
    w = z;
    z = x;
    x = n;
  }
  st29(out, t, fq29_sub<Fq29C4>(fq29_sub<Fq29C4>(x, z), w));
}

// the mixed addition as the accumulation kernel runs it: 3 waves per SIMD
__global__ __launch_bounds__(256, 3) void k_madd32(const uint4* in, uint4* out, int iters) {
  int t = blockIdx.x * 256 + threadIdx.x;
  Affine<Fq> p = {load_field<Fq>(in + 2 * (t & 1023)), load_field<Fq>(in + 2 * ((t + 7) & 1023))};
  XYZZ<Fq> acc = {load_field<Fq>(in + 2 * ((t + 1) & 1023)), load_field<Fq>(in + 2 * ((t + 2) & 1023)),
                  load_field<Fq>(in + 2 * ((t + 3) & 1023)), load_field<Fq>(in + 2 * ((t + 4) & 1023))};
  for (int i = 0; i < iters; i++) xyzz_add_affine(acc, p, (i & 1) != 0);
  store_field(out + 2 * t, acc.x + acc.y + acc.zz + acc.zzz);
}
__global__ __launch_bounds__(256, 3) void k_madd29(const uint4* in, uint4* out, int iters) {
  int t = blockIdx.x * 256 + threadIdx.x;
  Affine<Fq> p = {load_field<Fq>(in + 2 * (t & 1023)), load_field<Fq>(in + 2 * ((t + 7) & 1023))};
  G1Piece29 s;
  s.empty = false;
  s.a = {ld29(in, t + 1), ld29(in, t + 2), ld29(in, t + 3), ld29(in, t + 4)};
  for (int i = 0; i < iters; i++) g1piece29_add(s, p.x.l, p.y.l, (i & 1) != 0);   // re-limbs the base every time
  uint32_t w[32];
  g1piece29_finish(s, w);
  uint32_t x = 0;
#pragma unroll
  for (int i = 0; i < 32; i++) x ^= w[i];
  reinterpret_cast<uint32_t*>(out)[t] = x;
}

// issue cost of the 64-bit shifts: 4 independent chains each, as k_mad of tools/microbench4.hip
__global__ __launch_bounds__(256) void k_lshr64(uint32_t* out, uint32_t a0, int iters) {
  uint64_t acc[4];
#pragma unroll
  for (int k = 0; k < 4; k++) acc[k] = ((uint64_t)(a0 + threadIdx.x) << 32) | (k + blockIdx.x);
  for (int i = 0; i < iters; i++) {
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
      for (int k = 0; k < 4; k++) asm volatile("v_lshrrev_b64 %0, 1, %0" : "+v"(acc[k]));
  }
  uint64_t s = acc[0] + acc[1] + acc[2] + acc[3];
  out[blockIdx.x * 256 + threadIdx.x] = (uint32_t)s ^ (uint32_t)(s >> 32);
}
__global__ __launch_bounds__(256) void k_lshladd64(uint32_t* out, uint32_t a0, int iters) {
  uint64_t acc[4];
  uint64_t b = a0 + threadIdx.x;
#pragma unroll
  for (int k = 0; k < 4; k++) acc[k] = k + blockIdx.x;
  for (int i = 0; i < iters; i++) {
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
      for (int k = 0; k < 4; k++) asm volatile("v_lshl_add_u64 %0, %0, 1, %1" : "+v"(acc[k]) : "v"(b));
  }
  uint64_t s = acc[0] + acc[1] + acc[2] + acc[3];
  out[blockIdx.x * 256 + threadIdx.x] = (uint32_t)s ^ (uint32_t)(s >> 32);
}
__global__ __launch_bounds__(256) void k_mad64(uint32_t* out, uint32_t a0, uint32_t b0, int iters) {   // plain C++ mad, no carry
  uint64_t acc[4];
  uint32_t a = a0 + threadIdx.x, b = b0 + blockIdx.x;
#pragma unroll
  for (int k = 0; k < 4; k++) acc[k] = k;
  for (int i = 0; i < iters; i++) {
#pragma unroll
    for (int r = 0; r < 2; r++) {
      uint64_t c0, c1, c2, c3;
      asm volatile("v_mad_u64_u32 %0, %4, %8, %9, %0\n\t"
                   "v_mad_u64_u32 %1, %5, %8, %9, %1\n\t"
                   "v_mad_u64_u32 %2, %6, %8, %9, %2\n\t"
                   "v_mad_u64_u32 %3, %7, %8, %9, %3"
                   : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "=&s"(c0), "=&s"(c1), "=&s"(c2), "=&s"(c3)
                   : "v"(a), "v"(b));
    }
  }
  uint64_t s = acc[0] + acc[1] + acc[2] + acc[3];
  out[blockIdx.x * 256 + threadIdx.x] = (uint32_t)s ^ (uint32_t)(s >> 32);
}

// median and spread of 5 timed launches after one warm-up
struct T { float med, lo, hi; };
template <class K, class... A>
T timeit(K kernel, int grid, A... args) {
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, 0, args...);
  CK(hipDeviceSynchronize());
  float ms[5];
  for (int r = 0; r < 5; r++) {
    CK(hipEventRecord(e0));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, 0, args...);
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(&ms[r], e0, e1));
  }
  CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
  std::sort(ms, ms + 5);
  return {ms[2], ms[0], ms[4]};
}

int main() {
  hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  const double clk = prop.clockRate * 1e3;   // Hz
  printf("%s, %d CUs, %.0f MHz\n", prop.name, cus, clk / 1e6);
  uint32_t* d32; CK(hipMalloc(&d32, 64 << 20));
  std::vector<uint32_t> h(8 * 1024);
  for (size_t i = 0; i < h.size(); i++) h[i] = (uint32_t)(i * 2654435761u) & ((i % 8 == 7) ? 0x0fffffffu : 0xffffffffu);
  uint4* din; CK(hipMalloc(&din, 32 * 1024)); CK(hipMemcpy(din, h.data(), 32 * 1024, hipMemcpyHostToDevice));
  uint4* dout = (uint4*)d32;
  for (int wps : {1, 2, 3, 8}) {
    const int grid = cus * wps, iters = 4096;
    const double inst = (double)grid * 4 * iters * 8 / (cus * 4);   // wave-instructions per SIMD
    T a = timeit(k_lshr64, grid, d32, 3u, iters), b = timeit(k_lshladd64, grid, d32, 3u, iters),
      c = timeit(k_mad64, grid, d32, 3u, 5u, iters);
    printf("issue cost wps=%d, cycles/inst/SIMD: v_lshrrev_b64 %.2f  v_lshl_add_u64 %.2f  v_mad_u64_u32 %.2f\n", wps,
           a.med * 1e-3 * clk / inst, b.med * 1e-3 * clk / inst, c.med * 1e-3 * clk / inst);
  }
  const char* names[3] = {"product", "square ", "dot2   "};
  for (int wps : {1, 2, 3, 8}) {
    const int grid = cus * wps, iters = 1024;
    const double ops = (double)grid * 256 * iters;
    T o[3] = {timeit(k_f32<0>, grid, (const uint4*)din, dout, iters), timeit(k_f32<1>, grid, (const uint4*)din, dout, iters),
              timeit(k_f32<2>, grid, (const uint4*)din, dout, iters)};
    T n[3] = {timeit(k_f29<0>, grid, (const uint4*)din, dout, iters), timeit(k_f29<1>, grid, (const uint4*)din, dout, iters),
              timeit(k_f29<2>, grid, (const uint4*)din, dout, iters)};
    for (int k = 0; k < 3; k++)
      printf("%s wps=%d: 8x32 %.1f G/s (%.1f-%.1f)  9x29 %.1f G/s (%.1f-%.1f)  ratio %.3f\n", names[k], wps,
             ops / o[k].med / 1e6, ops / o[k].hi / 1e6, ops / o[k].lo / 1e6, ops / n[k].med / 1e6, ops / n[k].hi / 1e6,
             ops / n[k].lo / 1e6, o[k].med / n[k].med);
  }
  for (int wps : {1, 2, 3}) {
    const int grid = cus * wps, iters = 256;
    const double ops = (double)grid * 256 * iters;
    T o = timeit(k_madd32, grid, (const uint4*)din, dout, iters), n = timeit(k_madd29, grid, (const uint4*)din, dout, iters);
    printf("G1 mixed addition (launch bounds 3 waves/SIMD) wps=%d: 8x32 %.2f G adds/s (%.2f-%.2f)  9x29 %.2f (%.2f-%.2f)  ratio %.3f\n",
           wps, ops / o.med / 1e6, ops / o.hi / 1e6, ops / o.lo / 1e6, ops / n.med / 1e6, ops / n.hi / 1e6,
           ops / n.lo / 1e6, o.med / n.med);
  }
  return 0;
}
