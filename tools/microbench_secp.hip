// The parts the instruction bound of the ECDSA* kernel is built from: register-only loops of the
// secp256k1 field product and square, the product modulo the group order, the three group operations of the ladder and
// the Keccak permutation, for the signing kernel the SHA-256 compression and for BIP-32 the SHA-512 compression, at the recovery kernel's own shape (workgroups of 64, as many as fill the card twice at the
// occupancy the compiler gives them). Prints operations per second of the whole card.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I zk-proof-of-assets_amd/csrc tools/microbench_secp.hip -o tools/microbench_secp
#include "secp256k1.hip.h"
#include "sha512.hip.h"
#include <stdio.h>
#include <algorithm>
#include <vector>
using namespace zkpoa;
using namespace zkpoa::secp;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)

constexpr int kLanes = 1 << 17;   // 2048 waves: two per SIMD of 256 CUs

__device__ secp::Fp ldf(const uint32_t* in, int t) {
  secp::Fp a;
#pragma unroll
  for (int i = 0; i < 8; i++) a.l[i] = in[8 * (t & 1023) + i];
  a.l[7] &= 0x7fffffffu;   // canonical for either modulus
  return a;
}
__device__ uint32_t fold(const secp::Fp& a) {
  uint32_t s = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) s ^= a.l[i];
  return s;
}

// 0 Fp product, 1 Fp square, 2 product modulo n, 3 xyzz_dbl, 4 xyzz_add, 5 xyzz_add_affine, 6 Keccak-f[1600],
// 7 SHA-256 compression, 8 SHA-512 compression
template <int OP>
__global__ __launch_bounds__(64) void k_op(const uint32_t* in, uint32_t* out, int iters) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  uint32_t res = 0;
  if (OP <= 1) {
    secp::Fp x = ldf(in, t), y = ldf(in, t + 1);
#pragma unroll 1
    for (int i = 0; i < iters; i++) {
      const secp::Fp n = OP == 0 ? x * y : x.sqr();
      y = x;
      x = n;
    }
    res = fold(x + y);
  } else if (OP == 2) {
    Sc x, y;
    const secp::Fp a = ldf(in, t), b = ldf(in, t + 1);
#pragma unroll
    for (int i = 0; i < 8; i++) x.l[i] = a.l[i], y.l[i] = b.l[i];
#pragma unroll 1
    for (int i = 0; i < iters; i++) {
      const Sc n = x * y;
      y = x;
      x = n;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) res ^= x.l[i] ^ y.l[i];
  } else if (OP <= 5) {
    // not curve points: the formulas do the same work on any values, and the exceptional branches are as rare
    XyzzK acc = {ldf(in, t), ldf(in, t + 1), ldf(in, t + 2), ldf(in, t + 3)};
    const XyzzK b = {ldf(in, t + 4), ldf(in, t + 5), ldf(in, t + 6), ldf(in, t + 7)};
    const AffineK p = {b.x, b.y};
#pragma unroll 1
    for (int i = 0; i < iters; i++) {
      if (OP == 3) acc = xyzz_dbl(acc);
      else if (OP == 4) xyzz_add(acc, b);
      else xyzz_add_affine(acc, p, (i & 1) != 0);
    }
    res = fold(acc.x + acc.y + acc.zz + acc.zzz);
  } else if (OP == 6) {
    uint64_t a[25];
#pragma unroll
    for (int i = 0; i < 25; i++) a[i] = in[(t + i) & 8191];
#pragma unroll 1
    for (int i = 0; i < iters; i++) keccak::f1600(a);
#pragma unroll
    for (int i = 0; i < 25; i++) res ^= (uint32_t)a[i] ^ (uint32_t)(a[i] >> 32);
  } else if (OP == 8) {
    uint64_t h[8], blk[16];
#pragma unroll
    for (int i = 0; i < 16; i++) blk[i] = ((uint64_t)in[(t + 2 * i) & 8191] << 32) | in[(t + 2 * i + 1) & 8191];
    sha512::initial_state(h);
#pragma unroll 1
    for (int i = 0; i < iters; i++) {
      sha512::compress(h, blk);
      blk[3] ^= h[0];   // the next block depends on this state
    }
#pragma unroll
    for (int i = 0; i < 8; i++) res ^= (uint32_t)h[i] ^ (uint32_t)(h[i] >> 32);
  } else {
    uint32_t h[8], blk[16];
#pragma unroll
    for (int i = 0; i < 16; i++) blk[i] = in[(t + i) & 8191];
    sha256::initial_state(h);
#pragma unroll 1
    for (int i = 0; i < iters; i++) {
      sha256::compress(h, blk);
      blk[3] ^= h[0];   // the next block depends on this state
    }
#pragma unroll
    for (int i = 0; i < 8; i++) res ^= h[i];
  }
  out[t] = res;
}

template <int OP>
void run(const char* name, const uint32_t* in, uint32_t* out, int iters) {
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  std::vector<float> ms;
  for (int rep = 0; rep < 4; rep++) {   // the first is the warm run
    CK(hipEventRecord(a));
    hipLaunchKernelGGL(k_op<OP>, dim3(kLanes / 64), dim3(64), 0, 0, in, out, iters);
    CK(hipEventRecord(b));
    CK(hipEventSynchronize(b));
    CK(hipGetLastError());
    float t;
    CK(hipEventElapsedTime(&t, a, b));
    if (rep) ms.push_back(t);
  }
  std::sort(ms.begin(), ms.end());
  printf("%-18s %8d iterations x %d lanes: median %8.3f ms of 3  -> %9.3f G/s\n", name, iters, kLanes, ms[1],
         (double)iters * kLanes / ms[1] / 1e6);
}

int main() {
  std::vector<uint32_t> h(8192 + 64);
  uint32_t s = 12345;
  for (auto& v : h) v = (s = s * 1664525u + 1013904223u);
  uint32_t *in, *out;
  CK(hipMalloc(&in, h.size() * 4));
  CK(hipMalloc(&out, kLanes * 4));
  CK(hipMemcpy(in, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  run<0>("Fp product", in, out, 20000);
  run<1>("Fp square", in, out, 20000);
  run<2>("product mod n", in, out, 10000);
  run<3>("xyzz_dbl", in, out, 2000);
  run<4>("xyzz_add", in, out, 2000);
  run<5>("xyzz_add_affine", in, out, 2000);
  run<6>("Keccak-f[1600]", in, out, 2000);
  run<7>("SHA-256 compress", in, out, 4000);
  run<8>("SHA-512 compress", in, out, 2000);
  return 0;
}
