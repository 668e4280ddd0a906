// Keccak-f[1600] and Keccak-256 (the Keccak submission's padding, first pad byte 0x01, as Ethereum uses it; SHA3-256 is
// the same sponge with 0x06), one message per lane. The 25 lanes of 64 bits are held as u32 pairs in registers; a
// rotation by a compile-time amount is two 32-bit funnel shifts (v_alignbit_b32), by 32 a swap of the halves.
// The 24 rounds are NOT unrolled (#pragma unroll 1): one round is about 450 instructions, all 24 would be ~43 KB, most
// of the 64 KB instruction cache that the recovery kernel's field code has to share; the round constant is read from
// a table by the (wave-uniform) round index. Every index into the state is a compile-time constant.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef ZK_HD
#define ZK_HD __host__ __device__ __forceinline__
#endif

namespace zkpoa {
namespace keccak {

constexpr int kRate = 136;   // bytes per block of Keccak-256

template <int N>
ZK_HD uint64_t rotl(uint64_t x) {
  if (N == 0) return x;
  const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  if (N == 32) return ((uint64_t)lo << 32) | hi;
  constexpr int S = N & 31;
  constexpr int L = S ? S : 1, Rr = S ? 32 - S : 31;   // (S == 0 only for N == 0 / 32, handled above)
  const uint32_t a = (hi << L) | (lo >> Rr);   // funnel shift of hi:lo
  const uint32_t b = (lo << L) | (hi >> Rr);   // funnel shift of lo:hi
  return N < 32 ? (((uint64_t)a << 32) | b) : (((uint64_t)b << 32) | a);
}

ZK_HD uint64_t round_constant(int r) {
  constexpr uint64_t rc[24] = {
      0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull,
      0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull,
      0x0000000080008009ull, 0x000000008000000aull, 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull,
      0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
      0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
  return rc[r];
}

// b[y][2x + 3y] = rotl(a[x][y], rho[x][y]); lane (x, y) is a[x + 5 y]
#define ZK_KECCAK_RHO_PI(X, Y, N) b[(Y) + 5 * ((2 * (X) + 3 * (Y)) % 5)] = rotl<N>(a[(X) + 5 * (Y)])

ZK_HD void f1600(uint64_t (&a)[25]) {
#pragma unroll 1
  for (int round = 0; round < 24; round++) {
    uint64_t c[5], b[25];
#pragma unroll
    for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
    for (int x = 0; x < 5; x++) {
      const uint64_t d = c[(x + 4) % 5] ^ rotl<1>(c[(x + 1) % 5]);
#pragma unroll
      for (int y = 0; y < 5; y++) a[x + 5 * y] ^= d;
    }
    ZK_KECCAK_RHO_PI(0, 0, 0);  ZK_KECCAK_RHO_PI(1, 0, 1);  ZK_KECCAK_RHO_PI(2, 0, 62); ZK_KECCAK_RHO_PI(3, 0, 28); ZK_KECCAK_RHO_PI(4, 0, 27);
    ZK_KECCAK_RHO_PI(0, 1, 36); ZK_KECCAK_RHO_PI(1, 1, 44); ZK_KECCAK_RHO_PI(2, 1, 6);  ZK_KECCAK_RHO_PI(3, 1, 55); ZK_KECCAK_RHO_PI(4, 1, 20);
    ZK_KECCAK_RHO_PI(0, 2, 3);  ZK_KECCAK_RHO_PI(1, 2, 10); ZK_KECCAK_RHO_PI(2, 2, 43); ZK_KECCAK_RHO_PI(3, 2, 25); ZK_KECCAK_RHO_PI(4, 2, 39);
    ZK_KECCAK_RHO_PI(0, 3, 41); ZK_KECCAK_RHO_PI(1, 3, 45); ZK_KECCAK_RHO_PI(2, 3, 15); ZK_KECCAK_RHO_PI(3, 3, 21); ZK_KECCAK_RHO_PI(4, 3, 8);
    ZK_KECCAK_RHO_PI(0, 4, 18); ZK_KECCAK_RHO_PI(1, 4, 2);  ZK_KECCAK_RHO_PI(2, 4, 61); ZK_KECCAK_RHO_PI(3, 4, 56); ZK_KECCAK_RHO_PI(4, 4, 14);
#pragma unroll
    for (int y = 0; y < 5; y++) {
#pragma unroll
      for (int x = 0; x < 5; x++) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
    }
    a[0] ^= round_constant(round);
  }
}
#undef ZK_KECCAK_RHO_PI

// Keccak-256 of msg[0 .. len): any length; the padded message is absorbed 136 bytes at a time. digest: 4 words, the
// 32 bytes in order when stored little-endian.
ZK_HD void keccak256(const uint8_t* msg, uint32_t len, uint64_t (&digest)[4]) {
  uint64_t a[25];
#pragma unroll
  for (int i = 0; i < 25; i++) a[i] = 0;
  const uint32_t blocks = len / kRate + 1;
#pragma unroll 1
  for (uint32_t blk = 0; blk < blocks; blk++) {
    const uint32_t base = blk * kRate;
#pragma unroll
    for (int w = 0; w < kRate / 8; w++) {
      uint64_t word = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const uint32_t j = base + 8 * w + k;
        uint32_t byte = j < len ? msg[j] : (j == len ? 0x01u : 0u);
        if (j == blocks * kRate - 1) byte |= 0x80u;
        word |= (uint64_t)byte << (8 * k);
      }
      a[w] ^= word;
    }
    f1600(a);
  }
#pragma unroll
  for (int i = 0; i < 4; i++) digest[i] = a[i];
}

}  // namespace keccak
}  // namespace zkpoa
