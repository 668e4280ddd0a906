// SHA-256 and HMAC-SHA256 on the device, one message per lane: the hash of `ecdsa-sigs-parser sign` (--message, the
// key derivation of --generate-keys) and the HMAC-DRBG of RFC 6979 (csrc/secp256k1.hip.h). Words are the big-endian
// 32-bit words of FIPS 180-4: word k of a message is its bytes 4k .. 4k+3, first byte highest.
//
// One compression is four passes of sixteen rounds. The sixteen rounds of a pass are unrolled, so that the rolling
// message schedule w[16] is only ever indexed by compile-time constants and stays in registers; the four passes are NOT
// (#pragma unroll 1), and the round constant is read from a table by the pass index, which is the same in every lane --
// as keccak.hip.h does with its 24 rounds. hmac32() runs its four or five compressions through ONE call of compress()
// in a loop over phases, so a kernel that makes 22 of them (an RFC 6979 nonce) still holds one copy of the round code.
// Plain ZK_HD C++: the same text runs on the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef ZK_HD
#define ZK_HD __host__ __device__ __forceinline__
#endif

namespace zkpoa {
namespace sha256 {

ZK_HD uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

ZK_HD uint32_t round_constant(int i) {
  constexpr uint32_t k[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u,
      0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu,
      0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,
      0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
      0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u,
      0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
      0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  return k[i];
}

ZK_HD void initial_state(uint32_t (&h)[8]) {
  h[0] = 0x6a09e667u;
  h[1] = 0xbb67ae85u;
  h[2] = 0x3c6ef372u;
  h[3] = 0xa54ff53au;
  h[4] = 0x510e527fu;
  h[5] = 0x9b05688cu;
  h[6] = 0x1f83d9abu;
  h[7] = 0x5be0cd19u;
}

// h <- the compression of one 64-byte block (16 big-endian words) into h
ZK_HD void compress(uint32_t (&h)[8], const uint32_t (&block)[16]) {
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = block[i];
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll 1
  for (int pass = 0; pass < 4; pass++) {
#pragma unroll
    for (int j = 0; j < 16; j++) {
      if (pass) {
        const uint32_t w15 = w[(j + 1) & 15], w2 = w[(j + 14) & 15];
        w[j] += (rotr(w15, 7) ^ rotr(w15, 18) ^ (w15 >> 3)) + w[(j + 9) & 15] + (rotr(w2, 17) ^ rotr(w2, 19) ^ (w2 >> 10));
      }
      const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + round_constant(16 * pass + j) + w[j];
      const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      hh = g;
      g = f;
      f = e;
      e = d + t1;
      d = c;
      c = b;
      b = a;
      a = t1 + t2;
    }
  }
  h[0] += a;
  h[1] += b;
  h[2] += c;
  h[3] += d;
  h[4] += e;
  h[5] += f;
  h[6] += g;
  h[7] += hh;
}

// One-shot digest of the len bytes at(0) .. at(len - 1), any length: the padded message is taken 64 bytes at a time.
template <class ByteAt>
ZK_HD void digest_of(ByteAt at, uint32_t len, uint32_t (&out)[8]) {
  initial_state(out);
  const uint32_t blocks = (len + 8) / 64 + 1;   // 0x80 and the 8-byte bit count have to fit
#pragma unroll 1
  for (uint32_t blk = 0; blk < blocks; blk++) {
    uint32_t m[16];
#pragma unroll
    for (int w = 0; w < 16; w++) {
      uint32_t word = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t j = 64 * blk + 4 * w + k;
        const uint32_t byte = j < len ? at(j) : (j == len ? 0x80u : 0u);
        word |= byte << (24 - 8 * k);
      }
      m[w] = word;
    }
    if (blk + 1 == blocks) {
      m[14] = len >> 29;
      m[15] = len << 3;
    }
    compress(out, m);
  }
}
ZK_HD void digest(const uint8_t* msg, uint32_t len, uint32_t (&out)[8]) {
  digest_of([msg](uint32_t j) -> uint32_t { return msg[j]; }, len, out);
}

// HMAC-SHA256 with a 32-byte key (so the key block is the key and 32 pad bytes, never a hash of the key). The message
// comes as the words of its one or two blocks, ALREADY padded for a hash that has taken the 64-byte key block before it
// (the bit count in the last word is 8 * (64 + message bytes)): pad_32 / pad_33 / pad_97 below build the three shapes
// RFC 6979 needs. two_blocks must be the same in every lane.
//   phase 0: (key ^ ipad) block     1: m0     2: m1 (two_blocks only)     3: (key ^ opad) block     4: the inner digest
ZK_HD void hmac32(const uint32_t (&key)[8], const uint32_t (&m0)[16], const uint32_t (&m1)[16], bool two_blocks, uint32_t (&out)[8]) {
  uint32_t st[8], inner[8];
#pragma unroll
  for (int i = 0; i < 8; i++) st[i] = inner[i] = 0;
#pragma unroll 1
  for (int phase = 0; phase < 5; phase++) {
    if (phase == 2 && !two_blocks) continue;
    uint32_t blk[16];
    if (phase == 0 || phase == 3) {
      const uint32_t pad = phase == 0 ? 0x36363636u : 0x5c5c5c5cu;
#pragma unroll
      for (int i = 0; i < 8; i++) {
        blk[i] = key[i] ^ pad;
        blk[8 + i] = pad;
        inner[i] = st[i];
      }
      initial_state(st);
    } else if (phase == 4) {
#pragma unroll
      for (int i = 0; i < 8; i++) {
        blk[i] = inner[i];
        blk[8 + i] = 0;
      }
      blk[8] = 0x80000000u;
      blk[15] = 8 * (64 + 32);
    } else {
#pragma unroll
      for (int i = 0; i < 16; i++) blk[i] = phase == 1 ? m0[i] : m1[i];
    }
    compress(st, blk);
  }
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = st[i];
}

// the padded message blocks of hmac32 for a 32-byte message v
ZK_HD void pad_32(const uint32_t (&v)[8], uint32_t (&m0)[16]) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    m0[i] = v[i];
    m0[8 + i] = 0;
  }
  m0[8] = 0x80000000u;
  m0[15] = 8 * (64 + 32);
}
// ... for the 33 bytes v || tag
ZK_HD void pad_33(const uint32_t (&v)[8], uint32_t tag, uint32_t (&m0)[16]) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    m0[i] = v[i];
    m0[8 + i] = 0;
  }
  m0[8] = (tag << 24) | 0x00800000u;
  m0[15] = 8 * (64 + 33);
}
// ... for the 97 bytes v || tag || x || h: x and h stand one byte off the word grid
ZK_HD void pad_97(const uint32_t (&v)[8], uint32_t tag, const uint32_t (&x)[8], const uint32_t (&h)[8], uint32_t (&m0)[16],
                  uint32_t (&m1)[16]) {
  uint32_t prev = tag;
#pragma unroll
  for (int i = 0; i < 8; i++) m0[i] = v[i];
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const uint32_t cur = i < 8 ? x[i] : h[i - 8];
    const uint32_t word = (prev << 24) | (cur >> 8);
    if (i < 8) m0[8 + i] = word;
    else m1[i - 8] = word;
    prev = cur;
  }
  m1[8] = (prev << 24) | 0x00800000u;
#pragma unroll
  for (int i = 9; i < 15; i++) m1[i] = 0;
  m1[15] = 8 * (64 + 97);
}

}  // namespace sha256
}  // namespace zkpoa
