// SHA-512 and HMAC-SHA512 on the device and the host, one message per lane: the hash of BIP-32 (csrc/bip32.hip: the
// child-key step, the master key, PBKDF2 of BIP-39). Words are the big-endian 64-bit words of FIPS 180-4: word k of a
// message is its bytes 8k .. 8k+7, first byte highest.
//
// One compression is five passes of sixteen rounds, built as csrc/sha256.hip.h builds its four: the sixteen rounds of a
// pass are unrolled, so that the rolling schedule w[16] is only ever indexed by compile-time constants and stays in
// registers (32 of them); the five passes are NOT (#pragma unroll 1), and the round constant is read from a table by the
// pass index, which is the same in every lane. No inline assembly: the compiler turns a 64-bit rotate into a pair of
// v_alignbit_b32. Plain ZK_HD C++: the same text runs on the host.
//
// HMAC takes a key of any length (one above 128 bytes is hashed first) and is split in two: hmac_key() runs the two key
// blocks once and keeps the inner and the outer mid-state; a message then costs its own blocks and one outer block. All
// children of one BIP-32 parent share the key (the chain code), and all 2048 rounds of PBKDF2 share the password: with
// the mid-states a 37-byte or a 64-byte message costs two compressions where the plain HMAC costs four.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef ZK_HD
#define ZK_HD __host__ __device__ __forceinline__
#endif

namespace zkpoa {
namespace sha512 {

ZK_HD uint64_t rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

ZK_HD uint64_t round_constant(int i) {
  constexpr uint64_t k[80] = {
      0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull,
      0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull,
      0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull, 0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull,
      0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
      0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull, 0x983e5152ee66dfabull,
      0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
      0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull,
      0x53380d139d95b3dfull, 0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
      0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull,
      0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull, 0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull,
      0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull,
      0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
      0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull,
      0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull,
      0x113f9804bef90daeull, 0x1b710b35131c471bull, 0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull,
      0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
  return k[i];
}

ZK_HD void initial_state(uint64_t (&h)[8]) {
  h[0] = 0x6a09e667f3bcc908ull;
  h[1] = 0xbb67ae8584caa73bull;
  h[2] = 0x3c6ef372fe94f82bull;
  h[3] = 0xa54ff53a5f1d36f1ull;
  h[4] = 0x510e527fade682d1ull;
  h[5] = 0x9b05688c2b3e6c1full;
  h[6] = 0x1f83d9abfb41bd6bull;
  h[7] = 0x5be0cd19137e2179ull;
}

// h <- the compression of one 128-byte block (16 big-endian words) into h
ZK_HD void compress(uint64_t (&h)[8], const uint64_t (&block)[16]) {
  uint64_t w[16];
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = block[i];
  uint64_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll 1
  for (int pass = 0; pass < 5; pass++) {
#pragma unroll
    for (int j = 0; j < 16; j++) {
      if (pass) {
        const uint64_t w15 = w[(j + 1) & 15], w2 = w[(j + 14) & 15];
        w[j] += (rotr(w15, 1) ^ rotr(w15, 8) ^ (w15 >> 7)) + w[(j + 9) & 15] + (rotr(w2, 19) ^ rotr(w2, 61) ^ (w2 >> 6));
      }
      const uint64_t t1 = hh + (rotr(e, 14) ^ rotr(e, 18) ^ rotr(e, 41)) + ((e & f) ^ (~e & g)) + round_constant(16 * pass + j) + w[j];
      const uint64_t t2 = (rotr(a, 28) ^ rotr(a, 34) ^ rotr(a, 39)) + ((a & b) ^ (a & c) ^ (b & c));
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

// The len bytes at(0) .. at(len - 1), any length below 2^29, go into `st` 128 bytes at a time with the padding of a hash
// that has taken `before` bytes (a multiple of 128) already: 0x80, zeros, and the bit count of before + len in the last
// word (the word above it is zero at these lengths).
template <class ByteAt>
ZK_HD void absorb(uint64_t (&st)[8], ByteAt at, uint32_t len, uint32_t before) {
  const uint32_t blocks = (len + 16) / 128 + 1;   // 0x80 and the 16-byte bit count have to fit
#pragma unroll 1
  for (uint32_t blk = 0; blk < blocks; blk++) {
    uint64_t m[16];
#pragma unroll
    for (int w = 0; w < 16; w++) {
      uint64_t word = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const uint32_t j = 128 * blk + 8 * w + k;
        const uint64_t byte = j < len ? (uint64_t)(at(j) & 0xffu) : (j == len ? 0x80u : 0u);
        word |= byte << (56 - 8 * k);
      }
      m[w] = word;
    }
    if (blk + 1 == blocks) m[15] = (uint64_t)(before + len) << 3;
    compress(st, m);
  }
}

// one-shot digest
template <class ByteAt>
ZK_HD void digest_of(ByteAt at, uint32_t len, uint64_t (&out)[8]) {
  initial_state(out);
  absorb(out, at, len, 0);
}
ZK_HD void digest(const uint8_t* msg, uint32_t len, uint64_t (&out)[8]) {
  digest_of([msg](uint32_t j) -> uint32_t { return msg[j]; }, len, out);
}

// ---- HMAC ----------------------------------------------------------------------------------------------------------
// the state after the block (key ^ ipad) and after the block (key ^ opad)
struct HmacKey {
  uint64_t inner[8], outer[8];
};

template <class ByteAt>
ZK_HD void hmac_key_of(ByteAt at, uint32_t key_len, HmacKey& k) {
  uint64_t block[16], hashed[8];
  const bool is_long = key_len > 128;
  if (is_long) digest_of(at, key_len, hashed);
#pragma unroll
  for (int w = 0; w < 16; w++) {
    uint64_t word = 0;
    if (is_long) {
      word = w < 8 ? hashed[w] : 0;
    } else {
#pragma unroll
      for (int b = 0; b < 8; b++) {
        const uint32_t j = 8 * w + b;
        word |= (uint64_t)(j < key_len ? at(j) & 0xffu : 0u) << (56 - 8 * b);
      }
    }
    block[w] = word ^ 0x3636363636363636ull;
  }
  initial_state(k.inner);
  compress(k.inner, block);
#pragma unroll
  for (int w = 0; w < 16; w++) block[w] ^= 0x3636363636363636ull ^ 0x5c5c5c5c5c5c5c5cull;
  initial_state(k.outer);
  compress(k.outer, block);
}
ZK_HD void hmac_key(const uint8_t* key, uint32_t key_len, HmacKey& k) {
  hmac_key_of([key](uint32_t j) -> uint32_t { return key[j]; }, key_len, k);
}

// the outer hash: one block, the 64-byte inner digest after the 128-byte key block
ZK_HD void hmac_finish(const HmacKey& k, const uint64_t (&inner_digest)[8], uint64_t (&out)[8]) {
  uint64_t block[16];
#pragma unroll
  for (int w = 0; w < 16; w++) {
    block[w] = w < 8 ? inner_digest[w] : 0;
    out[w & 7] = k.outer[w & 7];
  }
  block[8] = 0x8000000000000000ull;
  block[15] = 8 * (128 + 64);
  compress(out, block);
}

// a message of any length
template <class ByteAt>
ZK_HD void hmac_of(const HmacKey& k, ByteAt at, uint32_t len, uint64_t (&out)[8]) {
  uint64_t st[8];
#pragma unroll
  for (int i = 0; i < 8; i++) st[i] = k.inner[i];
  absorb(st, at, len, 128);
  hmac_finish(k, st, out);
}

// A message of at most 111 bytes that the caller has laid out as its ONE padded block (0x80 after it, the bit count
// 8 * (128 + bytes) in word 15): two compressions. pad_64 is that block for a 64-byte message (PBKDF2's rounds).
ZK_HD void hmac_block(const HmacKey& k, const uint64_t (&m)[16], uint64_t (&out)[8]) {
  uint64_t st[8];
#pragma unroll
  for (int i = 0; i < 8; i++) st[i] = k.inner[i];
  compress(st, m);
  hmac_finish(k, st, out);
}
ZK_HD void pad_64(const uint64_t (&v)[8], uint64_t (&m)[16]) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    m[i] = v[i];
    m[8 + i] = 0;
  }
  m[8] = 0x8000000000000000ull;
  m[15] = 8 * (128 + 64);
}

}  // namespace sha512
}  // namespace zkpoa
