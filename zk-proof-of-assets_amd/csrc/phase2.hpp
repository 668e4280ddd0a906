// The phase-2 transcript of a .zkey (section 10), host side, no GPU: what `snarkjs zkey new / contribute / beacon / verify`
// hash and draw, written from DESIGN.md "Phase-2 transcript" (snarkjs and ffjavascript are not vendored anywhere near
// this project; the layout is restated from their published sources). Blake2b-512 (RFC 7693), SHA-256 (FIPS 180-4),
// the ChaCha20 generator of ffjavascript, square roots in Fq and Fq2, `fromRng` for Fr, G1 and G2, hash-to-G2 of a
// transcript hash, the beacon's key derivation, the hash form of a point, the type and params that end a record of either transcript
// (RecordParams) and the records of section 10.
#pragma once
#include "host_curve.hpp"
#include "pairing.hpp"

#include <stdint.h>
#include <string.h>

#include <stdexcept>
#include <string>
#include <vector>

namespace zkpoa {
namespace phase2 {

// ---- Blake2b-512, unkeyed (RFC 7693) ------------------------------------------------------------------------------------
struct Blake2b {
  uint64_t h[8], t[2] = {0, 0};
  uint8_t buf[128];
  size_t fill = 0;
  static constexpr uint64_t kIv[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull,
                                      0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
                                      0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
  Blake2b() {
    for (int i = 0; i < 8; i++) h[i] = kIv[i];
    h[0] ^= 0x01010040ull;   // digest length 64, no key, fanout 1, depth 1
  }
  static uint64_t rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }
  void compress(const uint8_t* block, bool last) {
    static const uint8_t kSigma[12][16] = {
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
        {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
        {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
        {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
        {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};
    uint64_t m[16], v[16];
    memcpy(m, block, 128);   // little-endian host
    for (int i = 0; i < 8; i++) {
      v[i] = h[i];
      v[i + 8] = kIv[i];
    }
    v[12] ^= t[0];
    v[13] ^= t[1];
    if (last) v[14] = ~v[14];
#define ZKPOA_B2B_G(a, b, c, d, x, y)     \
  v[a] = v[a] + v[b] + (x);               \
  v[d] = rotr(v[d] ^ v[a], 32);           \
  v[c] = v[c] + v[d];                     \
  v[b] = rotr(v[b] ^ v[c], 24);           \
  v[a] = v[a] + v[b] + (y);               \
  v[d] = rotr(v[d] ^ v[a], 16);           \
  v[c] = v[c] + v[d];                     \
  v[b] = rotr(v[b] ^ v[c], 63);
    for (int r = 0; r < 12; r++) {
      const uint8_t* s = kSigma[r];
      ZKPOA_B2B_G(0, 4, 8, 12, m[s[0]], m[s[1]])
      ZKPOA_B2B_G(1, 5, 9, 13, m[s[2]], m[s[3]])
      ZKPOA_B2B_G(2, 6, 10, 14, m[s[4]], m[s[5]])
      ZKPOA_B2B_G(3, 7, 11, 15, m[s[6]], m[s[7]])
      ZKPOA_B2B_G(0, 5, 10, 15, m[s[8]], m[s[9]])
      ZKPOA_B2B_G(1, 6, 11, 12, m[s[10]], m[s[11]])
      ZKPOA_B2B_G(2, 7, 8, 13, m[s[12]], m[s[13]])
      ZKPOA_B2B_G(3, 4, 9, 14, m[s[14]], m[s[15]])
    }
#undef ZKPOA_B2B_G
    for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[i + 8];
  }
  void count(uint64_t n) {
    t[0] += n;
    if (t[0] < n) t[1]++;
  }
  // the last block is held back until final() (it is compressed with the "last" flag, also when it is full)
  void update(const void* data, size_t len) {
    const uint8_t* p = static_cast<const uint8_t*>(data);
    while (len) {
      if (fill == 128) {
        count(128);
        compress(buf, false);
        fill = 0;
      }
      if (fill == 0 && len > 128) {   // whole blocks straight from the input, all but the last
        const size_t blocks = (len - 1) / 128;
        for (size_t b = 0; b < blocks; b++) {
          count(128);
          compress(p + 128 * b, false);
        }
        p += 128 * blocks;
        len -= 128 * blocks;
      }
      const size_t take = len < 128 - fill ? len : 128 - fill;
      memcpy(buf + fill, p, take);
      fill += take;
      p += take;
      len -= take;
    }
  }
  void update_u32_be(uint32_t v) {
    const uint8_t b[4] = {(uint8_t)(v >> 24), (uint8_t)(v >> 16), (uint8_t)(v >> 8), (uint8_t)v};
    update(b, 4);
  }
  void final(uint8_t out[64]) {
    count(fill);
    memset(buf + fill, 0, 128 - fill);
    compress(buf, true);
    memcpy(out, h, 64);
  }
};

inline void blake2b512(const void* data, size_t len, uint8_t out[64]) {
  Blake2b b;
  b.update(data, len);
  b.final(out);
}

// ---- SHA-256 (FIPS 180-4) ----------------------------------------------------------------------------------------------
inline void sha256(const void* data, size_t len, uint8_t out[32]) {
  static const uint32_t k[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
      0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
      0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
      0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
      0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
      0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
      0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  auto rotr = [](uint32_t x, int n) { return (x >> n) | (x << (32 - n)); };
  auto block = [&](const uint8_t* p) {
    uint32_t w[64];
    for (int i = 0; i < 16; i++) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
    for (int i = 16; i < 64; i++) {
      const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
      const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; i++) {
      const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + k[i] + w[i];
      const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
  };
  const uint8_t* p = static_cast<const uint8_t*>(data);
  size_t left = len;
  for (; left >= 64; left -= 64, p += 64) block(p);
  uint8_t tail[128] = {0};
  memcpy(tail, p, left);
  tail[left] = 0x80;
  const size_t tl = left + 9 <= 64 ? 64 : 128;
  const uint64_t bits = (uint64_t)len * 8;
  for (int i = 0; i < 8; i++) tail[tl - 1 - i] = (uint8_t)(bits >> (8 * i));
  block(tail);
  if (tl == 128) block(tail + 64);
  for (int i = 0; i < 8; i++)
    for (int j = 0; j < 4; j++) out[4 * i + j] = (uint8_t)(h[i] >> (24 - 8 * j));
}

// ---- ffjavascript's ChaCha generator: ChaCha20 blocks, key = eight u32 words, 64-bit block counter in words 12-13, zero
// nonce in words 14-15; the 16 words of a block are handed out in order ----------------------------------------------------
struct ChaCha {
  uint32_t state[16], buff[16];
  int idx = 16;
  explicit ChaCha(const uint32_t key[8]) {
    state[0] = 0x61707865; state[1] = 0x3320646e; state[2] = 0x79622d32; state[3] = 0x6b206574;
    for (int i = 0; i < 8; i++) state[4 + i] = key[i];
    for (int i = 12; i < 16; i++) state[i] = 0;
  }
  static uint32_t rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }
  static void qr(uint32_t* s, int a, int b, int c, int d) {
    s[a] += s[b]; s[d] = rotl(s[d] ^ s[a], 16);
    s[c] += s[d]; s[b] = rotl(s[b] ^ s[c], 12);
    s[a] += s[b]; s[d] = rotl(s[d] ^ s[a], 8);
    s[c] += s[d]; s[b] = rotl(s[b] ^ s[c], 7);
  }
  void refill() {
    memcpy(buff, state, 64);
    for (int i = 0; i < 10; i++) {
      qr(buff, 0, 4, 8, 12); qr(buff, 1, 5, 9, 13); qr(buff, 2, 6, 10, 14); qr(buff, 3, 7, 11, 15);
      qr(buff, 0, 5, 10, 15); qr(buff, 1, 6, 11, 12); qr(buff, 2, 7, 8, 13); qr(buff, 3, 4, 9, 14);
    }
    for (int i = 0; i < 16; i++) buff[i] += state[i];
    idx = 0;
    if (++state[12] == 0) ++state[13];
  }
  uint32_t next_u32() {
    if (idx == 16) refill();
    return buff[idx++];
  }
  uint64_t next_u64() {   // high word first
    const uint64_t hi = next_u32();
    return hi << 32 | next_u32();
  }
  bool next_bool() { return (next_u32() & 1u) == 1u; }
};

// ---- square roots ------------------------------------------------------------------------------------------------------
// q = 3 mod 4: a^((q + 1) / 4) is a root when there is one. Montgomery form in and out.
inline bool fq_sqrt(const HFq& a, HFq* root) {
  static const uint64_t e[4] = {0x4f082305b61f3f52ull, 0x65e05aa45a1c72a3ull, 0x6e14116da0605617ull, 0x0c19139cb84c680aull};
  const HFq r = a.pow(e);
  if (r.sqr() != a) return false;
  *root = r;
  return true;
}
// a = a0 + a1 u is a square iff its norm is one in Fq; then c0^2 = (a0 +- sqrt(norm)) / 2, c1 = a1 / (2 c0)
inline bool fq2_sqrt(const HFq2& a, HFq2* root) {
  if (a.c1.is_zero()) {
    HFq r;
    if (fq_sqrt(a.c0, &r)) *root = HFq2{r, HFq::zero()};
    else if (fq_sqrt(a.c0.neg(), &r)) *root = HFq2{HFq::zero(), r};   // u^2 = -1
    else return false;
    return true;
  }
  HFq d, c0;
  if (!fq_sqrt(a.c0.sqr() + a.c1.sqr(), &d)) return false;
  const HFq half = HFq::from_u64(2).inv();
  if (!fq_sqrt((a.c0 + d) * half, &c0) && !fq_sqrt((a.c0 - d) * half, &c0)) return false;
  const HFq2 r{c0, a.c1 * c0.dbl().inv()};
  if (r.sqr() != a) return false;
  *root = r;
  return true;
}
// "negative": the standard-form value is above (q - 1) / 2; for Fq2 the sign of c1, of c0 when c1 = 0
inline bool fq_is_negative(const HFq& a) {
  static const uint64_t half[4] = {0x9e10460b6c3e7ea3ull, 0xcbc0b548b438e546ull, 0xdc2822db40c0ac2eull, 0x183227397098d014ull};
  const HFq s = a.from_mont();
  for (int i = 3; i >= 0; i--) {
    if (s.l[i] > half[i]) return true;
    if (s.l[i] < half[i]) return false;
  }
  return false;
}
inline bool fq2_is_negative(const HFq2& a) { return a.c1.is_zero() ? fq_is_negative(a.c0) : fq_is_negative(a.c1); }

// ---- fromRng -----------------------------------------------------------------------------------------------------------
// A field element: four u64 draws, the first the least significant, masked to 254 bits, redrawn while >= the modulus.
// The accepted integer v IS the element's Montgomery representation (the value is v / 2^256), as in ffjavascript's
// field over wasm, which writes v into the element's buffer.
template <class HF>
inline HF fp_from_rng(ChaCha& rng) {
  for (;;) {
    uint64_t v[4];
    for (int i = 0; i < 4; i++) v[i] = rng.next_u64();
    v[3] &= 0x3fffffffffffffffull;
    if (!HF::geq_p(v)) return HF{{v[0], v[1], v[2], v[3]}};
  }
}
inline HFq2 fq2_from_rng(ChaCha& rng) {
  const HFq c0 = fp_from_rng<HFq>(rng);
  return HFq2{c0, fp_from_rng<HFq>(rng)};
}
// a scalar in standard form, 32 B little-endian
inline void fr_from_rng(ChaCha& rng, uint8_t out_le[32]) {
  const HFr s = fp_from_rng<HFr>(rng).from_mont();
  memcpy(out_le, s.l, 32);
}
// A point: x from the generator, one bool ("the greater root"), both redrawn until x^3 + b is a square; y is the
// negative root exactly when the bool is set.
inline pairing::G1 g1_from_rng(ChaCha& rng) {
  for (;;) {
    const HFq x = fp_from_rng<HFq>(rng);
    const bool greatest = rng.next_bool();
    HFq y;
    if (!fq_sqrt(x.sqr() * x + HFq::from_u64(3), &y)) continue;
    if (greatest != fq_is_negative(y)) y = y.neg();
    return {x, y};
  }
}
// G2 also clears the cofactor 2q - r of the twist
inline pairing::G2 g2_from_rng(ChaCha& rng) {
  static const uint64_t kCofactor[4] = {0x345f2299c0f9fa8dull, 0x06ceecda572a2489ull, 0xb85045b68181585eull, 0x30644e72e131a029ull};
  for (;;) {
    const HFq2 x = fq2_from_rng(rng);
    const bool greatest = rng.next_bool();
    HFq2 y;
    if (!fq2_sqrt(x.sqr() * x + pairing::twist_b(), &y)) continue;
    if (greatest != fq2_is_negative(y)) y = y.neg();
    return h_to_affine(h_mul(XYZZ<HFq2>::from_affine(pairing::G2{x, y}), kCofactor));
  }
}
inline void key_from_be(const uint8_t* bytes32, uint32_t key[8]) {
  for (int i = 0; i < 8; i++)
    key[i] = (uint32_t)bytes32[4 * i] << 24 | (uint32_t)bytes32[4 * i + 1] << 16 | (uint32_t)bytes32[4 * i + 2] << 8 | bytes32[4 * i + 3];
}
inline pairing::G2 hash_to_g2(const uint8_t hash[64]) {
  uint32_t key[8];
  key_from_be(hash, key);
  ChaCha rng(key);
  return g2_from_rng(rng);
}
// the beacon: SHA-256 iterated 2^exp times over the beacon bytes; exp above kMaxBeaconExp (2^30 hashes, minutes) is refused
constexpr uint32_t kMaxBeaconExp = 30;
inline void beacon_key(const uint8_t* beacon, size_t len, uint32_t exp, uint32_t key[8]) {
  if (exp > kMaxBeaconExp) throw std::runtime_error("beacon: numIterationsExp above 30");
  uint8_t cur[32];
  sha256(beacon, len, cur);
  for (uint64_t i = 1; i < (1ull << exp); i++) sha256(cur, 32, cur);
  key_from_be(cur, key);
}

// ---- the hash form of a point: uncompressed, big-endian, standard form; an Fq2 coordinate is c1 then c0; infinity is
// 0x40 followed by zeros -------------------------------------------------------------------------------------------------
inline void fq_to_be(const HFq& a, uint8_t out[32]) {
  const HFq s = a.from_mont();
  for (int i = 0; i < 32; i++) out[i] = (uint8_t)(s.l[3 - i / 8] >> (56 - 8 * (i % 8)));
}
inline void g1_hash_form(const pairing::G1& p, uint8_t out[64]) {
  if (p.is_inf()) {
    memset(out, 0, 64);
    out[0] = 0x40;
    return;
  }
  fq_to_be(p.x, out);
  fq_to_be(p.y, out + 32);
}
inline void g2_hash_form(const pairing::G2& p, uint8_t out[128]) {
  if (p.is_inf()) {
    memset(out, 0, 128);
    out[0] = 0x40;
    return;
  }
  fq_to_be(p.x.c1, out);
  fq_to_be(p.x.c0, out + 32);
  fq_to_be(p.y.c1, out + 64);
  fq_to_be(p.y.c0, out + 96);
}
// The way back, for the handful of points of a key: hash form -> wire form. False for a coordinate not below q, a set bit
// 7 in the first byte, or 0x40 followed by anything but zeros; 0x40 then zeros is infinity, the all-zero point.
inline bool coords_from_hash_form(const uint8_t* in, int coords, const int* order, uint8_t* wire) {
  if (in[0] & 0x80) return false;
  if (in[0] == 0x40) {
    for (int i = 1; i < 32 * coords; i++)
      if (in[i]) return false;
    memset(wire, 0, 32 * coords);
    return true;
  }
  for (int c = 0; c < coords; c++) {
    uint64_t v[4] = {0, 0, 0, 0};
    for (int i = 0; i < 32; i++) v[3 - i / 8] |= (uint64_t)in[32 * c + i] << (56 - 8 * (i % 8));
    if (HFq::geq_p(v)) return false;
    HFq{{v[0], v[1], v[2], v[3]}}.to_mont().to_bytes(wire + 32 * order[c]);
  }
  return true;
}
inline bool g1_from_hash_form(const uint8_t in[64], uint8_t wire[64]) {
  static const int order[2] = {0, 1};
  return coords_from_hash_form(in, 2, order, wire);
}
inline bool g2_from_hash_form(const uint8_t in[128], uint8_t wire[128]) {
  static const int order[4] = {1, 0, 3, 2};   // c1 then c0 -> c0 then c1
  return coords_from_hash_form(in, 4, order, wire);
}
inline void hash_g1_wire(Blake2b& h, const uint8_t* wire) {
  uint8_t b[64];
  g1_hash_form(h_affine_from_bytes<HFq>(wire), b);
  h.update(b, 64);
}
inline void hash_g2_wire(Blake2b& h, const uint8_t* wire) {
  uint8_t b[128];
  g2_hash_form(h_affine_from_bytes<HFq2>(wire), b);
  h.update(b, 128);
}

// k * P on wire-form bytes (k: 32 B little-endian standard form); out may be in
template <class HF>
inline void mul_wire(const uint8_t* in, const uint8_t k_le[32], uint8_t* out) {
  uint64_t kv[4];
  memcpy(kv, k_le, 32);
  h_affine_to_bytes<HF>(h_to_affine(h_mul(XYZZ<HF>::from_affine(h_affine_from_bytes<HF>(in)), kv)), out);
}
// what a beacon's generator yields per secret: the secret (fromRng Fr, standard form), then g1_s (fromRng G1, wire form)
inline void beacon_draw(ChaCha& rng, uint8_t x[32], uint8_t g1_s[64]) {
  fr_from_rng(rng, x);
  h_affine_to_bytes<HFq>(g1_from_rng(rng), g1_s);
}

// ---- what a record of a .ptau's section 7 and of a .zkey's section 10 ends with: u32 type, u32 length of the params, the
// params: tag 1 = name (u8 length, bytes); tag 2 = numIterationsExp (one byte, no length); tag 3 = beacon (u8 length, bytes)
struct RecordParams {
  uint32_t type = 0;   // 0 contribution, 1 beacon
  std::string name;
  std::vector<uint8_t> beacon;
  uint32_t num_iterations_exp = 0;
  // what a command may append: throws "<command>: ..." for a name or beacon that has no u8 length, or a beacon that
  // would not finish
  void check(const char* command) const {
    if (num_iterations_exp > kMaxBeaconExp)
      throw std::runtime_error(std::string(command) + ": numIterationsExp above 30 is refused (2^30 hashes take minutes; more would not finish)");
    if (name.size() > 255 || beacon.size() > 255) throw std::runtime_error(std::string(command) + ": name or beacon longer than 255 bytes");
  }
  size_t len() const {   // of what write() appends
    return 8 + (name.empty() ? 0 : 2 + name.size()) + (type == 1 ? 2 + 2 + beacon.size() : 0);
  }
  void write(std::vector<uint8_t>& out) const {
    const uint32_t head[2] = {type, (uint32_t)(len() - 8)};
    out.insert(out.end(), (const uint8_t*)head, (const uint8_t*)head + 8);
    if (!name.empty()) {
      out.push_back(1);
      out.push_back((uint8_t)name.size());
      out.insert(out.end(), name.begin(), name.end());
    }
    if (type == 1) {
      out.push_back(2);
      out.push_back((uint8_t)num_iterations_exp);
      out.push_back(3);
      out.push_back((uint8_t)beacon.size());
      out.insert(out.end(), beacon.begin(), beacon.end());
    }
  }
  // from the `avail` bytes at p; returns the bytes taken, throws `what` for a type above 1, an unknown tag or anything
  // that runs past avail
  uint64_t parse(const uint8_t* p, uint64_t avail, const char* what) {
    auto fail = [&] { throw std::runtime_error(what); };
    uint32_t plen;
    if (avail < 8) fail();
    memcpy(&type, p, 4);
    memcpy(&plen, p + 4, 4);
    if (avail - 8 < plen || type > 1) fail();
    const uint8_t* q = p + 8;
    for (uint32_t i = 0; i < plen;) {
      const uint8_t tag = q[i++];
      if (tag == 2) {
        if (i >= plen) fail();
        num_iterations_exp = q[i++];
      } else if (tag == 1 || tag == 3) {
        if (i >= plen || plen - i - 1 < q[i]) fail();
        const uint8_t l = q[i++];
        if (tag == 1) name.assign((const char*)q + i, l);
        else beacon.assign(q + i, q + i + l);
        i += l;
      } else fail();
    }
    return 8 + (uint64_t)plen;
  }
};

// ---- section 10 --------------------------------------------------------------------------------------------------------
struct Record : RecordParams {
  uint8_t delta_after[64], g1_s[64], g1_sx[64], g2_spx[128], transcript[64];   // points in zkey wire form
  void hash_pubkey(Blake2b& h) const {
    hash_g1_wire(h, delta_after);
    hash_g1_wire(h, g1_s);
    hash_g1_wire(h, g1_sx);
    hash_g2_wire(h, g2_spx);
    h.update(transcript, 64);
  }
};
struct Transcript {
  uint8_t cs_hash[64];
  std::vector<Record> records;
  bool present() const {
    for (int i = 0; i < 64; i++)
      if (cs_hash[i]) return true;
    return false;
  }
};
inline Transcript parse_section10(const uint8_t* p, uint64_t len) {
  const char* const what = "zkey: section 10 is truncated or over-long";
  if (len < 68) throw std::runtime_error(what);
  Transcript t;
  memcpy(t.cs_hash, p, 64);
  uint32_t count;
  memcpy(&count, p + 64, 4);
  uint64_t at = 68;
  for (uint32_t k = 0; k < count; k++) {
    if (len - at < 384) throw std::runtime_error(what);
    Record r;
    memcpy(r.delta_after, p + at, 64);
    memcpy(r.g1_s, p + at + 64, 64);
    memcpy(r.g1_sx, p + at + 128, 64);
    memcpy(r.g2_spx, p + at + 192, 128);
    memcpy(r.transcript, p + at + 320, 64);
    at += 384;
    at += r.parse(p + at, len - at, what);
    t.records.push_back(r);
  }
  if (at != len) throw std::runtime_error(what);
  return t;
}
inline std::vector<uint8_t> write_section10(const Transcript& t) {
  std::vector<uint8_t> out(t.cs_hash, t.cs_hash + 64);
  const uint32_t count = (uint32_t)t.records.size();
  out.insert(out.end(), (const uint8_t*)&count, (const uint8_t*)&count + 4);
  for (const Record& r : t.records) {
    out.insert(out.end(), r.delta_after, r.delta_after + 64);
    out.insert(out.end(), r.g1_s, r.g1_s + 64);
    out.insert(out.end(), r.g1_sx, r.g1_sx + 64);
    out.insert(out.end(), r.g2_spx, r.g2_spx + 128);
    out.insert(out.end(), r.transcript, r.transcript + 64);
    r.write(out);
  }
  return out;
}
// the transcript hash of the record that follows `earlier`: cs hash, the earlier records, then g1_s and g1_sx
inline void transcript_hash(const Transcript& t, size_t earlier, const uint8_t* g1_s, const uint8_t* g1_sx, uint8_t out[64]) {
  Blake2b h;
  h.update(t.cs_hash, 64);
  for (size_t i = 0; i < earlier; i++) t.records[i].hash_pubkey(h);
  hash_g1_wire(h, g1_s);
  hash_g1_wire(h, g1_sx);
  h.final(out);
}

}  // namespace phase2
}  // namespace zkpoa
