// secp256k1 on the device: the coordinate field, arithmetic modulo the group order, and ECDSA public-key recovery in
// the ECDSA* form of the reference's scripts/lib/ecdsa_star.ts (the first step of full_workflow.sh, :354-357).
//
// Fp, p = 2^256 - 2^32 - 977. 8 x u32 limbs, little-endian, plain (no Montgomery form), and CANONICAL: every value a
// function here returns is in [0, p). Fp<PRM> of bn254_field.hip.h keeps values lazily in [0, 2p), which needs
// 4p < 2^256; this prime leaves no such room, so there is no redundant range at all: add and sub correct by one
// conditional +-p, a product is the 16-limb schoolbook product folded twice with 2^256 = 2^32 + 977 (mod p) and
// corrected once. Because the range is canonical, is_zero() and == are plain comparisons, and the type has exactly the
// interface xyzz_add / xyzz_dbl / xyzz_add_affine of bn254_ec.hip.h ask of a field (zero, one, is_zero, +, -, *, sqr,
// dbl, neg): both curves have a = 0, those formulas never lean on the lazy range, so they are used as they are (complete
// for P + P, P - P and infinity on either side) and no group operation is written again here.
//
// Sc, integers modulo the group order n. n has no form that helps beyond being close to 2^256: a product is folded
// three times with 2^256 = c (mod n), c = 2^256 - n (129 bits), and corrected once. Canonical [0, n) as well.
//
// The last part is the other direction, signing (`ecdsa-sigs-parser sign`): RFC 6979 nonces over csrc/sha256.hip.h, a
// fixed-base multiplication by G from a shared table, and the ECDSA equation.
//
// Everything is __host__ __device__ plain C++ (the compiler turns a u32 x u32 + u64 into v_mad_u64_u32), so the same
// text runs in a CPU program against a big-integer model.
#pragma once
#include "bn254_ec.hip.h"
#include "keccak.hip.h"
#include "sha256.hip.h"

namespace zkpoa {
namespace secp {

struct Fp {
  uint32_t l[8];

  static ZK_HD Fp zero() { return {{0, 0, 0, 0, 0, 0, 0, 0}}; }
  static ZK_HD Fp one() { return {{1, 0, 0, 0, 0, 0, 0, 0}}; }
  static ZK_HD Fp small(uint32_t v) { return {{v, 0, 0, 0, 0, 0, 0, 0}}; }
  ZK_HD bool is_zero() const { return (l[0] | l[1] | l[2] | l[3] | l[4] | l[5] | l[6] | l[7]) == 0; }
  ZK_HD bool operator==(const Fp& o) const {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d |= l[i] ^ o.l[i];
    return d == 0;
  }
  ZK_HD bool is_odd() const { return l[0] & 1u; }
  // p = ffffffff ffffffff ffffffff ffffffff ffffffff ffffffff fffffffe fffffc2f
  ZK_HD bool ge_p() const {
    const uint32_t hi = l[2] & l[3] & l[4] & l[5] & l[6] & l[7];
    return hi == 0xffffffffu && (l[1] == 0xffffffffu || (l[1] == 0xfffffffeu && l[0] >= 0xfffffc2fu));
  }
  // += (2^32 + 977) * m modulo 2^256, m = 0 / 1: subtracts p from a value in [p, 2^256 + p) whose bit 256 was dropped
  ZK_HD void add_k(uint32_t m) {
    uint64_t c = (uint64_t)l[0] + 977u * m;
    l[0] = (uint32_t)c;
    c = (c >> 32) + l[1] + m;
    l[1] = (uint32_t)c;
#pragma unroll
    for (int i = 2; i < 8; i++) {
      c = (c >> 32) + l[i];
      l[i] = (uint32_t)c;
    }
  }
  ZK_HD Fp operator+(const Fp& o) const {
    Fp r;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      c += (uint64_t)l[i] + o.l[i];
      r.l[i] = (uint32_t)c;
      c >>= 32;
    }
    r.add_k((c != 0 || r.ge_p()) ? 1u : 0u);   // the sum is below 2p: one correction
    return r;
  }
  ZK_HD Fp operator-(const Fp& o) const {
    Fp r;
    uint64_t b = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint64_t d = (uint64_t)l[i] - o.l[i] - b;
      r.l[i] = (uint32_t)d;
      b = (d >> 32) & 1u;
    }
    // a borrow: + p, which modulo 2^256 is - (2^32 + 977)
    const uint32_t m = (uint32_t)b;
    uint64_t d = (uint64_t)r.l[0] - 977u * m;
    r.l[0] = (uint32_t)d;
    d = (uint64_t)r.l[1] - m - ((d >> 32) & 1u);
    r.l[1] = (uint32_t)d;
#pragma unroll
    for (int i = 2; i < 8; i++) {
      d = (uint64_t)r.l[i] - ((d >> 32) & 1u);
      r.l[i] = (uint32_t)d;
    }
    return r;
  }
  ZK_HD Fp neg() const { return zero() - *this; }
  ZK_HD Fp dbl() const { return *this + *this; }

  // t (16 limbs, below p^2) modulo p
  static ZK_HD Fp reduce512(const uint32_t (&t)[16]) {
    Fp r;
    // lo + hi * 977 ...
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      c += (uint64_t)t[8 + i] * 977u + t[i];
      r.l[i] = (uint32_t)c;
      c >>= 32;
    }
    uint64_t top = c;   // below 2^10
    // ... + hi * 2^32
    c = 0;
#pragma unroll
    for (int i = 1; i < 8; i++) {
      c += (uint64_t)r.l[i] + t[8 + i - 1];
      r.l[i] = (uint32_t)c;
      c >>= 32;
    }
    top += c + t[15];   // what stands above 2^256: below 2^32 + 2^11
    // second fold: top * (2^32 + 977), below 2^66
    const uint64_t m = top * 977u;
    c = (uint64_t)r.l[0] + (uint32_t)m;
    r.l[0] = (uint32_t)c;
    c = (c >> 32) + r.l[1] + (m >> 32) + (uint32_t)top;
    r.l[1] = (uint32_t)c;
    c = (c >> 32) + r.l[2] + (top >> 32);
    r.l[2] = (uint32_t)c;
#pragma unroll
    for (int i = 3; i < 8; i++) {
      c = (c >> 32) + r.l[i];
      r.l[i] = (uint32_t)c;
    }
    // a carry out of limb 7 leaves a value below 2^67 (+ 2^256): one more 2^32 + 977 and it is reduced. Without a
    // carry the value is below 2^256 < 2p: one conditional subtraction. The two cases exclude each other.
    r.add_k(((c >> 32) != 0 || r.ge_p()) ? 1u : 0u);
    return r;
  }
  ZK_HD Fp operator*(const Fp& o) const {
    uint32_t t[16];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      uint64_t c = 0;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        c += (uint64_t)l[i] * o.l[j] + (i ? t[i + j] : 0u);
        t[i + j] = (uint32_t)c;
        c >>= 32;
      }
      t[i + 8] = (uint32_t)c;
    }
    return reduce512(t);
  }
  // the off-diagonal products once, doubled, plus the diagonal: 36 multiplications instead of 64
  ZK_HD Fp sqr() const {
    uint32_t t[16];
#pragma unroll
    for (int i = 0; i < 16; i++) t[i] = 0;
#pragma unroll
    for (int i = 0; i < 7; i++) {
      uint64_t c = 0;
#pragma unroll
      for (int j = i + 1; j < 8; j++) {
        c += (uint64_t)l[i] * l[j] + t[i + j];
        t[i + j] = (uint32_t)c;
        c >>= 32;
      }
      t[i + 8] = (uint32_t)c;
    }
    uint32_t top = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const uint32_t nt = t[i] >> 31;
      t[i] = (t[i] << 1) | top;
      top = nt;
    }
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint64_t d = (uint64_t)l[i] * l[i];
      c += (uint64_t)t[2 * i] + (uint32_t)d;
      t[2 * i] = (uint32_t)c;
      c >>= 32;
      c += (uint64_t)t[2 * i + 1] + (d >> 32);
      t[2 * i + 1] = (uint32_t)c;
      c >>= 32;
    }
    return reduce512(t);
  }
  ZK_HD Fp sqrn(int n) const {
    Fp r = *this;
#pragma unroll 1
    for (int i = 0; i < n; i++) r = r.sqr();
    return r;
  }
  // One fixed addition chain for every lane, as fq_sqrt of csrc/ptau_response.hip: the exponents (p + 1) / 4 (square
  // root: the candidate, to be squared and compared by the caller) and p - 2 (inverse) share the run of 223 ones at
  // the top, 2^223 - 1, built from 2^k - 1 for k = 2, 3, 6, 9, 11, 22, 44, 88, 176, 220.
  //   (p + 1) / 4 = (2^223 - 1) 2^31 + (2^22 - 1) 2^8 + 0b00001100     253 squarings + 13 products
  //   p - 2       = (2^223 - 1) 2^33 + (2^22 - 1) 2^10 + 0b0000101101  255 squarings + 15 products
  template <bool kInverse>
  ZK_HD Fp pow_chain() const {
    const Fp& a = *this;
    const Fp x2 = a.sqr() * a;
    const Fp x3 = x2.sqr() * a;
    Fp t = x3.sqrn(3) * x3;       // x6
    t = t.sqrn(3) * x3;           // x9
    t = t.sqrn(2) * x2;           // x11
    const Fp x22 = t.sqrn(11) * t;
    const Fp x44 = x22.sqrn(22) * x22;
    t = x44.sqrn(44) * x44;       // x88
    t = t.sqrn(88) * t;           // x176
    t = t.sqrn(44) * x44;         // x220
    t = t.sqrn(3) * x3;           // x223
    t = t.sqrn(23) * x22;
    if (kInverse) {
      t = t.sqrn(5) * a;
      t = t.sqrn(3) * x2;
      return t.sqrn(2) * a;
    }
    t = t.sqrn(6) * x2;
    return t.sqrn(2);
  }
  ZK_HD Fp sqrt_candidate() const { return pow_chain<false>(); }
  ZK_HD Fp inv() const { return pow_chain<true>(); }   // 0 -> 0
};

// ---- integers modulo the group order ---------------------------------------------------------------------------------
// n = ffffffff ffffffff ffffffff fffffffe baaedce6 af48a03b bfd25e8c d0364141
struct Sc {
  uint32_t l[8];
  static ZK_HD uint32_t N(int i) {
    constexpr uint32_t n[8] = {0xd0364141u, 0xbfd25e8cu, 0xaf48a03bu, 0xbaaedce6u, 0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    return n[i];
  }
  static ZK_HD uint32_t C(int i) {   // 2^256 - n
    constexpr uint32_t c[5] = {0x2fc9bebfu, 0x402da173u, 0x50b75fc4u, 0x45512319u, 0x1u};
    return c[i];
  }
  static ZK_HD Sc one() { return {{1, 0, 0, 0, 0, 0, 0, 0}}; }
  ZK_HD bool is_zero() const { return (l[0] | l[1] | l[2] | l[3] | l[4] | l[5] | l[6] | l[7]) == 0; }
  // *this - bound as 256-bit integers: the borrow (1: *this < bound)
  template <class Fn>
  ZK_HD uint32_t borrow_of(Fn bound) const {
    uint64_t b = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) b = (((uint64_t)l[i] - bound(i) - b) >> 32) & 1u;
    return (uint32_t)b;
  }
  ZK_HD bool ge_n() const { return borrow_of([](int i) { return N(i); }) == 0; }
  // above (n - 1) / 2 = 7fffffff ffffffff ffffffff ffffffff 5d576e73 57a4501d dfe92f46 681b20a0
  ZK_HD bool is_high() const {
    return borrow_of([](int i) {
             constexpr uint32_t h[8] = {0x681b20a1u, 0xdfe92f46u, 0x57a4501du, 0x5d576e73u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x7fffffffu};
             return h[i];
           }) == 0;
  }
  ZK_HD void add_c(uint32_t m) {   // += (2^256 - n) * m modulo 2^256
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      c += (uint64_t)l[i] + (i < 5 ? C(i) * m : 0u);
      l[i] = (uint32_t)c;
      c >>= 32;
    }
  }
  ZK_HD Sc reduce_once() const {   // a 256-bit integer -> [0, n): 2^256 < 2n
    Sc r = *this;
    r.add_c(ge_n() ? 1u : 0u);
    return r;
  }
  ZK_HD Sc neg() const {   // n - a, 0 -> 0
    Sc r;
    uint64_t b = 0;
    const uint32_t keep = is_zero() ? 0u : 0xffffffffu;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint64_t d = (uint64_t)N(i) - l[i] - b;
      r.l[i] = (uint32_t)d & keep;
      b = (d >> 32) & 1u;
    }
    return r;
  }
  // out (NOUT limbs) = lo (8 limbs, the rest zero) + hi (NH limbs) * (2^256 - n)
  template <int NH, int NOUT>
  static ZK_HD void fold(const uint32_t* lo, const uint32_t* hi, uint32_t* out) {
#pragma unroll
    for (int i = 0; i < NOUT; i++) out[i] = i < 8 ? lo[i] : 0u;
#pragma unroll
    for (int i = 0; i < NH; i++) {
      uint64_t c = 0;
#pragma unroll
      for (int j = 0; j < 5; j++) {
        c += (uint64_t)hi[i] * C(j) + out[i + j];
        out[i + j] = (uint32_t)c;
        c >>= 32;
      }
#pragma unroll
      for (int k = i + 5; k < NOUT; k++) {
        c += out[k];
        out[k] = (uint32_t)c;
        c >>= 32;
      }
    }
  }
  ZK_HD Sc operator*(const Sc& o) const {
    uint32_t t[16];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      uint64_t c = 0;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        c += (uint64_t)l[i] * o.l[j] + (i ? t[i + j] : 0u);
        t[i + j] = (uint32_t)c;
        c >>= 32;
      }
      t[i + 8] = (uint32_t)c;
    }
    // t < 2^512 -> w1 < 2^386 -> w2 < 2^259 -> w3 < 2^256 + 2^132
    uint32_t w1[14], w2[12], w3[9];
    fold<8, 14>(t, t + 8, w1);
    fold<6, 12>(w1, w1 + 8, w2);
    fold<1, 9>(w2, w2 + 8, w3);
    Sc r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = w3[i];
    // as in Fp::reduce512: a carry leaves a small value that one more c reduces, else one conditional subtraction
    r.add_c((w3[8] != 0 || r.ge_n()) ? 1u : 0u);
    return r;
  }
  ZK_HD Sc sqrn(int k) const {
    Sc r = *this;
#pragma unroll 1
    for (int i = 0; i < k; i++) r = r * r;
    return r;
  }
  // a^(n - 2): n - 2 = (2^127 - 1) 2^129 + (its low 128 bits, bit 128 being 0). The run of 127 ones by a chain
  // (2^k - 1 for k = 2, 3, 6, 12, 24, 48, 96, 120, 126, 127), the low 128 bits by square-and-multiply: the exponent is
  // the same in every lane, so the branch on its bits is uniform. 256 squarings + 78 products. 0 -> 0.
  ZK_HD Sc inv() const {
    const Sc& a = *this;
    const Sc x2 = (a * a) * a;
    const Sc x3 = (x2 * x2) * a;
    const Sc x6 = x3.sqrn(3) * x3;
    Sc t = x6.sqrn(6) * x6;       // x12
    const Sc x24 = t.sqrn(12) * t;
    t = x24.sqrn(24) * x24;       // x48
    t = t.sqrn(48) * t;           // x96
    t = t.sqrn(24) * x24;         // x120
    t = t.sqrn(6) * x6;           // x126
    t = (t * t) * a;              // x127
    t = t * t;                    // bit 128 of n - 2 is 0
#pragma unroll 1
    for (int w = 3; w >= 0; w--) {
      uint32_t bits = w == 3 ? 0xbaaedce6u : w == 2 ? 0xaf48a03bu : w == 1 ? 0xbfd25e8cu : 0xd036413fu;
#pragma unroll 1
      for (int b = 0; b < 32; b++) {
        t = t * t;
        if (bits >> 31) t = t * a;
        bits <<= 1;
      }
    }
    return t;
  }
};

typedef Affine<Fp> AffineK;
typedef XYZZ<Fp> XyzzK;

ZK_HD AffineK generator() {
  return {{{0x16f81798u, 0x59f2815bu, 0x2dce28d9u, 0x029bfcdbu, 0xce870b07u, 0x55a06295u, 0xf9dcbbacu, 0x79be667eu}},
          {{0xfb10d4b8u, 0x9c47d08fu, 0xa6855419u, 0xfd17b448u, 0x0e1108a8u, 0x5da4fbfcu, 0x26a3c465u, 0x483ada77u}}};
}

// x = X / ZZ, y = Y / ZZZ with one inversion: 1 / ZZ = (ZZ / ZZZ)^2 because ZZ^3 = ZZZ^2. p must not be infinity.
ZK_HD AffineK to_affine(const XyzzK& p) {
  const Fp i3 = p.zzz.inv();
  const Fp iz = p.zz * i3;
  return {p.x * iz.sqr(), p.y * i3};
}

// ---- byte order ----------------------------------------------------------------------------------------------------
// The 32-byte integers of the ECDSA* entry points are big-endian, as the hex strings of the signature files spell them
// and as Keccak takes the public key. Word loads: every array is 4-byte aligned at any index (32, 64 and 20 bytes).
ZK_HD uint32_t bswap32(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }
ZK_HD void load_be32(const void* base, uint64_t idx, uint32_t (&l)[8]) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(base) + 8 * idx;
#pragma unroll
  for (int i = 0; i < 8; i++) l[7 - i] = bswap32(w[i]);
}
ZK_HD void store_be32(void* base, uint64_t idx, const uint32_t (&l)[8]) {
  uint32_t* w = reinterpret_cast<uint32_t*>(base) + 8 * idx;
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = bswap32(l[7 - i]);
}
// what lane t of the recovery, signing and public-key kernels ends with: its key, address words and status
ZK_HD void store_key_outputs(uint64_t t, const AffineK& q, const uint32_t (&addr)[5], uint32_t status, void* out_pubkey,
                             uint32_t* out_address, uint8_t* out_status) {
  store_be32(out_pubkey, 2 * t, q.x.l);
  store_be32(out_pubkey, 2 * t + 1, q.y.l);
#pragma unroll
  for (int i = 0; i < 5; i++) out_address[5 * t + i] = addr[i];
  out_status[t] = (uint8_t)status;
}

// ---- the Ethereum address of a public key --------------------------------------------------------------------------
// Keccak-256 of the 64 bytes x || y (big-endian), last 20 bytes: as five words in memory order (word k = bytes 4k..)
ZK_HD void eth_address_words(const AffineK& q, uint32_t (&addr)[5]) {
  uint64_t a[25];
#pragma unroll
  for (int i = 0; i < 25; i++) a[i] = 0;
#pragma unroll
  for (int w = 0; w < 4; w++) {   // message word w = bytes 8w .. 8w+7, little-endian in the state
    a[w] = (uint64_t)bswap32(q.x.l[7 - 2 * w]) | ((uint64_t)bswap32(q.x.l[6 - 2 * w]) << 32);
    a[4 + w] = (uint64_t)bswap32(q.y.l[7 - 2 * w]) | ((uint64_t)bswap32(q.y.l[6 - 2 * w]) << 32);
  }
  a[8] ^= 0x01;                     // pad10*1 of the Keccak submission (SHA-3 would be 0x06)
  a[16] ^= 0x8000000000000000ull;   // byte 135
  keccak::f1600(a);
  addr[0] = (uint32_t)(a[1] >> 32);   // digest bytes 12..15
  addr[1] = (uint32_t)a[2];
  addr[2] = (uint32_t)(a[2] >> 32);
  addr[3] = (uint32_t)a[3];
  addr[4] = (uint32_t)(a[3] >> 32);
}

// EIP-55: Keccak-256 of the 40 lower-case hex characters of the address; hex digit i is written in upper case when it
// is a letter and nibble i of that digest is 8 or more. Writes "0x" + 40 characters, no terminator.
ZK_HD uint32_t hex_char(uint32_t nib) { return nib < 10 ? '0' + nib : 'a' + (nib - 10); }
ZK_HD void eip55_text(const uint32_t (&addr)[5], uint8_t* out42) {
  uint64_t a[25];
#pragma unroll
  for (int i = 0; i < 25; i++) a[i] = 0;
#pragma unroll
  for (int w = 0; w < 5; w++) {   // four address bytes = eight characters = one message word
    uint64_t m = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const uint32_t byte = (addr[w] >> (8 * b)) & 0xffu;
      m |= (uint64_t)hex_char(byte >> 4) << (16 * b);
      m |= (uint64_t)hex_char(byte & 15u) << (16 * b + 8);
    }
    a[w] = m;
  }
  a[5] ^= 0x01;
  a[16] ^= 0x8000000000000000ull;
  keccak::f1600(a);
  out42[0] = '0';
  out42[1] = 'x';
#pragma unroll
  for (int i = 0; i < 40; i++) {
    const uint32_t byte = (addr[i / 8] >> (8 * ((i / 2) % 4))) & 0xffu;
    const uint32_t nib = (i & 1) ? (byte & 15u) : (byte >> 4);
    const uint32_t hbyte = (uint32_t)(a[i / 16] >> (8 * ((i / 2) % 8))) & 0xffu;
    const uint32_t hn = (i & 1) ? (hbyte & 15u) : (hbyte >> 4);
    uint32_t ch = hex_char(nib);
    if (nib >= 10 && hn >= 8) ch -= 32;
    out42[i + 2] = (uint8_t)ch;
  }
}

// ---- recovery ------------------------------------------------------------------------------------------------------
enum Status : uint8_t {
  kOk = 0,
  kBadV = 1,          // v is not 27 or 28 (ecdsa_star.ts:86-88)
  kBadScalar = 2,     // r or s is zero or not below n
  kHighS = 3,         // s >= 2^255: ethers' "non-canonical s"
  kNotOnCurve = 4,    // r^3 + 7 is not a square
  kInfinity = 5,      // the recovered key is the point at infinity (s R = z G)
  kAddress = 6,       // the derived address differs from the one given
};

// signed digits d_i in [-7, 8], k = sum d_i 16^i, of k <= (n - 1) / 2 < 2^255 (no carry out of the top digit):
// magnitudes packed as nibbles, signs as a bit mask -- the recoding of ec_mul_windowed (csrc/ec_ntt.hip.h)
ZK_HD void recode_signed4(const uint32_t (&k)[8], uint32_t (&mag)[8], uint64_t& sgn) {
  sgn = 0;
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
}

// The multiples 1R .. 8R of one lane's base live in global memory, never in a private array: an array indexed by a
// run-time digit cannot stay in registers, and ec_mul_windowed's copy of this table is what puts 1 KiB per lane of
// that kernel into scratch. Word w of entry m of lane t is tab[(32 m + w) * stride + t]: the lanes of a wave read
// and write consecutive words. Only the lane itself touches its column, so no synchronisation is needed.
struct LaneTable {
  uint32_t* tab;
  uint64_t stride;
  ZK_HD void put(int m, const XyzzK& p) const {
    uint32_t* q = tab + (uint64_t)(32 * m) * stride;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      q[(uint64_t)i * stride] = p.x.l[i];
      q[(uint64_t)(8 + i) * stride] = p.y.l[i];
      q[(uint64_t)(16 + i) * stride] = p.zz.l[i];
      q[(uint64_t)(24 + i) * stride] = p.zzz.l[i];
    }
  }
  ZK_HD XyzzK get(uint32_t m) const {
    const uint32_t* q = tab + (uint64_t)(32 * m) * stride;
    XyzzK p;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      p.x.l[i] = q[(uint64_t)i * stride];
      p.y.l[i] = q[(uint64_t)(8 + i) * stride];
      p.zz.l[i] = q[(uint64_t)(16 + i) * stride];
      p.zzz.l[i] = q[(uint64_t)(24 + i) * stride];
    }
    return p;
  }
};

// 1G .. 8G in affine form, the shared table of double_mul, the same for every lane: computed on the host (seven
// additions) rather than spelt out
inline void generator_table(AffineK (&tab)[8]) {
  const AffineK g = generator();
  XyzzK e = XyzzK::from_affine(g);
  tab[0] = g;
  for (int m = 1; m < 8; m++) {
    xyzz_add_affine(e, g, false);
    tab[m] = to_affine(e);
  }
}

// u2 R + u1 G. One ladder for both bases (Straus, interleaved): 64 windows of 4 doublings, one addition from the
// lane's table of R and one mixed addition from the shared affine table 1G .. 8G (gtab, 8 x 64 B). A scalar above
// (n - 1) / 2 is replaced by n - k with the sign of every digit flipped.
ZK_HD XyzzK double_mul(const AffineK& R, Sc u2, Sc u1, const AffineK* gtab, const LaneTable& lt) {
  const bool neg2 = u2.is_high(), neg1 = u1.is_high();
  if (neg2) u2 = u2.neg();
  if (neg1) u1 = u1.neg();
  uint32_t mag2[8], mag1[8];
  uint64_t sgn2, sgn1;
  recode_signed4(u2.l, mag2, sgn2);
  recode_signed4(u1.l, mag1, sgn1);
  if (neg2) sgn2 = ~sgn2;
  if (neg1) sgn1 = ~sgn1;
  XyzzK e = XyzzK::from_affine(R);
  lt.put(0, e);
#pragma unroll 1
  for (int m = 1; m < 8; m++) {
    xyzz_add_affine(e, R, false);
    lt.put(m, e);
  }
  XyzzK acc = XyzzK::inf();
#pragma unroll 1
  for (int i = 0; i < 64; i++) {   // most significant digit first
#pragma unroll 1
    for (int d = 0; d < 4; d++) acc = xyzz_dbl(acc);
    const uint32_t m2 = mag2[7] >> 28, m1 = mag1[7] >> 28;
    const bool minus2 = (sgn2 >> 63) != 0, minus1 = (sgn1 >> 63) != 0;
#pragma unroll
    for (int w = 7; w > 0; w--) {
      mag2[w] = (mag2[w] << 4) | (mag2[w - 1] >> 28);
      mag1[w] = (mag1[w] << 4) | (mag1[w - 1] >> 28);
    }
    mag2[0] <<= 4;
    mag1[0] <<= 4;
    sgn2 <<= 1;
    sgn1 <<= 1;
    if (m2) {
      XyzzK t = lt.get(m2 - 1);
      if (minus2) t.y = t.y.neg();
      xyzz_add(acc, t);
    }
    if (m1) xyzz_add_affine(acc, gtab[m1 - 1], minus1);
  }
  return acc;
}

struct Recovered {
  Fp r_prime;
  AffineK q;
  uint32_t addr[5];
  uint32_t status;
};

// One signature. r, s, z: the 256-bit integers as given (z = the message hash, reduced modulo n here); given: the
// address claimed. The first status that applies wins. A lane that fails early still walks the whole path, on the
// generator in place of R and with both scalars 1, so that the lanes of a wave stay together; whatever it computed is
// zeroed at the end. Status 6 keeps its values: the command's message names both addresses.
ZK_HD Recovered recover_one(const uint32_t (&r_in)[8], const uint32_t (&s_in)[8], const uint32_t (&z_in)[8], uint32_t v,
                            const uint32_t (&given)[5], const AffineK* gtab, const LaneTable& lt) {
  Sc r, s, z;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    r.l[i] = r_in[i];
    s.l[i] = s_in[i];
    z.l[i] = z_in[i];
  }
  uint32_t status = kOk;
  if (v != 27 && v != 28) status = kBadV;
  else if (r.is_zero() || s.is_zero() || r.ge_n() || s.ge_n()) status = kBadScalar;
  else if (s.l[7] >> 31) status = kHighS;
  AffineK R = generator();
  if (status == kOk) {
#pragma unroll
    for (int i = 0; i < 8; i++) R.x.l[i] = r.l[i];   // r < n < p: canonical
  }
  // r' = sqrt(r^3 + 7) with the parity v selects (27: even, 28: odd): R = (r, r') is the nonce point itself
  const Fp rhs = R.x.sqr() * R.x + Fp::small(7);
  Fp y = rhs.sqrt_candidate();
  if (status == kOk && !(y.sqr() == rhs)) status = kNotOnCurve;
  if (status != kOk) {
    R = generator();
    y = R.y;
  } else if (y.is_odd() != (v == 28)) {
    y = y.neg();
  }
  R.y = y;
  // Q = r^-1 (s R - z G)
  Sc u1 = Sc::one(), u2 = Sc::one();
  if (status == kOk) {
    const Sc ri = r.inv();
    u1 = (z.reduce_once() * ri).neg();
    u2 = s * ri;
  }
  XyzzK Q = double_mul(R, u2, u1, gtab, lt);
  if (status == kOk && Q.is_inf()) status = kInfinity;
  if (Q.is_inf()) Q = XyzzK::from_affine(generator());
  Recovered out;
  out.q = to_affine(Q);
  out.r_prime = y;
  eth_address_words(out.q, out.addr);
  if (status == kOk) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) d |= out.addr[i] ^ given[i];
    if (d) status = kAddress;
  }
  if (status != kOk && status != kAddress) {
    out.r_prime = Fp::zero();
    out.q = {Fp::zero(), Fp::zero()};
#pragma unroll
    for (int i = 0; i < 5; i++) out.addr[i] = 0;
  }
  out.status = status;
  return out;
}

// ---- signing: RFC 6979 nonces, a fixed-base multiplication by G, the ECDSA equation -------------------------------
// What `ecdsa-sigs-parser sign` computes per key, and what noble-secp256k1's sign(msghash, key, {canonical: true})
// gives: HMAC-SHA256 DRBG, no extra entropy, low s with the recovery bit flipped. NOT hardened against side channels:
// the table index, the skipped zero digits and the branch on a high scalar all depend on the key and the nonce.
enum SignStatus : uint8_t {
  kSignOk = 0,
  kSignBadKey = 1,   // the key is zero or not below n
  kSignHighX = 2,    // the nonce point's x is n or more: r = x - n would need recovery id 2 / 3, which v = 27 / 28 cannot say
};

ZK_HD Sc sc_add(const Sc& a, const Sc& b) {   // (a + b) mod n of canonical values
  Sc r;
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)a.l[i] + b.l[i];
    r.l[i] = (uint32_t)c;
    c >>= 32;
  }
  r.add_c((c != 0 || r.ge_n()) ? 1u : 0u);   // the sum is below 2n: one correction
  return r;
}

// The key of `--generate-keys`: (h mod (n - 1)) + 1 for a 256-bit h, in [1, n). n - 1 > 2^255: one subtraction at most,
// and h - (n - 1) = h + (2^256 - n) + 1 modulo 2^256.
ZK_HD Sc key_from_hash(const uint32_t (&h)[8]) {
  Sc r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.l[i] = h[i];
  const bool ge = r.borrow_of([](int i) { return i ? Sc::N(i) : Sc::N(0) - 1u; }) == 0;
  if (ge) r.add_c(1u);
  uint64_t c = ge ? 2u : 1u;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += r.l[i];
    r.l[i] = (uint32_t)c;
    c >>= 32;
  }
  return r;
}

// key `index` of a seed: key_from_hash(SHA-256(seed || the index as 8 big-endian bytes))
ZK_HD Sc derive_key(const uint8_t* seed, uint32_t seed_len, uint64_t index) {
  uint32_t h[8], l[8];
  sha256::digest_of([=](uint32_t j) -> uint32_t { return j < seed_len ? seed[j] : (uint32_t)(index >> (8 * (7 - (j - seed_len)))) & 0xffu; },
                    seed_len + 8, h);
#pragma unroll
  for (int i = 0; i < 8; i++) l[i] = h[7 - i];
  return key_from_hash(l);
}

// The table of the fixed-base multiplication: m 16^i G for i = 0 .. 63 and m = 1 .. 8, affine, entry (i, m) at
// tab[8 i + m - 1]: the eight entries a window can ask for are 512 consecutive bytes. 512 points, 32 KiB, the same for
// every lane. Built on the host, once: 8 additions per window and 4 doublings to the next.
constexpr int kFixedWindows = 64;
constexpr int kFixedEntries = 8 * kFixedWindows;
inline void fixed_base_table(AffineK* tab) {
  AffineK base = generator();
  for (int i = 0; i < kFixedWindows; i++) {
    XyzzK e = XyzzK::from_affine(base);
    tab[8 * i] = base;
    for (int m = 1; m < 8; m++) {
      xyzz_add_affine(e, base, false);
      tab[8 * i + m] = to_affine(e);
    }
    xyzz_add_affine(e, base, false);              // 9 * 16^i G
    xyzz_add_affine(e, tab[8 * i + 6], false);    // + 7 * 16^i G
    base = to_affine(e);
  }
}
const AffineK* fixed_table_host();   // that table, built on first use and kept (csrc/ecdsa_sign.hip): the library's one copy

// k G for k in [1, n): signed digits in [-7, 8] as double_mul takes them (a scalar above (n - 1) / 2 is replaced by n - k
// with every sign flipped, so the top digit never carries), one mixed addition per non-zero digit, no doubling. The
// digit selects an entry of the shared table in global memory: all lanes are at the same window, so a wave reads from
// one 512-byte row. Never infinity: the digits describe k or n - k, neither a multiple of n.
ZK_HD XyzzK fixed_mul(Sc k, const AffineK* ftab) {
  const bool neg = k.is_high();
  if (neg) k = k.neg();
  uint32_t mag[8];
  uint64_t sgn;
  recode_signed4(k.l, mag, sgn);
  if (neg) sgn = ~sgn;
  XyzzK acc = XyzzK::inf();
#pragma unroll 1
  for (int i = 0; i < kFixedWindows; i++) {   // least significant digit first: the order is free without doublings
    const uint32_t m = mag[0] & 15u;
    const bool minus = (sgn & 1u) != 0;
#pragma unroll
    for (int w = 0; w < 7; w++) mag[w] = (mag[w] >> 4) | (mag[w + 1] << 28);
    mag[7] >>= 4;
    sgn >>= 1;
    if (m) xyzz_add_affine(acc, ftab[8 * i + (int)m - 1], minus);
  }
  return acc;
}

// HMAC-DRBG of RFC 6979 section 3.2 with SHA-256. K and V as big-endian words (word 0 = the first four bytes).
struct Drbg {
  uint32_t K[8], V[8];
};
// One HMAC of the generator. kind 0: K = HMAC(K, V || tag || x || h) (steps d and f); kind 1: K = HMAC(K, V || 0x00) (the
// retry of step h.3); kind 2: V = HMAC(K, V). kind and tag must be the same in every lane.
ZK_HD void drbg_hmac(Drbg& g, int kind, uint32_t tag, const uint32_t (&x)[8], const uint32_t (&h)[8]) {
  uint32_t m0[16], m1[16], out[8];
#pragma unroll
  for (int i = 0; i < 16; i++) m1[i] = 0;
  if (kind == 0) sha256::pad_97(g.V, tag, x, h, m0, m1);
  else if (kind == 1) sha256::pad_33(g.V, 0u, m0);
  else sha256::pad_32(g.V, m0);
  sha256::hmac32(g.K, m0, m1, kind == 0, out);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    if (kind == 2) g.V[i] = out[i];
    else g.K[i] = out[i];
  }
}
// HMACs first .. first + count - 1 of the sequence d, e, f, g, h.2 (0 .. 4: after them V is the first candidate) and then
// the retry's three per rejected candidate (K = HMAC(K, V || 0x00), V = HMAC(K, V), and h.2 again). One loop and one call:
// a kernel holds the HMAC once however many of them it runs.
ZK_HD void rfc6979_run(Drbg& g, const uint32_t (&x)[8], const uint32_t (&h)[8], int first, int count) {
#pragma unroll 1
  for (int s = first; s < first + count; s++) {
    int kind;
    if (s < 5) kind = (s == 0 || s == 2) ? 0 : 2;
    else kind = (s - 5) % 3 == 0 ? 1 : 2;
    drbg_hmac(g, kind, s == 2 ? 1u : 0u, x, h);
  }
}
// steps b - h.2: x = int2octets(key), h = bits2octets(message hash) = the hash, minus n when it is n or more
ZK_HD void rfc6979_begin(Drbg& g, const uint32_t (&x)[8], const uint32_t (&h)[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    g.K[i] = 0;
    g.V[i] = 0x01010101u;
  }
  rfc6979_run(g, x, h, 0, 5);
}
// step h.3 for a candidate that was refused: afterwards V is the next one. `refused`: how many were refused before it.
ZK_HD void rfc6979_retry(Drbg& g, const uint32_t (&x)[8], const uint32_t (&h)[8], int refused) {
  rfc6979_run(g, x, h, 5 + 3 * refused, 3);
}
// a 256-bit integer (least significant limb first) as the words of its 32 big-endian bytes, and back
ZK_HD void be_words(const uint32_t (&l)[8], uint32_t (&w)[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = l[7 - i];
}
// The candidate after `skip` refusals for this key and hash, valid or not (bits2int of V: qlen = 256, nothing to shift).
// The key is taken as it is, also when it is zero or not below n.
ZK_HD void rfc6979_candidate(const uint32_t (&key)[8], const uint32_t (&hash)[8], int skip, uint32_t (&k)[8]) {
  Sc z;
#pragma unroll
  for (int i = 0; i < 8; i++) z.l[i] = hash[i];
  z = z.reduce_once();
  uint32_t x[8], h[8];
  be_words(key, x);
  be_words(z.l, h);
  Drbg g;
  rfc6979_begin(g, x, h);
#pragma unroll 1
  for (int j = 0; j < skip; j++) rfc6979_retry(g, x, h, j);
  be_words(g.V, k);
}

struct PublicKey {
  AffineK q;
  uint32_t addr[5];
  uint32_t status;
};
// Q = d G and its address. Status 1 for a key that is zero or not below n: zeros, after the same walk with key 1.
ZK_HD PublicKey public_key(const uint32_t (&d_in)[8], const AffineK* ftab) {
  Sc d;
#pragma unroll
  for (int i = 0; i < 8; i++) d.l[i] = d_in[i];
  const uint32_t status = (d.is_zero() || d.ge_n()) ? kSignBadKey : kSignOk;
  if (status != kSignOk) d = Sc::one();
  PublicKey out;
  out.q = to_affine(fixed_mul(d, ftab));
  eth_address_words(out.q, out.addr);
  if (status != kSignOk) {
    out.q = {Fp::zero(), Fp::zero()};
#pragma unroll
    for (int i = 0; i < 5; i++) out.addr[i] = 0;
  }
  out.status = status;
  return out;
}

struct Signed {
  Sc r, s;
  uint32_t v;
  AffineK q;
  uint32_t addr[5];
  uint32_t status;
};
// One signature: Q = d G and its address, R = k G, r = R.x mod n, s = (z + r d) / k with z = hash mod n, the recovery bit
// = the parity of R.y, flipped when s is replaced by n - s because it is above (n - 1) / 2; v = 27 + bit. The two
// conversions to affine share one inversion. A candidate that is 0 or not below n, or that gives r = 0 or s = 0, is
// refused and the generator's retry step gives the next: the loop runs once but for an event of probability 2^-128. A
// lane with a bad key walks the same path with key 1 and gets zeros.
ZK_HD Signed sign_one(const uint32_t (&d_in)[8], const uint32_t (&z_in)[8], const AffineK* ftab) {
  Sc d, z;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    d.l[i] = d_in[i];
    z.l[i] = z_in[i];
  }
  uint32_t status = (d.is_zero() || d.ge_n()) ? kSignBadKey : kSignOk;
  if (status != kSignOk) d = Sc::one();
  // (Nothing but the key and the hash is kept across the generator, and the generator's state is not kept across the
  // multiplications: a retry, which never happens, starts all of it again. That is what keeps the registers down.)
  Signed out;
  int refused = 0;
#pragma unroll 1
  for (;;) {
    Sc k;
    rfc6979_candidate(d.l, z.l, refused, k.l);
    const bool bad_k = k.is_zero() || k.ge_n();
    if (bad_k) k = Sc::one();
    const XyzzK Q = fixed_mul(d, ftab);
    const XyzzK R = fixed_mul(k, ftab);
    // 1 / Q.zzz and 1 / R.zzz from one inversion; x = X / ZZ = X (ZZ / ZZZ)^2, y = Y / ZZZ as to_affine
    const Fp t = (Q.zzz * R.zzz).inv();
    const Fp iq = t * R.zzz, ir = t * Q.zzz;
    const Fp zq = Q.zz * iq, zr = R.zz * ir;
    out.q = {Q.x * zq.sqr(), Q.y * iq};
    const AffineK ra = {R.x * zr.sqr(), R.y * ir};
#pragma unroll
    for (int i = 0; i < 8; i++) out.r.l[i] = ra.x.l[i];
    const bool high_x = out.r.ge_n();
    if (high_x) out.r = Sc::one();
    out.s = k.inv() * sc_add(z.reduce_once(), out.r * d);
    uint32_t bit = ra.y.is_odd() ? 1u : 0u;
    if (out.s.is_high()) {
      out.s = out.s.neg();
      bit ^= 1u;
    }
    out.v = 27u + bit;
    const bool refuse = bad_k || (!high_x && (out.r.is_zero() || out.s.is_zero()));
    if (status == kSignOk && !refuse && high_x) status = kSignHighX;
    if (status != kSignOk || !refuse) break;
    refused++;
  }
  eth_address_words(out.q, out.addr);
  if (status != kSignOk) {
    out.r = out.s = {{0, 0, 0, 0, 0, 0, 0, 0}};
    out.v = 0;
    out.q = {Fp::zero(), Fp::zero()};
#pragma unroll
    for (int i = 0; i < 5; i++) out.addr[i] = 0;
  }
  out.status = status;
  return out;
}

}  // namespace secp
}  // namespace zkpoa
