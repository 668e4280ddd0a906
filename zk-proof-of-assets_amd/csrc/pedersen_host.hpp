// The Pedersen commitment of the balance sum on ed25519, as scripts/lib/pedersen_commitment.ts computes it: extended
// coordinates (x, y, z, t), the addition formula of `pointAdd` for additions and doublings alike, the double-and-add of
// `pointMul` from the least significant bit, the two generators, the 3 x 85-bit chunks of the circuit's signals and the
// projective comparison of `pointEqual`. Host only: the whole check is two scalar multiplications.
#pragma once
#include "host_text.hpp"

namespace zkpoa {

// GF(2^255 - 19) on U256 values; every function takes any value below 2^256 and returns one, canon() the least residue
struct Fe25519 {
  typedef unsigned __int128 u128;
  static U256 reduce_wide(const uint64_t t[8]) {   // 2^256 = 38
    U256 r;
    u128 c = 0;
    for (int i = 0; i < 4; i++) {
      c += (u128)t[i] + (u128)t[4 + i] * 38;
      r.v[i] = (uint64_t)c;
      c >>= 64;
    }
    for (int pass = 0; pass < 2; pass++) {   // the carry is below 39; after the second pass there is none
      c *= 38;
      for (int i = 0; i < 4; i++) {
        c += r.v[i];
        r.v[i] = (uint64_t)c;
        c >>= 64;
      }
    }
    return r;
  }
  static U256 canon(U256 a) {
    const uint64_t top = a.v[3] >> 63;   // 2^255 = 19
    a.v[3] &= ~(1ull << 63);
    u128 c = top * 19;
    for (int i = 0; i < 4; i++) {
      c += a.v[i];
      a.v[i] = (uint64_t)c;
      c >>= 64;
    }
    static const uint64_t P[4] = {0xffffffffffffffedull, 0xffffffffffffffffull, 0xffffffffffffffffull, 0x7fffffffffffffffull};
    while (!a.below(P)) {   // below p + 38: at most once
      u128 bw = 0;
      for (int i = 0; i < 4; i++) {
        const u128 d = (u128)a.v[i] - P[i] - bw;
        a.v[i] = (uint64_t)d;
        bw = (d >> 64) & 1;
      }
    }
    return a;
  }
  static U256 add(const U256& a, const U256& b) {
    uint64_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    u128 c = 0;
    for (int i = 0; i < 4; i++) {
      c += (u128)a.v[i] + b.v[i];
      t[i] = (uint64_t)c;
      c >>= 64;
    }
    t[4] = (uint64_t)c;
    return reduce_wide(t);
  }
  static U256 neg(const U256& a) {   // p - a, for the least residue a
    static const uint64_t P[4] = {0xffffffffffffffedull, 0xffffffffffffffffull, 0xffffffffffffffffull, 0x7fffffffffffffffull};
    const U256 x = canon(a);
    U256 r;
    u128 bw = 0;
    for (int i = 0; i < 4; i++) {
      const u128 d = (u128)P[i] - x.v[i] - bw;
      r.v[i] = (uint64_t)d;
      bw = (d >> 64) & 1;
    }
    return r;   // p for a = 0: canon() makes it 0 again
  }
  static U256 sub(const U256& a, const U256& b) { return add(a, neg(b)); }
  static U256 mul(const U256& a, const U256& b) {
    uint64_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
      u128 c = 0;
      for (int j = 0; j < 4; j++) {
        c += (u128)a.v[i] * b.v[j] + t[i + j];
        t[i + j] = (uint64_t)c;
        c >>= 64;
      }
      t[i + 4] = (uint64_t)c;
    }
    return reduce_wide(t);
  }
  static bool is_zero(const U256& a) {
    const U256 x = canon(a);
    return (x.v[0] | x.v[1] | x.v[2] | x.v[3]) == 0;
  }
  static U256 inv(const U256& a) {   // a^(p - 2), bit by bit from the top; 0 for a = 0
    static const uint64_t E[4] = {0xffffffffffffffebull, 0xffffffffffffffffull, 0xffffffffffffffffull, 0x7fffffffffffffffull};
    U256 r;
    r.v[0] = 1;
    for (int b = 254; b >= 0; b--) {
      r = mul(r, r);
      if ((E[b >> 6] >> (b & 63)) & 1) r = mul(r, a);
    }
    return r;
  }
};

struct EdPoint {
  U256 x, y, z, t;
};

inline U256 u256_dec(const char* s) {
  U256 x;
  if (!x.parse_dec(s, s + strlen(s))) throw std::runtime_error("pedersen: a constant does not parse");
  return x;
}

// generator_g (the base point of ed25519) and generator_h (Bulletproofs' hash of it) of lib/pedersen_commitment.ts
inline const EdPoint& pedersen_generator_g() {
  static const EdPoint g{u256_dec("15112221349535400772501151409588531511454012693041857206046113283949847762202"),
                         u256_dec("46316835694926478169428394003475163141307993866256225615783033603165251855960"), u256_dec("1"),
                         u256_dec("46827403850823179245072216630277197565144205554125654976674165829533817101731")};
  return g;
}
inline const EdPoint& pedersen_generator_h() {
  static const EdPoint h{u256_dec("33610936965734216034622052748864527785054979741013463956582067314415336407764"),
                         u256_dec("39037926758455103342491841394431773648115673280860795116462000885017926418697"),
                         u256_dec("44972472311651602601636560056538958210842501314939311016992875096561375476462"),
                         u256_dec("25285931357802837959040485138497351343220742265312934020814563180777586254493")};
  return h;
}

inline const U256& ed_d() {   // the curve's d = -121665 / 121666
  static const U256 d = u256_dec("37095705934669439343138083508754565189542113879843219016388785533085940283555");
  return d;
}

inline EdPoint ed_add(const EdPoint& p, const EdPoint& q) {   // pointAdd
  typedef Fe25519 F;
  const U256& d = ed_d();
  const U256 A = F::mul(F::sub(p.y, p.x), F::sub(q.y, q.x));
  const U256 B = F::mul(F::add(p.y, p.x), F::add(q.y, q.x));
  const U256 tt = F::mul(p.t, q.t), zz = F::mul(p.z, q.z);
  const U256 C = F::mul(F::add(tt, tt), d);
  const U256 D = F::add(zz, zz);
  const U256 E = F::sub(B, A), Fv = F::sub(D, C), G = F::add(D, C), H = F::add(B, A);
  return EdPoint{F::mul(E, Fv), F::mul(G, H), F::mul(Fv, G), F::mul(E, H)};
}

inline EdPoint ed_mul(U256 s, EdPoint p) {   // pointMul: the same additions in the same order
  EdPoint q{U256(), u256_dec("1"), u256_dec("1"), U256()};
  while (s.v[0] | s.v[1] | s.v[2] | s.v[3]) {
    if (s.v[0] & 1) q = ed_add(q, p);
    p = ed_add(p, p);
    for (int i = 0; i < 4; i++) s.v[i] = (s.v[i] >> 1) | (i < 3 ? s.v[i + 1] << 63 : 0);
  }
  return q;
}

inline EdPoint ed_canon(const EdPoint& p) {
  return EdPoint{Fe25519::canon(p.x), Fe25519::canon(p.y), Fe25519::canon(p.z), Fe25519::canon(p.t)};
}

// pedersenCommitment: secret * G + blinding * H, every coordinate the least residue
inline EdPoint pedersen_commit(const U256& secret, const U256& blinding) {
  return ed_canon(ed_add(ed_mul(secret, pedersen_generator_g()), ed_mul(blinding, pedersen_generator_h())));
}

// dechunkToPoint: coordinate i = signals[3i] + 2^85 signals[3i + 1] + 2^170 signals[3i + 2] (mod p)
inline EdPoint pedersen_dechunk(const U256 signals[12]) {
  typedef Fe25519 F;
  U256 s85, s170;
  s85.v[1] = 1ull << 21;
  s170.v[2] = 1ull << 42;
  U256 c[4];
  for (int i = 0; i < 4; i++)
    c[i] = F::add(signals[3 * i], F::add(F::mul(signals[3 * i + 1], s85), F::mul(signals[3 * i + 2], s170)));
  return EdPoint{c[0], c[1], c[2], c[3]};
}

inline bool ed_equal(const EdPoint& p, const EdPoint& q) {   // pointEqual: x1 z2 = x2 z1 and y1 z2 = y2 z1
  typedef Fe25519 F;
  return F::is_zero(F::sub(F::mul(p.x, q.z), F::mul(q.x, p.z))) && F::is_zero(F::sub(F::mul(p.y, q.z), F::mul(q.y, p.z)));
}

// The point the layer-three circuit's first 12 public signals spell, as a verifier reads it: false when a signal does not
// fit 85 bits, Z = 0, or (X, Y, Z, T) does not satisfy the extended-coordinate equations of ed25519,
// -X^2 + Y^2 = Z^2 + d T^2 and X Y = Z T. compressed <- the RFC 8032 encoding of (X / Z, Y / Z): y little-endian, bit
// 255 = the low bit of x. Whether the point lies in the prime-order subgroup is NOT checked.
inline bool pedersen_decode(const U256 signals[12], uint8_t compressed[32]) {
  typedef Fe25519 F;
  memset(compressed, 0, 32);
  for (int i = 0; i < 12; i++)
    if (signals[i].v[3] | signals[i].v[2] | (signals[i].v[1] >> 21)) return false;
  const EdPoint p = pedersen_dechunk(signals);
  if (F::is_zero(p.z)) return false;
  const U256 xx = F::mul(p.x, p.x), yy = F::mul(p.y, p.y), zz = F::mul(p.z, p.z), tt = F::mul(p.t, p.t);
  if (!F::is_zero(F::sub(F::sub(yy, xx), F::add(zz, F::mul(ed_d(), tt))))) return false;
  if (!F::is_zero(F::sub(F::mul(p.x, p.y), F::mul(p.z, p.t)))) return false;
  const U256 zi = F::inv(p.z);
  const U256 x = F::canon(F::mul(p.x, zi));
  U256 y = F::canon(F::mul(p.y, zi));
  y.v[3] |= (x.v[0] & 1) << 63;
  y.to_le(compressed);
  return true;
}

// x as three 85-bit chunks, least significant first (chunkBigInt(x, 2^85), padded to 3)
inline void chunks85(const U256& x, U256 out[3]) {
  for (int k = 0; k < 3; k++) {
    out[k] = U256();
    for (int b = 0; b < 85; b++) {
      const int src = 85 * k + b;
      if (src < 256 && ((x.v[src >> 6] >> (src & 63)) & 1)) out[k].v[b >> 6] |= 1ull << (b & 63);
    }
  }
}

}  // namespace zkpoa
