// The phase-1 transcript of a .ptau (section 7), host side, no GPU: what `snarkjs powersoftau new / contribute / beacon /
// verify` hash, draw and check, written from DESIGN.md "Phase-1 transcript" on top of the primitives of csrc/phase2.hpp
// (Blake2b-512, the ChaCha generator, `fromRng`, hash-to-G2, the beacon key and draw, the hash form of a point, mul_wire,
// the type and params that end a record: RecordParams) and the section table of csrc/binfile.hpp. The saved Blake2b
// state, the contribution key, the records of section 7 and the checks that need pairings only.
#pragma once
#include "binfile.hpp"
#include "phase2.hpp"

namespace zkpoa {
template <class HF>
Affine<HF> host_generator();
template <> Affine<HFq> host_generator<HFq>();     // hooks_g1.hip
template <> Affine<HFq2> host_generator<HFq2>();   // hooks_g2.hip
namespace phase1 {

namespace p2 = zkpoa::phase2;

// ---- the Blake2b state of a record's partialHash: h[8], t[2], the buffer, its fill; little-endian u64 ---------------------
constexpr size_t kStateLen = 216;
inline void blake2b_save(const p2::Blake2b& b, uint8_t out[kStateLen]) {
  memcpy(out, b.h, 64);
  memcpy(out + 64, b.t, 16);
  memset(out + 80, 0, 128);
  memcpy(out + 80, b.buf, b.fill);
  const uint64_t fill = b.fill;
  memcpy(out + 208, &fill, 8);
}
inline bool blake2b_restore(const uint8_t in[kStateLen], p2::Blake2b* b) {
  uint64_t fill;
  memcpy(&fill, in + 208, 8);
  if (fill > 128) return false;
  memcpy(b->h, in, 64);
  memcpy(b->t, in + 64, 16);
  memcpy(b->buf, in + 80, 128);
  b->fill = (size_t)fill;
  return true;
}

// ---- the contribution key ---------------------------------------------------------------------------------------------
// nine points, wire form: tau.g1_s, tau.g1_sx, alpha.g1_s, alpha.g1_sx, beta.g1_s, beta.g1_sx, tau.g2_spx, alpha.g2_spx,
// beta.g2_spx
constexpr size_t kKeyLen = 6 * 64 + 3 * 128;
inline const uint8_t* key_g1_s(const uint8_t* key, int k) { return key + 128 * k; }
inline const uint8_t* key_g1_sx(const uint8_t* key, int k) { return key + 128 * k + 64; }
inline const uint8_t* key_g2_spx(const uint8_t* key, int k) { return key + 384 + 128 * k; }

struct Secrets {   // k = 0 tau, 1 alpha, 2 beta
  uint8_t x[3][32];      // standard form, little-endian, in [1, r)
  uint8_t g1_s[3][64];   // wire form
};
// g2_sp = hashToG2(Blake2b-512(personalisation byte | challenge | hash form of g1_s | hash form of g1_sx))
inline pairing::G2 g2_sp(int k, const uint8_t challenge[64], const uint8_t* g1_s, const uint8_t* g1_sx) {
  p2::Blake2b h;
  const uint8_t pers = (uint8_t)k;
  h.update(&pers, 1);
  h.update(challenge, 64);
  p2::hash_g1_wire(h, g1_s);
  p2::hash_g1_wire(h, g1_sx);
  uint8_t d[64];
  h.final(d);
  return p2::hash_to_g2(d);
}
inline void make_key(const Secrets& s, const uint8_t challenge[64], uint8_t key[kKeyLen]) {
  for (int k = 0; k < 3; k++) {
    uint8_t* g1_s = key + 128 * k;
    memcpy(g1_s, s.g1_s[k], 64);
    p2::mul_wire<HFq>(g1_s, s.x[k], g1_s + 64);
    uint8_t sp[128];
    h_affine_to_bytes<HFq2>(g2_sp(k, challenge, g1_s, g1_s + 64), sp);
    p2::mul_wire<HFq2>(sp, s.x[k], key + 384 + 128 * k);
  }
}
// a beacon: per key, in the order tau, alpha, beta: the secret (fromRng Fr), then g1_s (fromRng G1), one generator
inline void beacon_secrets(const uint8_t* beacon, size_t len, uint32_t exp, Secrets* s) {
  uint32_t key[8];
  p2::beacon_key(beacon, len, exp, key);
  p2::ChaCha rng(key);
  for (int k = 0; k < 3; k++) p2::beacon_draw(rng, s->x[k], s->g1_s[k]);
}
inline void hash_key(p2::Blake2b& h, const uint8_t key[kKeyLen]) {
  for (int i = 0; i < 6; i++) p2::hash_g1_wire(h, key + 64 * i);
  for (int i = 0; i < 3; i++) p2::hash_g2_wire(h, key + 384 + 128 * i);
}
// the response hash, finished from the state after the sections and the key; false for a state that cannot be one
inline bool response_hash(const uint8_t partial[kStateLen], const uint8_t key[kKeyLen], uint8_t out[64]) {
  p2::Blake2b h;
  if (!blake2b_restore(partial, &h)) return false;
  hash_key(h, key);
  h.final(out);
  return true;
}
// the challenge of a fresh file of 2^power: Blake2b-512(Blake2b-512("") | hash form of sections 2-6, all generators)
inline void fresh_challenge(uint32_t power, uint8_t out[64]) {
  uint8_t g1[64], g2[128], e[64];
  p2::g1_hash_form(host_generator<HFq>(), g1);
  p2::g2_hash_form(host_generator<HFq2>(), g2);
  p2::blake2b512("", 0, e);
  p2::Blake2b h;
  h.update(e, 64);
  std::vector<uint8_t> run1(64 * 1024), run2(128 * 1024);   // 1024 points at a time
  for (size_t i = 0; i < 1024; i++) {
    memcpy(&run1[64 * i], g1, 64);
    memcpy(&run2[128 * i], g2, 128);
  }
  for (const PowerSec& sc : ptau_power_secs(power))
    for (uint64_t done = 0; done < sc.count; done += 1024)
      h.update(sc.group == 2 ? run2.data() : run1.data(), sc.unit() * std::min<uint64_t>(1024, sc.count - done));
  h.final(out);
}

// ---- section 7: u32 count, then the records --------------------------------------------------------------------------
struct Record : p2::RecordParams {
  uint8_t tau_g1[64], tau_g2[128], alpha_g1[64], beta_g1[64], beta_g2[128];   // after the contribution, wire form
  uint8_t key[kKeyLen];
  uint8_t partial[kStateLen], next_challenge[64];
};
constexpr size_t kRecordHead = 448 + kKeyLen + kStateLen + 64;   // what precedes the record's type and params
inline std::vector<Record> parse_section7(const uint8_t* p, uint64_t len) {
  const char* const what = "ptau: section 7 is truncated, over-long or holds an unknown record";
  if (len < 4) throw std::runtime_error(what);
  uint32_t count;
  memcpy(&count, p, 4);
  uint64_t at = 4;
  std::vector<Record> out;
  for (uint32_t k = 0; k < count; k++) {
    if (len - at < kRecordHead) throw std::runtime_error(what);
    Record r;
    memcpy(r.tau_g1, p + at, 64);
    memcpy(r.tau_g2, p + at + 64, 128);
    memcpy(r.alpha_g1, p + at + 192, 64);
    memcpy(r.beta_g1, p + at + 256, 64);
    memcpy(r.beta_g2, p + at + 320, 128);
    memcpy(r.key, p + at + 448, kKeyLen);
    memcpy(r.partial, p + at + 448 + kKeyLen, kStateLen);
    memcpy(r.next_challenge, p + at + 448 + kKeyLen + kStateLen, 64);
    at += kRecordHead;
    at += r.parse(p + at, len - at, what);
    out.push_back(r);
  }
  if (at != len) throw std::runtime_error(what);
  return out;
}
inline std::vector<uint8_t> write_section7(const std::vector<Record>& records) {
  std::vector<uint8_t> out;
  auto put = [&](const uint8_t* p, size_t n) { out.insert(out.end(), p, p + n); };
  const uint32_t count = (uint32_t)records.size();
  put((const uint8_t*)&count, 4);
  for (const Record& r : records) {
    put(r.tau_g1, 64);
    put(r.tau_g2, 128);
    put(r.alpha_g1, 64);
    put(r.beta_g1, 64);
    put(r.beta_g2, 128);
    put(r.key, kKeyLen);
    put(r.partial, kStateLen);
    put(r.next_challenge, 64);
    r.write(out);
  }
  return out;
}

// ---- the checks of `powersoftau verify` that need the records and pairings only -------------------------------------
inline bool coords_ok(const uint8_t* p, size_t count32) {
  for (size_t i = 0; i < count32; i++) {
    uint64_t v[4];
    memcpy(v, p + 32 * i, 32);
    if (HFq::geq_p(v)) return false;
  }
  return true;
}
inline bool g1_ok(const uint8_t* w, pairing::G1* out) {
  if (!coords_ok(w, 2)) return false;
  *out = h_affine_from_bytes<HFq>(w);
  return !out->is_inf() && pairing::g1_on_curve(*out);
}
inline bool g2_ok(const uint8_t* w, pairing::G2* out) {
  static const uint64_t kR[4] = {HFrParams::P[0], HFrParams::P[1], HFrParams::P[2], HFrParams::P[3]};
  if (!coords_ok(w, 4)) return false;
  *out = h_affine_from_bytes<HFq2>(w);
  return !out->is_inf() && pairing::g2_on_curve(*out) && h_mul(XYZZ<HFq2>::from_affine(*out), kR).is_inf();
}
// Where a trail stands before a record: the five points the record's are checked against (the generators before the
// first) and the challenge its key was made for (the fresh challenge before the first).
struct Trail {
  pairing::G1 tau1, alpha1, beta1;
  pairing::G2 tau2, beta2;
  uint8_t challenge[64];
};
inline Trail fresh_trail(uint32_t power) {
  Trail t{host_generator<HFq>(), host_generator<HFq>(), host_generator<HFq>(), host_generator<HFq2>(), host_generator<HFq2>(), {}};
  fresh_challenge(power, t.challenge);
  return t;
}
// the trail after r, taken from r alone: false when one of its five points is no point of its group
inline bool trail_after(const Record& r, Trail* t) {
  if (!g1_ok(r.tau_g1, &t->tau1) || !g2_ok(r.tau_g2, &t->tau2) || !g1_ok(r.alpha_g1, &t->alpha1) || !g1_ok(r.beta_g1, &t->beta1) ||
      !g2_ok(r.beta_g2, &t->beta2))
    return false;
  memcpy(t->challenge, r.next_challenge, 64);
  return true;
}
// Where the trail of a file of 2^power with these records stands, the one statement of it: what the last record left,
// or the fresh file's (whose challenge is a hash over 2^(power + 2) points: made only for a file without records).
inline void trail_challenge(const std::vector<Record>& records, uint32_t power, uint8_t out[64]) {   // what the next key answers
  if (records.empty()) fresh_challenge(power, out);
  else memcpy(out, records.back().next_challenge, 64);
}
inline bool trail_end(const std::vector<Record>& records, uint32_t power, Trail* t) {   // false: as trail_after
  if (!records.empty()) return trail_after(records.back(), t);
  *t = fresh_trail(power);
  return true;
}
// the response hash that opens a challenge file: Blake2b-512("") before the first record; false: as response_hash
inline bool trail_response(const std::vector<Record>& records, uint8_t out[64]) {
  if (!records.empty()) return response_hash(records.back().partial, records.back().key, out);
  p2::blake2b512("", 0, out);
  return true;
}
// One record against the trail before it: its points and its key's are points of their groups, a beacon's key is the
// beacon's, each g2_spx carries the x of its g1_sx, and the record's points are the trail's times those x. On true the
// trail has moved past the record.
inline bool verify_record(const Record& r, Trail& t) {
  pairing::G1 s[3], sx[3];
  pairing::G2 spx[3], sp[3];
  Trail next;
  if (!trail_after(r, &next)) return false;
  for (int k = 0; k < 3; k++)
    if (!g1_ok(key_g1_s(r.key, k), &s[k]) || !g1_ok(key_g1_sx(r.key, k), &sx[k]) || !g2_ok(key_g2_spx(r.key, k), &spx[k]))
      return false;
  if (r.type == 1) {   // a beacon's secrets are public: g1_s and g1_sx recomputed
    if (r.num_iterations_exp > p2::kMaxBeaconExp) return false;
    Secrets bs;
    beacon_secrets(r.beacon.data(), r.beacon.size(), r.num_iterations_exp, &bs);
    for (int k = 0; k < 3; k++) {
      uint8_t want[64];
      p2::mul_wire<HFq>(bs.g1_s[k], bs.x[k], want);
      if (memcmp(bs.g1_s[k], key_g1_s(r.key, k), 64) || memcmp(want, key_g1_sx(r.key, k), 64)) return false;
    }
  }
  for (int k = 0; k < 3; k++) {
    sp[k] = g2_sp(k, t.challenge, key_g1_s(r.key, k), key_g1_sx(r.key, k));
    if (!pairing::pair_eq(s[k], spx[k], sx[k], sp[k])) return false;   // the same x in g1_sx and g2_spx
  }
  if (!pairing::pair_eq(next.tau1, sp[0], t.tau1, spx[0]) || !pairing::pair_eq(next.alpha1, sp[1], t.alpha1, spx[1]) ||
      !pairing::pair_eq(next.beta1, sp[2], t.beta1, spx[2]))
    return false;
  if (!pairing::pair_eq(s[0], next.tau2, sx[0], t.tau2) || !pairing::pair_eq(s[2], next.beta2, sx[2], t.beta2)) return false;
  t = next;
  return true;
}
// Every record against the one before it (the generators and the fresh challenge before the first); the last record's
// five points against the file's (T_1, U_1, A_0, B_0, beta2: wire form). On true, *last_response holds the last record's
// response hash: the caller compares Blake2b(response | hash form of the file's sections 2-6) with its nextChallenge.
inline bool verify_records(const std::vector<Record>& records, uint32_t power, const uint8_t* T1, const uint8_t* U1,
                           const uint8_t* A0, const uint8_t* B0, const uint8_t* beta2, uint8_t last_response[64]) {
  if (records.empty()) return true;
  Trail t = fresh_trail(power);
  for (const Record& r : records)
    if (!verify_record(r, t)) return false;
  const Record& last = records.back();
  if (memcmp(last.tau_g1, T1, 64) || memcmp(last.tau_g2, U1, 128) || memcmp(last.alpha_g1, A0, 64) ||
      memcmp(last.beta_g1, B0, 64) || memcmp(last.beta_g2, beta2, 128))
    return false;
  return response_hash(last.partial, last.key, last_response);
}

}  // namespace phase1
}  // namespace zkpoa
