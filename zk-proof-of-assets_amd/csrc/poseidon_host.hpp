// circomlib's Poseidon over the BN254 scalar field on the host: the parameter generator (Grain LFSR, the Poseidon
// reference's generate_parameters_grain.sage) for any width t and partial-round count R_P, and on top of it circomlibjs
// `poseidon(inputs, initState, nOut)` for t = 2..17 and the sponge of scripts/input_prep_for_layer_two.ts:46-79.
// The one generator of the library: poseidon.hip takes its t = 3, R_P = 57 tables for the device from here. Host only, no
// HIP. The hash here is the plain round form (add constants, S-box, MDS product): its largest input is the 4 limbs per
// key of one batch, a few thousand elements through rounds that depend on each other.
#pragma once
#include "host_field.hpp"

#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <vector>

namespace zkpoa {

constexpr int kPoseidonRF = 8;
constexpr int kPoseidonMaxT = 17;
// circomlib's partial rounds for t = 2..17 (poseidon.circom N_ROUNDS_P)
constexpr int kPoseidonRP[16] = {56, 57, 56, 60, 60, 63, 64, 63, 60, 66, 60, 65, 70, 60, 64, 68};

struct PoseidonHostParams {   // Montgomery form
  int t = 0, rp = 0;
  std::vector<HFr> C;   // (R_F + R_P) * t round constants, round by round
  std::vector<HFr> M;   // t x t MDS matrix, row-major: new[i] = sum_j M[i * t + j] * old[j]
};

// ---- parameter generation: generate_parameters_grain.sage 1 0 254 t 8 R_P ----------------------------------------
struct PoseidonGrain {
  uint8_t st[80];
  int step() {
    int nb = st[62] ^ st[51] ^ st[38] ^ st[23] ^ st[13] ^ st[0];
    memmove(st, st + 1, 79);
    st[79] = (uint8_t)nb;
    return nb;
  }
  int bit() {   // self-shrinking generator: a 0 discards the bit that follows it
    int nb = step();
    while (nb == 0) {
      step();
      nb = step();
    }
    return step();
  }
  PoseidonGrain(unsigned t, unsigned rf, unsigned rp) {
    const unsigned vals[6] = {1, 0, 254, t, rf, rp}, widths[6] = {2, 4, 12, 12, 10, 10};   // field, sbox, n, t, R_F, R_P
    unsigned pos = 0;
    for (int f = 0; f < 6; f++)
      for (int b = (int)widths[f] - 1; b >= 0; b--) st[pos++] = (vals[f] >> b) & 1u;
    while (pos < 80) st[pos++] = 1;
    for (int i = 0; i < 160; i++) step();
  }
  void bits254(uint64_t out[4]) {   // most significant bit first
    out[0] = out[1] = out[2] = out[3] = 0;
    for (int i = 253; i >= 0; i--)
      if (bit()) out[i >> 6] |= 1ull << (i & 63);
  }
};

inline void poseidon_generate(int t, int rp, PoseidonHostParams& out) {
  out.t = t;
  out.rp = rp;
  out.C.resize((size_t)(kPoseidonRF + rp) * t);
  out.M.resize((size_t)t * t);
  PoseidonGrain g((unsigned)t, kPoseidonRF, (unsigned)rp);
  for (size_t i = 0; i < out.C.size();) {   // round constants: rejection sampling
    uint64_t v[4];
    g.bits254(v);
    if (HFr::geq_p(v)) continue;
    out.C[i++] = HFr{{v[0], v[1], v[2], v[3]}}.to_mont();
  }
  for (;;) {   // MDS: Cauchy matrix 1 / (x_i + y_j) over 2t distinct elements (reduced, not rejected)
    std::vector<HFr> xy((size_t)2 * t);
    bool ok = true;
    for (int i = 0; i < 2 * t; i++) {
      uint64_t v[4];
      g.bits254(v);
      if (HFr::geq_p(v)) HFr::sub_p(v);   // F(bits): 2^254 < 2r, one subtraction
      xy[i] = HFr{{v[0], v[1], v[2], v[3]}}.to_mont();
    }
    for (int i = 0; i < 2 * t && ok; i++)
      for (int j = 0; j < i; j++)
        if (xy[i] == xy[j]) ok = false;
    for (int i = 0; i < t && ok; i++)
      for (int j = 0; j < t; j++) {
        const HFr s = xy[i] + xy[t + j];
        if (s.is_zero()) {
          ok = false;
          break;
        }
        out.M[(size_t)i * t + j] = s.inv();
      }
    if (ok) return;
  }
}

// circomlib's parameters of width t (2..17), generated on first use and kept
inline const PoseidonHostParams& poseidon_params_for(int t) {
  if (t < 2 || t > kPoseidonMaxT) throw std::runtime_error("poseidon: the width must be 2..17 (1..16 inputs)");
  static std::mutex mu;
  static std::map<int, std::unique_ptr<PoseidonHostParams>> made;
  std::lock_guard<std::mutex> lock(mu);
  std::unique_ptr<PoseidonHostParams>& p = made[t];
  if (!p) {
    p.reset(new PoseidonHostParams());
    poseidon_generate(t, kPoseidonRP[t - 2], *p);
  }
  return *p;
}

inline HFr poseidon_pow5(const HFr& x) {
  const HFr x2 = x.sqr();
  return x2.sqr() * x;
}

// circomlibjs poseidon(inputs, initState, nOut): the state is [init, inputs...]; out <- its first n_out elements after
// the permutation. Montgomery form in and out; n = 1..16, n_out = 1..n + 1.
inline void poseidon_hash(const HFr* inputs, int n, const HFr& init, int n_out, HFr* out) {
  const PoseidonHostParams& prm = poseidon_params_for(n + 1);
  const int t = prm.t, rounds = kPoseidonRF + prm.rp;
  if (n_out < 1 || n_out > t) throw std::runtime_error("poseidon: the number of outputs must be 1..t");
  HFr s[kPoseidonMaxT], nx[kPoseidonMaxT];
  s[0] = init;
  for (int i = 0; i < n; i++) s[i + 1] = inputs[i];
  for (int r = 0; r < rounds; r++) {
    for (int i = 0; i < t; i++) s[i] = s[i] + prm.C[(size_t)r * t + i];
    if (r < kPoseidonRF / 2 || r >= kPoseidonRF / 2 + prm.rp) {
      for (int i = 0; i < t; i++) s[i] = poseidon_pow5(s[i]);
    } else {
      s[0] = poseidon_pow5(s[0]);
    }
    for (int i = 0; i < t; i++) {
      HFr acc = HFr::zero();
      for (int j = 0; j < t; j++) acc = acc + prm.M[(size_t)i * t + j] * s[j];
      nx[i] = acc;
    }
    for (int i = 0; i < t; i++) s[i] = nx[i];
  }
  for (int i = 0; i < n_out; i++) out[i] = s[i];
}

// poseidonSponge (input_prep_for_layer_two.ts:46-79): 16 inputs per round with the previous round's state[0] as the
// initial state; the last round asks for two outputs and its state[1] is the hash. The last round reads its inputs at
// i * lastRoundLength, not at i * 16 (:71 after :67 has overwritten roundLength): for 28 inputs the second round absorbs
// inputs 12..23 and inputs 24..27 are never read. The reference's committed hashes hold only with this rule.
inline HFr poseidon_sponge(const HFr* inputs, uint64_t n) {
  if (n == 0) throw std::runtime_error("poseidon sponge: no input");
  uint64_t rounds = n / 16, last = 16;
  if (n % 16) {
    rounds++;
    last = n % 16;
  }
  HFr h = HFr::zero();
  for (uint64_t i = 0; i + 1 < rounds; i++) poseidon_hash(inputs + 16 * i, 16, h, 1, &h);
  HFr two[2];
  poseidon_hash(inputs + (rounds - 1) * last, (int)last, h, 2, two);
  return two[1];
}

}  // namespace zkpoa
