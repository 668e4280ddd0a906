// Host-only C entry points of the phase-2 transcript's primitives (csrc/phase2.hpp; include/zkpoa_prover.h): no context,
// no GPU. The tests reach Blake2b, SHA-256, the ChaCha generator, the square roots and `fromRng` through these.
#include "../../include/zkpoa_prover.h"
#include "phase2.hpp"

using namespace zkpoa;
namespace p2 = zkpoa::phase2;

#define P2_TRY try {
#define P2_END                       \
  }                                  \
  catch (const std::exception&) {    \
    return PROVER_ERROR;             \
  }                                  \
  return PROVER_OK;

extern "C" int zkpoa_blake2b512(const void* data, unsigned long len, uint8_t out[64]) {
  P2_TRY
  p2::blake2b512(data, len, out);
  P2_END
}
extern "C" void* zkpoa_blake2b_new(void) { return new p2::Blake2b(); }
extern "C" int zkpoa_blake2b_update(void* state, const void* data, unsigned long len) {
  if (!state) return PROVER_ERROR;
  static_cast<p2::Blake2b*>(state)->update(data, len);
  return PROVER_OK;
}
extern "C" int zkpoa_blake2b_final(void* state, uint8_t out[64]) {
  if (!state) return PROVER_ERROR;
  p2::Blake2b* b = static_cast<p2::Blake2b*>(state);
  b->final(out);
  delete b;
  return PROVER_OK;
}
extern "C" int zkpoa_sha256(const void* data, unsigned long len, uint8_t out[32]) {
  P2_TRY
  p2::sha256(data, len, out);
  P2_END
}
extern "C" void* zkpoa_chacha_new(const uint32_t key[8]) { return new p2::ChaCha(key); }
extern "C" uint32_t zkpoa_chacha_next_u32(void* rng) { return static_cast<p2::ChaCha*>(rng)->next_u32(); }
extern "C" uint64_t zkpoa_chacha_next_u64(void* rng) { return static_cast<p2::ChaCha*>(rng)->next_u64(); }
extern "C" int zkpoa_chacha_next_bool(void* rng) { return static_cast<p2::ChaCha*>(rng)->next_bool() ? 1 : 0; }
extern "C" void zkpoa_chacha_free(void* rng) { delete static_cast<p2::ChaCha*>(rng); }

static bool fq_in(const uint8_t* p, HFq* out) {
  uint64_t v[4];
  memcpy(v, p, 32);
  if (HFq::geq_p(v)) return false;
  *out = HFq::from_bytes(p).to_mont();
  return true;
}
extern "C" int zkpoa_fq_sqrt(const uint8_t a[32], uint8_t root[32]) {
  HFq x, r;
  if (!fq_in(a, &x) || !p2::fq_sqrt(x, &r)) return 0;
  r.from_mont().to_bytes(root);
  return 1;
}
extern "C" int zkpoa_fq2_sqrt(const uint8_t a[64], uint8_t root[64]) {
  HFq2 x, r;
  if (!fq_in(a, &x.c0) || !fq_in(a + 32, &x.c1) || !p2::fq2_sqrt(x, &r)) return 0;
  r.c0.from_mont().to_bytes(root);
  r.c1.from_mont().to_bytes(root + 32);
  return 1;
}
extern "C" int zkpoa_fr_from_rng(const uint32_t key[8], uint8_t out[32]) {
  P2_TRY
  p2::ChaCha rng(key);
  p2::fr_from_rng(rng, out);
  P2_END
}
extern "C" int zkpoa_g1_from_rng(const uint32_t key[8], uint8_t out[64]) {
  P2_TRY
  p2::ChaCha rng(key);
  h_affine_to_bytes<HFq>(p2::g1_from_rng(rng), out);
  P2_END
}
extern "C" int zkpoa_g2_from_rng(const uint32_t key[8], uint8_t out[128]) {
  P2_TRY
  p2::ChaCha rng(key);
  h_affine_to_bytes<HFq2>(p2::g2_from_rng(rng), out);
  P2_END
}
extern "C" int zkpoa_hash_to_g2(const uint8_t hash[64], uint8_t out[128]) {
  P2_TRY
  h_affine_to_bytes<HFq2>(p2::hash_to_g2(hash), out);
  P2_END
}
extern "C" int zkpoa_beacon_key(const uint8_t* beacon, unsigned long len, uint32_t num_iterations_exp, uint32_t key[8]) {
  P2_TRY
  p2::beacon_key(beacon, len, num_iterations_exp, key);
  P2_END
}
