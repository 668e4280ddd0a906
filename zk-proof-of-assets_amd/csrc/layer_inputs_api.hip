// Host-only C entry points of the layer-two / layer-three input arithmetic (include/zkpoa_layer_inputs.h): the Poseidon
// of poseidon_host.hpp and the ed25519 commitment of pedersen_host.hpp; and the verifier's reading of that commitment
// (zkpoa_pedersen_decode, include/zkpoa_audit.h). No context, no GPU.
#include "../../include/zkpoa_prover.h"
#include "pedersen_host.hpp"
#include "poseidon_host.hpp"

using namespace zkpoa;

namespace {

// n x 32 B little-endian, each below the field's order -> Montgomery form
void load_fr(const uint8_t* in, uint64_t n, HFr* out) {
  for (uint64_t i = 0; i < n; i++) {
    const HFr v = HFr::from_bytes(in + 32 * i);
    if (HFr::geq_p(v.l)) throw std::runtime_error("poseidon: an input is not below the field's order");
    out[i] = v.to_mont();
  }
}

void store_point(const EdPoint& p, uint8_t out[128]) {
  p.x.to_le(out);
  p.y.to_le(out + 32);
  p.z.to_le(out + 64);
  p.t.to_le(out + 96);
}

}  // namespace

#define LI_TRY try {
#define LI_END                       \
  }                                  \
  catch (const std::exception&) {    \
    return PROVER_ERROR;             \
  }                                  \
  return PROVER_OK;

extern "C" int zkpoa_poseidon_hash(const uint8_t* inputs, unsigned n_inputs, const uint8_t init_state[32], unsigned n_out,
                                   uint8_t* out) {
  if (!inputs || !init_state || !out || n_inputs < 1 || n_inputs > 16 || n_out < 1 || n_out > n_inputs + 1) return PROVER_ERROR;
  LI_TRY
  HFr in[16], init, res[kPoseidonMaxT];
  load_fr(inputs, n_inputs, in);
  load_fr(init_state, 1, &init);
  poseidon_hash(in, (int)n_inputs, init, (int)n_out, res);
  for (unsigned i = 0; i < n_out; i++) res[i].from_mont().to_bytes(out + 32 * i);
  LI_END
}

extern "C" int zkpoa_poseidon_sponge(const uint8_t* inputs, uint64_t n, uint8_t out[32]) {
  if (!inputs || !out || n == 0) return PROVER_ERROR;
  LI_TRY
  std::vector<HFr> in(n);
  load_fr(inputs, n, in.data());
  poseidon_sponge(in.data(), n).from_mont().to_bytes(out);
  LI_END
}

extern "C" int zkpoa_pedersen_commit(const uint8_t secret[32], const uint8_t blinding[32], uint8_t out_xyzt[128]) {
  if (!secret || !blinding || !out_xyzt) return PROVER_ERROR;
  LI_TRY
  store_point(pedersen_commit(U256::from_le(secret), U256::from_le(blinding)), out_xyzt);
  LI_END
}

extern "C" int zkpoa_pedersen_check(const uint8_t secret[32], const uint8_t blinding[32], const uint8_t signals[12 * 32], int* equal) {
  if (!secret || !blinding || !signals || !equal) return PROVER_ERROR;
  LI_TRY
  U256 sig[12];
  for (int i = 0; i < 12; i++) sig[i] = U256::from_le(signals + 32 * i);
  *equal = ed_equal(pedersen_commit(U256::from_le(secret), U256::from_le(blinding)), pedersen_dechunk(sig)) ? 1 : 0;
  LI_END
}

extern "C" int zkpoa_pedersen_decode(const uint8_t signals[12 * 32], uint8_t compressed32[32], int* valid) {
  if (!signals || !compressed32 || !valid) return PROVER_ERROR;
  LI_TRY
  U256 sig[12];
  for (int i = 0; i < 12; i++) sig[i] = U256::from_le(signals + 32 * i);
  *valid = pedersen_decode(sig, compressed32) ? 1 : 0;
  LI_END
}
