/* libzkpoa_prover.so -- the arithmetic of the workflow's last input steps; host only, no context, no GPU.
 *
 * `ecdsa-sigs-parser layer-two-input | layer-three-input | pedersen-check` stand in for the reference's
 * scripts/input_prep_for_layer_two.ts, input_prep_for_layer_three.ts and pedersen_commitment_checker.ts
 * (scripts/full_workflow.sh:521-529, :575-579, :588-591). These four entry points are what those commands compute,
 * exported for callers that hold the values already and for the tests. Integers are 32 bytes, little-endian.
 *
 * include/zkpoa_prover.h includes this file: its prototypes are part of the library's C ABI like those declared there.
 */
#ifndef ZKPOA_LAYER_INPUTS_H
#define ZKPOA_LAYER_INPUTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* circomlibjs `poseidon(inputs, initState, nOut)` over the BN254 scalar field: the state [init_state, inputs...] of width
 * t = n_inputs + 1 (n_inputs = 1..16), x^5, 8 full rounds and circomlib's partial rounds for that t, constants and MDS
 * matrix from the Grain generator; out <- the first n_out (1..t) state elements. PROVER_ERROR for a count out of range
 * or a value that is not below the field's order. A width's parameters are generated on its first use. */
int zkpoa_poseidon_hash(const uint8_t* inputs, unsigned n_inputs, const uint8_t init_state[32], unsigned n_out, uint8_t* out);

/* `poseidonSponge` of input_prep_for_layer_two.ts:46-79 over n > 0 field elements: 16 inputs per round, the previous
 * round's first state element as the next initial state, the second state element of the last round as the hash; the
 * last round reads its inputs at (round index) * (n mod 16) when n is no multiple of 16, as the reference does. */
int zkpoa_poseidon_sponge(const uint8_t* inputs, uint64_t n, uint8_t out[32]);

/* scripts/lib/pedersen_commitment.ts on ed25519: secret * G + blinding * H in extended coordinates (x, y, z, t), each
 * the least residue mod 2^255 - 19, computed with the reference's additions in the reference's order. */
int zkpoa_pedersen_commit(const uint8_t secret[32], const uint8_t blinding[32], uint8_t out_xyzt[128]);

/* *equal <- is that commitment the point of the layer-three circuit's first 12 public signals (three 85-bit chunks per
 * coordinate, least significant first), compared projectively as `pointEqual` does */
int zkpoa_pedersen_check(const uint8_t secret[32], const uint8_t blinding[32], const uint8_t signals[12 * 32], int* equal);

#ifdef __cplusplus
}
#endif
#endif /* ZKPOA_LAYER_INPUTS_H */
