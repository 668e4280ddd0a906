/* libzkpoa_prover.so -- the verifier's side of the protocol.
 *
 * The prover publishes a proof, the anonymity set and a commitment. The verifier rebuilds the Merkle root from the set,
 * checks that the proof's public signals name that root and that commitment, and verifies the proof. The reference has
 * no program for this ("Verifier: script still needs to be written", its README); `zkpoa-audit` is that program and
 * these four entry points are what it computes. Integers are 32 bytes, little-endian, standard form.
 *
 * include/zkpoa_prover.h includes this file: its prototypes are part of the library's C ABI like those declared there.
 */
#ifndef ZKPOA_AUDIT_H
#define ZKPOA_AUDIT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* d_perm[0..n) <- the row numbers ordered by (address ascending, row ascending): a STABLE sort of the n keys, exact for
 * every input (an LSD radix sort over the key's bytes; no hashing). Keys: n x 32 B little-endian standard form, as
 * zkpoa_merkle_build_device takes addresses (any 256-bit value, not only 160-bit ones). d_addresses and d_perm are
 * device pointers. n < 2^32; n = 0 is a no-op. zkpoa_last_ms id 9 = the kernels of the last call. */
int zkpoa_anon_set_index_device(zkpoa_context* ctx, const void* d_addresses, uint64_t n, uint32_t* d_perm);

/* Host buffers. out[0] = rows whose address equals that of an EARLIER row (0 = no duplicates),
 * out[1], out[2] = the pair (i < j) with the smallest j among those rows (both ~0 when out[0] = 0),
 * out[3] = 1 when the file is already in strictly ascending address order, else 0 (1 for n < 2). */
int zkpoa_anon_set_audit(zkpoa_context* ctx, const void* addresses, uint64_t n, uint64_t out[4]);

/* Host only, no context. The layer-three circuit's first 12 public signals (three 85-bit chunks per coordinate, least
 * significant first) -> the point they spell. *valid = 0 when a signal is >= 2^85, Z = 0, or (X, Y, Z, T) is not on
 * ed25519 in extended coordinates (-X^2 + Y^2 = Z^2 + d T^2 and X Y = Z T, mod 2^255 - 19); compressed32 is zero then.
 * Otherwise compressed32 <- the RFC 8032 encoding of the affine point (y little-endian, bit 255 = x's low bit).
 * Torsion is NOT checked: a point of the curve outside the prime-order subgroup is reported valid. */
int zkpoa_pedersen_decode(const uint8_t signals[12 * 32], uint8_t compressed32[32], int* valid);

/* The verifier's whole job in one call: the set's duplicate check and Merkle root on the device, the root and the
 * commitment bound to public.json, the Groth16 verification. *failed_checks <- the checks that failed: */
#define ZKPOA_ASSETS_SET        0x1u   /* duplicate addresses (or an empty set) */
#define ZKPOA_ASSETS_ROOT       0x2u   /* public[12] != root of the set; also when public.json has != 13 signals */
#define ZKPOA_ASSETS_COMMITMENT 0x4u   /* signals 0..11 are no valid point, or differ from expected_commitment */
#define ZKPOA_ASSETS_PROOF      0x8u   /* zkpoa_groth16_verify says invalid */
typedef struct {
  uint8_t root_le[32];     /* the root of the set (zero for an empty set) */
  uint8_t commitment[32];  /* zkpoa_pedersen_decode of signals 0..11 (zero when they are no valid point) */
  uint64_t rows, duplicate_rows, first_dup[2];   /* as zkpoa_anon_set_audit's out[0..2] */
  int ascending;                                 /* its out[3] */
} zkpoa_assets_report;
/* PROVER_OK means every check ran (each runs whatever the others found); only malformed JSON, or a field element >= r in
 * the set, is PROVER_ERROR (zkpoa_last_error says which). addresses / balances: host buffers, n x 32 B each.
 * expected_commitment32: optional (NULL: only the point's validity is checked). report: optional. */
int zkpoa_assets_verify(zkpoa_context* ctx, const void* addresses, const void* balances, uint64_t n,
                        const char* vkey_json, const char* public_json, const char* proof_json,
                        const uint8_t* expected_commitment32, uint32_t* failed_checks, zkpoa_assets_report* report);

#ifdef __cplusplus
}
#endif
#endif /* ZKPOA_AUDIT_H */
