/* libzkpoa_prover.so -- ECDSA signing on the GPU: what `ecdsa-sigs-parser sign` and `anon-set` compute.
 *
 * The workflow of the reference begins with two files, signatures.json and anonymity_set.csv, that its
 * tests/generate_ecdsa_signatures.ts (noble-secp256k1's sign, at most 128 keys, one thread) and tests/generate_anon_set.ts
 * make. These entry points are the arithmetic of those two: SHA-256, public keys and addresses, the RFC 6979 nonce and
 * the signature, one key per GPU lane. Host buffers, nothing kept between calls. Every 32-byte integer (keys, hashes, k,
 * r, s, x, y) is BIG-endian, as with zkpoa_ecdsa_star.
 *
 * NOT hardened against side channels: memory addresses and branches depend on the key and the nonce. Keys pass through
 * host memory. Made for rehearsals and test data; signing with keys that hold value is the caller's decision.
 *
 * include/zkpoa_prover.h includes this file: its prototypes are part of the library's C ABI like those declared there.
 * (zkpoa_sha256 without a context, declared there, is the host's one-message SHA-256; this one is batched.)
 */
#ifndef ZKPOA_ECDSA_SIGN_H
#define ZKPOA_ECDSA_SIGN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct zkpoa_context;

/* SHA-256 of n messages of one common length message_len (0..4096 bytes) packed back to back -> n x 32 B; the limits and
 * argument checks of zkpoa_keccak256. */
int zkpoa_sha256_batch(struct zkpoa_context* ctx, const void* messages, uint64_t message_len, uint64_t n, void* out32);

/* Q = d G for n secret keys (n x 32 B): x || y (n x 64 B), the Ethereum address (n x 20 B) and a status byte: 0 ok;
 * 1 the key is zero or not below the group order, with zeros in the other outputs. n = 0 is a no-op. */
int zkpoa_secp256k1_pubkey(struct zkpoa_context* ctx, uint64_t n, const void* seckeys, void* out_pubkey_xy, void* out_address20,
                           uint8_t* out_status);

/* The keys of `--generate-keys`: d_i = (SHA-256(seed || be64(i)) mod (n - 1)) + 1 for i = first .. first + n - 1 (be64: the
 * index as 8 big-endian bytes) -> n x 32 B, every one in [1, group order). seed_len 0..4096. */
int zkpoa_secp256k1_derive_keys(struct zkpoa_context* ctx, const void* seed, uint64_t seed_len, uint64_t first, uint64_t n,
                                void* out_seckeys);

/* The RFC 6979 nonce candidate (HMAC-SHA256 DRBG, section 3.2, no extra entropy) of n keys, each with its own message
 * hash (n x 32 B; reduced modulo the group order as bits2octets says), after `skip` candidates have been refused:
 * skip = 0 is the nonce zkpoa_ecdsa_sign uses. The candidate is returned whether or not it is in [1, group order), and
 * the key is hashed as given. skip is at most 64. */
int zkpoa_rfc6979_nonce(struct zkpoa_context* ctx, uint64_t n, const void* seckeys, const void* msghash, uint32_t skip, void* out_k);

/* n signatures (n = 0 .. 2^32). msghash: one 32-byte hash for all keys (msghash_stride 0) or one per key (msghash_stride
 * 32); any other stride is an error. Out: r, s (n x 32 B each, s at most (group order - 1) / 2), v (27 / 28: 27 + the
 * parity of the nonce point's y, flipped when s was replaced by its negative), the public key x || y (n x 64 B), its
 * address (n x 20 B) and a status byte: 0 ok; 1 the key is zero or not below the group order; 2 the nonce point's x is
 * not below the group order (probability 2^-128; 27 / 28 cannot express it). A status other than 0 comes with zeros in
 * every other output of that key. Returns PROVER_OK when it ran, whatever the statuses. zkpoa_last_ms(ctx, 8) is the
 * time of its kernels afterwards. */
int zkpoa_ecdsa_sign(struct zkpoa_context* ctx, uint64_t n, const void* seckeys, const void* msghash, uint64_t msghash_stride,
                     void* out_r, void* out_s, uint8_t* out_v, void* out_pubkey_xy, void* out_address20, uint8_t* out_status);

#ifdef __cplusplus
}
#endif
#endif /* ZKPOA_ECDSA_SIGN_H */
