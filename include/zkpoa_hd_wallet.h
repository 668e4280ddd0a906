/* libzkpoa_prover.so -- HD-wallet key sources: BIP-32 derivation on the GPU, one child per lane.
 *
 * A custodian holds a hierarchical wallet: a mnemonic or an xprv / xpub, and its deposit addresses are the children
 * m/44'/60'/0'/0/i of one account key. These entry points derive them: SHA-512 and HMAC-SHA512 (batched), the child-key
 * step of BIP-32 for a range of indices under one parent (private: k_i = IL + k_par; public: K_i = IL G + K_par), and on
 * the host the master key of a seed, the seed of a BIP-39 mnemonic, the reading of an extended key and of a path.
 * `ecdsa-sigs-parser sign`, `anon-set` and `hd-list` take their keys through them (--hd-key, --mnemonic, --hd-seed).
 *
 * Conventions. Every 32-byte integer is BIG-endian. A key is the 33-byte "key data" of BIP-32: a private key is
 * 0x00 || k, a public key is 02 / 03 || x (the compressed point); its first byte says which kind it is. An index of
 * 2^31 or more is a hardened child, which only a private parent has.
 *
 * The stance of include/zkpoa_ecdsa_sign.h carries over: NOT hardened against side channels (memory addresses and
 * branches depend on the keys), secrets pass through host memory, made for rehearsals and test data; signing with keys
 * that hold value is the caller's decision. The public (xpub) path holds no secrets: it is the part meant for real
 * wallets (a watch-only listing of the addresses of an account).
 *
 * include/zkpoa_prover.h includes this file: its prototypes are part of the library's C ABI like those declared there.
 */
#ifndef ZKPOA_HD_WALLET_H
#define ZKPOA_HD_WALLET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct zkpoa_context;

/* SHA-512 of n messages of one common length message_len (0..4096 bytes) packed back to back -> n x 64 B; the limits and
 * argument checks of zkpoa_sha256_batch. */
int zkpoa_sha512_batch(struct zkpoa_context* ctx, const void* messages, uint64_t message_len, uint64_t n, void* out64);

/* HMAC-SHA512 of the same kind of batch under ONE key of key_len bytes (0..4096; one above 128 bytes is hashed first, as
 * RFC 2104 says) -> n x 64 B. */
int zkpoa_hmac_sha512_batch(struct zkpoa_context* ctx, const void* key, uint64_t key_len, const void* messages, uint64_t message_len,
                            uint64_t n, void* out64);

/* The children first_index .. first_index + n - 1 of one parent (its key data and its chain code), first_index + n at most
 * 2^32. Out, per child: the key data (n x 33 B: private under a private parent, public under a public one), the chain
 * code (n x 32 B), the public key x || y (n x 64 B), its Ethereum address (n x 20 B) and a status byte: 0 ok; 1 BIP-32's
 * "invalid child" -- IL is not below the group order, the child key is zero, or the child point is the point at
 * infinity (IL = 0 is refused as well, under either kind of parent, so that the two always agree) -- with zeros in every
 * other output of that child: the caller goes on to the next index. A public parent with an index of 2^31 or more
 * anywhere in the range is an error return, and nothing is written; so are a parent key that is not key data (a
 * private key of 0 or not below the group order, a public key that is not on the curve). n = 0 is a no-op. Returns
 * PROVER_OK when it ran, whatever the statuses. zkpoa_last_ms(ctx, 8) is the time of its kernels afterwards. */
int zkpoa_bip32_children(struct zkpoa_context* ctx, const uint8_t* parent_key33, const uint8_t* chain32, uint64_t first_index, uint64_t n,
                         void* out_key33, void* out_chain32, void* out_pubkey_xy, void* out_address20, uint8_t* out_status);

/* The second half of that step alone, on IL values the caller gives (n x 32 B): child i of parent_key33 for tweak IL_i.
 * It is the kernel zkpoa_bip32_children runs after its HMAC kernel; the outputs and the status are the same, without a
 * chain code. */
int zkpoa_bip32_tweak(struct zkpoa_context* ctx, const uint8_t* parent_key33, uint64_t n, const void* tweaks32, void* out_key33,
                      void* out_pubkey_xy, void* out_address20, uint8_t* out_status);

/* Host only. The master key of a seed of 16..64 bytes: I = HMAC-SHA512("Bitcoin seed", seed), key 0x00 || IL, chain code
 * IR. An error return when IL is 0 or not below the group order. */
int zkpoa_bip32_master(const void* seed, uint64_t seed_len, uint8_t* out_key33, uint8_t* out_chain32);

/* Host only. The 64-byte seed of a BIP-39 mnemonic: PBKDF2-HMAC-SHA512, 2048 rounds, password = the mnemonic as given,
 * salt = "mnemonic" || passphrase (both NUL-terminated; passphrase NULL = empty). The word list and the checksum of the
 * mnemonic are NOT checked: any text gives a seed, and a mistyped word gives another wallet without a complaint. Input
 * with a byte outside ASCII is refused (an error return): BIP-39 asks for NFKD normalisation, which is not implemented. */
int zkpoa_bip39_seed(const char* mnemonic, const char* passphrase, uint8_t* out_seed64);

/* Host only. Reads an extended key (xprv... / xpub...: base58check of 78 bytes, versions 0488ADE4 / 0488B21E): the key
 * data, the chain code, and its depth and child index. Checked: the alphabet, the length, the checksum, the version,
 * that a private key's first byte is 0 and the key is in [1, group order), that a public key's first byte is 02 / 03
 * and x is the coordinate of a curve point. The parent-fingerprint field is ignored. (Writing extended keys is not
 * offered: the fingerprint is a RIPEMD-160.) */
int zkpoa_bip32_parse_key(const char* text, uint8_t* out_key33, uint8_t* out_chain32, uint32_t out_depth_index[2]);

/* Host only. Reads a path -- "m", "m/0", "m/44'/60'/0'/0"; h stands for ' -- into its indices (a hardened level has bit
 * 31 set): out_index has room for 255, the most a path may have; *out_levels is how many there are. A level is a decimal
 * number below 2^31. An error return for anything else (an empty level, a trailing slash, 256 levels). */
int zkpoa_bip32_parse_path(const char* path, uint32_t* out_index, uint32_t* out_levels);

/* The key at `path` below the given key (which stands for "m"). Each level is zkpoa_bip32_children with n = 1. A hardened
 * level under a public key is an error; so is a level whose child is invalid (status 1). */
int zkpoa_bip32_derive_path(struct zkpoa_context* ctx, const uint8_t* key33, const uint8_t* chain32, const char* path,
                            uint8_t* out_key33, uint8_t* out_chain32);

#ifdef __cplusplus
}
#endif
#endif /* ZKPOA_HD_WALLET_H */
