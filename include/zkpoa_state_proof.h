/* libzkpoa_prover.so -- the anonymity set against an Ethereum state root.
 *
 * The reference's README leaves the verifier to "check that anonymity set matches on-chain data". A block header commits
 * to a state root, and `eth_getProof` returns, per address, the Merkle-Patricia trie nodes that tie the account's
 * balance to that root. These entry points check such proofs on the device: Keccak-256 of every node (one lane per node)
 * and the walk along the key's 64 nibbles (one lane per item).
 *
 * Input layout of the node arguments, the same for zkpoa_mpt_verify and zkpoa_eth_account_proofs (host buffers):
 *   nodes         one blob of nodes_bytes bytes; every node starts on an 8-byte boundary (what lies between nodes is
 *                 never looked at)
 *   node_offset   T x u64, each a multiple of 8, not descending
 *   node_length   T x u32, at most 2^20 each (one lane hashes one node), node_offset[k] + node_length[k] <= nodes_bytes
 *   first_node    (n + 1) x u64, not descending, first_node[0] = 0 and first_node[n] = T: item i owns the nodes
 *                 first_node[i] .. first_node[i + 1] - 1, in root-to-leaf order
 * T and n are below 2^32. A layout that breaks one of these rules is PROVER_ERROR (zkpoa_last_error says which) before
 * anything is launched, and no output is written.
 *
 * Per-item status (ABI; the first failing condition in walk order wins) and `where`, the index within the item's proof
 * of the node at which the status arose (for ZKPOA_MPT_SHORT the index the missing node would have, the proof's length): */
#ifndef ZKPOA_STATE_PROOF_H
#define ZKPOA_STATE_PROOF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZKPOA_MPT_PRESENT    0u   /* the key is in the trie; its value's span is returned */
#define ZKPOA_MPT_ABSENT     1u   /* proven absent: an empty branch slot, or an extension or leaf whose path diverges */
#define ZKPOA_MPT_NO_NODES   2u   /* no nodes (ZKPOA_MPT_ABSENT instead when the root is the empty-trie root 56e81f17...b421) */
#define ZKPOA_MPT_HASH       3u   /* a node's hash differs from the reference that names it (node 0: from the root) */
#define ZKPOA_MPT_RLP        4u   /* malformed RLP: not a list of 2 or 17 items, or a length that leaves the node */
#define ZKPOA_MPT_CHILD      5u   /* a child reference that is neither empty nor a 32-byte string (embedded nodes are refused) */
#define ZKPOA_MPT_SHORT      6u   /* the proof ends although a reference is still to be followed */
#define ZKPOA_MPT_LONG       7u   /* nodes follow after the walk has ended */
#define ZKPOA_MPT_HEX_PREFIX 8u   /* flag nibble above 3, non-zero pad nibble, empty path item, a path longer than the
                                     key's remainder, or a branch reached with the key used up */
#define ZKPOA_MPT_ACCOUNT    9u   /* (account form) the value is not an account */

#define ZKPOA_MPT_KEY32      0    /* keys: n x 32 B, the trie keys themselves */
#define ZKPOA_MPT_ADDRESS20  1    /* keys: n x 20 B addresses; the trie key is Keccak-256 of each */

/* The generic form. out_status: n bytes; out_where: n x u32; out_value_span: n x 2 x u64 = (offset into `nodes`,
 * length) of the value for status 0, zero otherwise. n = 0 is a no-op. zkpoa_last_ms id 8 = the kernels. */
int zkpoa_mpt_verify(zkpoa_context* ctx, uint64_t n, const void* keys, int key_kind, const uint8_t* root32,
                     const void* nodes, uint64_t nodes_bytes, const uint64_t* node_offset, const uint32_t* node_length,
                     const uint64_t* first_node, uint8_t* out_status, uint32_t* out_where, uint64_t* out_value_span);

/* The account trie: the key is Keccak-256 of the 20-byte address and the value must be a list of 4 strings -- nonce (at
 * most 8 bytes), balance (at most 32), neither with a leading zero byte, storage root and code hash (32 each) -- else
 * ZKPOA_MPT_ACCOUNT. out_nonce: n x u64; out_balance32: n x 32 B big-endian; out_storage_root32, out_code_hash32:
 * optional (NULL), n x 32 B. All are zero unless the status is 0. */
int zkpoa_eth_account_proofs(zkpoa_context* ctx, uint64_t n, const void* address20, const uint8_t* root32,
                             const void* nodes, uint64_t nodes_bytes, const uint64_t* node_offset, const uint32_t* node_length,
                             const uint64_t* first_node, uint8_t* out_status, uint32_t* out_where, uint64_t* out_nonce,
                             void* out_balance32, void* out_storage_root32, void* out_code_hash32);

/* Host only, no context. A block header's RLP -> its hash (Keccak-256 of the bytes: what an explorer shows), the state
 * root (item 3) and the number (item 8). PROVER_ERROR for anything that is not exactly one list of at least 9 strings
 * with items 0, 1, 3, 4, 5 of 32 bytes, item 2 of 20, item 6 of 256, item 7 of at most 32 and item 8 of at most 8. */
int zkpoa_eth_block_header(const uint8_t* rlp, uint64_t len, uint8_t* hash32, uint8_t* state_root32, uint64_t* number);

/* The whole check of a published set against a state root. zkpoa-audit's fifth check: */
#define ZKPOA_ASSETS_STATE      0x10u  /* a row without a valid proof, or whose balance is not the chain's */
#define ZKPOA_STATE_BAD_NO_PROOF 1u    /* first_bad_kind: the file holds no proof for the row's address */
#define ZKPOA_STATE_BAD_PROOFS   2u    /* every proof of the row failed; first_bad_status / first_bad_where: the first read */
#define ZKPOA_STATE_BAD_BALANCE  3u    /* a valid proof gives another balance (or absence, and the csv balance is not 0) */
typedef struct {
  uint64_t rows, proven_present, proven_absent;   /* rows whose proof and balance are good */
  uint64_t rows_without_proof, rows_failed, rows_differ;   /* the three ways a row is bad */
  uint64_t proofs_read, proofs_not_in_set;   /* proofs for addresses not in the set are counted and ignored */
  uint64_t first_bad_row;                    /* the lowest bad row, ~0 when every row is good */
  uint32_t first_bad_kind, first_bad_status, first_bad_where;
  uint32_t first_diff_absent;                /* 1: the first differing row is proven absent */
  uint64_t first_diff_row;                   /* the lowest row of kind 3, ~0 when there is none */
  uint8_t first_diff_chain_balance32[32];    /* its balance on the chain in wei, big-endian */
  float kernel_ms;                           /* the hash, walk and account kernels of all slabs */
} zkpoa_state_report;
/* addresses / balances: host buffers, n x 32 B little-endian, as zkpoa_assets_verify takes them. proofs_path: JSON
 * Lines, one `eth_getProof(address, [], block)` result per line, bare or inside its JSON-RPC envelope under "result";
 * only "address" and "accountProof" are read (a claimed "balance" is not trusted). unit_divisor: 1 (the csv is in wei),
 * 10^9 (gwei) or 10^18 (ether). A row is good when a proof of its address has status 0 and
 * floor(chain balance / unit_divisor) equals the csv balance, or has status 1 and the csv balance is 0. Of several rows
 * with one address only the first is matched: the others count as without proof (the duplicate check names them).
 * The file is streamed in slabs: device memory does not grow with it. Every row is examined whatever the others gave;
 * only an unreadable or malformed file (the message names the line) is PROVER_ERROR -- a bad proof is a finding. */
int zkpoa_anon_set_state_check_file(zkpoa_context* ctx, const void* addresses, const void* balances, uint64_t n,
                                    const char* proofs_path, const uint8_t* root32, uint64_t unit_divisor,
                                    zkpoa_state_report* report);

#ifdef __cplusplus
}
#endif
#endif /* ZKPOA_STATE_PROOF_H */
