/* libzkpoa_prover.so -- the owned leaves of an anonymity set at the prover's scale: where they are, and their paths.
 *
 * zkpoa_merkle_path (include/zkpoa_prover.h) is the single-leaf form: one 32-byte copy per level. A custodian with 2^20
 * accounts under a height-24 tree needs 25 M of those; the entry points below locate any number of leaves through the
 * stable index of include/zkpoa_audit.h and gather all their paths with one kernel. Integers are 32 bytes,
 * little-endian, standard form.
 *
 * include/zkpoa_prover.h includes this file: its prototypes are part of the library's C ABI like those declared there.
 */
#ifndef ZKPOA_MERKLE_PATHS_H
#define ZKPOA_MERKLE_PATHS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Lookup through the stable index. d_keys (n x 32 B) and d_perm are exactly what zkpoa_anon_set_index_device took and
 * produced; d_queries is m x 32 B in the same form; d_first and d_count are m words each. All are device pointers.
 * d_count[i] <- the number of rows whose key equals query i; d_first[i] <- the lowest such row (the index is stable: the
 * first of the equal run), 0xFFFFFFFF when there is none. Exact for every input: keys compare as 256-bit little-endian
 * integers, most significant limb first, which is the index's order; no hashing. One lane per query, a lower-bound and
 * an upper-bound binary search over keys[perm[.]]; an entry of d_perm that is no row number (>= n) is never followed
 * into the keys: the query that meets one reports no match. n < 2^32, m < 2^32. m = 0 is a no-op; with n = 0 every
 * count is 0 and nothing but the outputs is touched. zkpoa_last_ms id 10 = the kernel of the last call. */
int zkpoa_anon_set_find_device(zkpoa_context* ctx, const void* d_keys, uint64_t n, const uint32_t* d_perm,
                               const void* d_queries, uint64_t m, uint32_t* d_first, uint32_t* d_count);

/* The same over a resident tree: leaf_hashes (host, m x 32 B) are looked up among the tree's first n_set stored leaves
 * (zkpoa_merkle_info's out[0]); first and count are host buffers of m words. Padding leaves are never searched: a query
 * of 32 zero bytes has count 0 even when the tree is padded. The index of those leaves is built on the first call, kept
 * in the handle (4 B per row) and released by zkpoa_merkle_free; a later call does not sort again.
 * zkpoa_last_ms id 10 = the kernels of the call (the first one's include the index). */
int zkpoa_merkle_find(zkpoa_context* ctx, zkpoa_merkle* tree, const void* leaf_hashes, uint64_t m, uint32_t* first,
                      uint32_t* count);

/* The sibling paths of m leaves, host buffers. paths_le: m x k x 32 B with k the path length of zkpoa_merkle_info;
 * element (i, l) is node (leaf_index[i] >> l) ^ 1 of level l -- the bytes and the order of m calls of zkpoa_merkle_path.
 * path_indices: optional, m x k bytes, bit l of the index at position l. Padding leaves are valid indices; an index
 * >= 2^k is refused with PROVER_ERROR before anything is launched. The work goes in rounds of at most 2^16 indices, so
 * device memory does not grow with m. k = 0 (a one-row set) or m = 0: PROVER_OK, nothing is written.
 * zkpoa_last_ms id 10 = the gather kernels of the call. */
int zkpoa_merkle_paths(zkpoa_context* ctx, const zkpoa_merkle* tree, const uint64_t* leaf_index, uint64_t m,
                       uint8_t* paths_le, uint8_t* path_indices);

/* The kernel alone: d_leaf_index (m x 8 B) and d_paths (m x k x 32 B, 16-byte aligned) are device pointers. For an index
 * >= 2^k it writes k x 32 zero bytes and reads nothing. m x k < 2^37. */
int zkpoa_merkle_paths_device(zkpoa_context* ctx, const zkpoa_merkle* tree, const uint64_t* d_leaf_index, uint64_t m,
                              void* d_paths);

#ifdef __cplusplus
}
#endif
#endif /* ZKPOA_MERKLE_PATHS_H */
