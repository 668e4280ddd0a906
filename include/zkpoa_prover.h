/* libzkpoa_prover.so -- C ABI of the MI355X (gfx950) Groth16 prover for zk-proof-of-assets.
 *
 * Drop-in boundary. The reference has an EXEC boundary, not an FFI:
 *   scripts/g16_prove.sh:248-252   "$rapidsnark_path" zkey witness.wtns proof.json public.json
 *   scripts/g16_prove.sh:255-259   npx snarkjs groth16 prove   (same four positional arguments)
 * The `prover` executable built from this library takes exactly that argv. The library
 * entry points below are what an FFI binding for the same step would bind; the first two
 * mirror iden3/rapidsnark's prover.h (the C API of the binary the reference execs), the
 * zkpoa_* ones expose the stages of the path for device-resident use and for parity tests.
 *
 * Conventions: plain C types, caller-allocated buffers, no global state except what hangs
 * off a zkpoa_context. All byte formats are the reference's wire formats:
 *   Fq/Fr element : 32 bytes little-endian
 *   G1 point      : 64 bytes  = x||y, affine, Montgomery form (R = 2^256), infinity = zeros
 *   G2 point      : 128 bytes = x.c0||x.c1||y.c0||y.c1, same conventions
 *   scalar        : 32 bytes little-endian, standard (non-Montgomery) form, < r
 * exactly as in .zkey sections 5-9 and .wtns section 2.
 *
 * The compute path is HIP-only: every function that needs the GPU fails with an error
 * (never falls back to the CPU) when no gfx950 device is usable.
 */
#ifndef ZKPOA_PROVER_H
#define ZKPOA_PROVER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes: same values as rapidsnark prover.h ---------------------------------- */
#define PROVER_OK 0x0
#define PROVER_ERROR 0x1
#define PROVER_ERROR_SHORT_BUFFER 0x2
#define PROVER_INVALID_WITNESS_LENGTH 0x3
/* Extension (not in rapidsnark): the failure came from the HIP runtime (sticky GPU fault, lost device, out of device or
 * host memory), not from the inputs -- the process's GPU context cannot be trusted any more. Returned by the two
 * groth16_prover* entry points; callers that only test != PROVER_OK are unaffected. */
#define PROVER_ERROR_RUNTIME 0x4

/* ---- one-shot prove: replaces the process exec'd at scripts/g16_prove.sh:248-252 -------- */
/* zkey / wtns are complete file images. proof_buffer / public_buffer receive NUL-terminated
 * JSON text; *proof_size / *public_size are in: capacity, out: bytes needed incl. NUL (also
 * on PROVER_ERROR_SHORT_BUFFER). JSON style is rapidsnark's unless env ZKPOA_JSON=snarkjs.
 * r, s come from /dev/urandom unless env ZKPOA_R / ZKPOA_S (decimal) are set.
 * Self-check: like the reference, which verifies every proof right after proving it (scripts/g16_verify.sh:213-216),
 * the first proof of every key is verified against the verification key the zkey itself carries (sections 2-3)
 * before anything is returned; a failure is PROVER_ERROR with a message. Env ZKPOA_SELFCHECK=0 disables it,
 * =all checks every proof (host only, ~7 ms). */
int groth16_prover(const void* zkey_buffer, unsigned long zkey_size,
                   const void* wtns_buffer, unsigned long wtns_size,
                   char* proof_buffer, unsigned long* proof_size,
                   char* public_buffer, unsigned long* public_size,
                   char* error_msg, unsigned long error_msg_maxsize);

/* Same, reading the zkey from a path (mmap) -- what the `prover` CLI uses. */
int groth16_prover_zkey_file(const char* zkey_file_path,
                             const void* wtns_buffer, unsigned long wtns_size,
                             char* proof_buffer, unsigned long* proof_size,
                             char* public_buffer, unsigned long* public_size,
                             char* error_msg, unsigned long error_msg_maxsize);

/* Same again with BOTH inputs as paths -- exactly the argv of the process exec'd at scripts/g16_prove.sh:248-252
 * (`prover <zkey> <wtns> ...`), and what the `prover` executable calls. Extension (rapidsnark's prover.h has no such
 * entry): the witness is never mapped or copied on the host -- its values go from the page cache straight into the
 * pinned staging buffers of the upload (pread), which at the layer-three size (1.7 GB .wtns) saves the ~50 ms a mapping
 * costs to populate and tear down. Same return codes, buffers and environment as groth16_prover_zkey_file. */
int zkpoa_groth16_prover_files(const char* zkey_file_path, const char* wtns_file_path,
                               char* proof_buffer, unsigned long* proof_size,
                               char* public_buffer, unsigned long* public_size,
                               char* error_msg, unsigned long error_msg_maxsize);

/* Per-thread request options for the three entry points above. They read r, s (ZKPOA_R / ZKPOA_S, decimal; test use),
 * the JSON style (ZKPOA_JSON=snarkjs) and verbosity (ZKPOA_VERBOSE) from the environment; a host that serves several
 * requests from several threads (the `prover` executable's resident server does) cannot change its environment per
 * request. After zkpoa_set_thread_options the CALLING THREAD's following calls use these values instead: a NULL string /
 * verbose 0 means "unset for this thread, whatever the environment says". zkpoa_clear_thread_options returns the thread
 * to the environment. Calls from different threads may overlap: a request on a resident key stages its witness while
 * the previous request is still proving. */
int zkpoa_set_thread_options(const char* r_decimal, const char* s_decimal, const char* json_style, int verbose);
int zkpoa_clear_thread_options(void);

/* "The host has nothing to do right now." groth16_prover_zkey_file / zkpoa_groth16_prover_files keep keys resident
 * (env ZKPOA_KEY_CACHE) and prove ~10 % faster once a key has its fixed-base tables, but building them is seconds of GPU
 * time at the layer-two / -three sizes -- so by default (ZKPOA_PRECOMP unset or "idle") that never happens inside a
 * request: each call of zkpoa_idle_work builds ONE table of the most recently used key that still lacks some and returns
 * 1 (call again while idle), or returns 0 at once when there is nothing to do or a request is in flight. The `prover`
 * server calls it after 300 ms without a request. A host that never calls it gets the whole set built inside the request
 * that follows a key's ZKPOA_PRECOMP_AFTER-th proof (default 64). ZKPOA_PRECOMP=eager: at the second use, inside the
 * request (r03); =0: never. */
int zkpoa_idle_work(void);

/* ---- context ----------------------------------------------------------------------------- */
typedef struct zkpoa_context zkpoa_context;
typedef struct zkpoa_zkey zkpoa_zkey;

/* Creates a context on HIP device `device` (streams + workspace). Fails if no GPU.
 * Threads: a context is not re-entrant -- calls on one context must not overlap, with one exception: the lane-addressed
 * MSM calls (zkpoa_msm_g1_device_lane, zkpoa_msm_table_run_lane) may run concurrently on DISTINCT lanes. Use one
 * context per host thread (or per GPU) otherwise; the one-shot groth16_prover* entry points serialise themselves. */
int zkpoa_context_create(int device, zkpoa_context** ctx, char* error_msg, unsigned long error_msg_maxsize);
void zkpoa_context_destroy(zkpoa_context* ctx);
/* message of the last failing call on this context (valid until the next call) */
const char* zkpoa_last_error(const zkpoa_context* ctx);

/* ---- device-resident proving key: replaces snarkjs readSection(zkey, 4..9) per prove ------ */
/* Parses the binfile container and uploads sections 4-9 to HBM once. */
int zkpoa_zkey_load(zkpoa_context* ctx, const void* zkey_buffer, unsigned long zkey_size, zkpoa_zkey** zkey);
void zkpoa_zkey_free(zkpoa_context* ctx, zkpoa_zkey* zkey);
/* header fields: out[0]=nVars, out[1]=nPublic, out[2]=domainSize, out[3]=nCoefs */
int zkpoa_zkey_info(const zkpoa_zkey* zkey, uint64_t out[4]);

/* Full prove against a resident key: groth16_prove.js steps 2-7.
 * r_le / s_le: 32-byte little-endian standard-form scalars, or NULL for /dev/urandom.
 * proof_points: 64 (pi_a) + 128 (pi_b) + 64 (pi_c) bytes, wire format above.
 * public_le: nPublic * 32 bytes (w[1..nPublic], standard form). */
int zkpoa_prove(zkpoa_context* ctx, const zkpoa_zkey* zkey,
                const void* wtns_buffer, unsigned long wtns_size,
                const uint8_t* r_le, const uint8_t* s_le,
                uint8_t proof_points[256], uint8_t* public_le, unsigned long public_capacity);

/* Same two calls for data that already lives in HBM (what bench.py times for the prove workloads;
 * also the hook for a device-native zkey cache). The five point sections stay owned
 * by the caller and must outlive the handle; d_coef_records = n_coefs 44-byte records of section 4;
 * header_points = alpha1(64) beta1(64) beta2(128) delta1(64) delta2(128), wire format. */
int zkpoa_zkey_load_device(zkpoa_context* ctx, uint64_t n_vars, uint64_t n_public, unsigned log_domain,
                           const void* d_A, const void* d_B1, const void* d_B2, const void* d_C, const void* d_H,
                           const void* d_coef_records, uint64_t n_coefs, const uint8_t header_points[448],
                           zkpoa_zkey** zkey);
/* One rank's shard of a key whose sections are already in HBM (bench.py --gpus N generates only its own ranges of
 * the synthetic key; a device-native zkey cache would hand over what it keeps per GPU). Same arguments, but with
 * world > 1 the buffers hold only what zkpoa_zkey_load_shard / _load_shard_split would upload for this rank:
 * d_A, d_B1, d_B2 the wires [lo, lo + cnt) of sections 5-7 and d_C the same split of section 8, where for n items
 * lo = rank * (n / world) + min(rank, n % world), cnt = n / world + (rank < n % world); d_H that range of section 9,
 * or with split != 0 the cyclic shard H[t * world + rank], t < domain / world (copied: the handle owns its copy);
 * d_coef_records all n_coefs records, or with split != 0 at least those of the constraints c = rank (mod world)
 * (others are ignored). The handle is a shard: zkpoa_prove_partials (+ the split stages) and zkpoa_prove_assemble.
 * `split` is a set of shard flags (below): 1 = ZKPOA_SHARD_SPLIT_CHAIN as before; with ZKPOA_SHARD_BLOCK_CYCLIC(L)
 * d_A, d_B1, d_B2, d_C hold this rank's blocks of 2^L items (block b = rank mod world), concatenated. */
int zkpoa_zkey_load_device_shard(zkpoa_context* ctx, uint64_t n_vars, uint64_t n_public, unsigned log_domain,
                                 uint64_t rank, uint64_t world, int split, const void* d_A, const void* d_B1,
                                 const void* d_B2, const void* d_C, const void* d_H, const void* d_coef_records,
                                 uint64_t n_coefs, const uint8_t header_points[448], zkpoa_zkey** zkey);
/* d_witness: n_vars x 32 B standard form on the device (w[0] = 1). */
int zkpoa_prove_device(zkpoa_context* ctx, const zkpoa_zkey* zkey, const void* d_witness,
                       const uint8_t* r_le, const uint8_t* s_le,
                       uint8_t proof_points[256], uint8_t* public_le, unsigned long public_capacity);

/* ---- one proof sharded over several GPUs (BASELINE.json configs[3]) -------------------
 * The five MSMs shard by contiguous index ranges; one process per GPU owns shard `rank` of `world`:
 *   zkpoa_zkey_load_shard   uploads only that rank's byte range of zkey sections 5-9 (coefficients and
 *                           the H-scalar chain are replicated; see the split chain below for sharding them);
 *   zkpoa_zkey_set_shard    restricts a fully resident key (zkpoa_zkey_load / _load_device) to a shard;
 *   zkpoa_prove_partials    -> partials = A(64) B1(64) B2(128) C(64) H(64): the shard's five MSM results;
 *   (the caller all-gathers the 384 bytes over RCCL and sums component-wise: zkpoa_g1_sum / zkpoa_g2_sum)
 *   zkpoa_prove_assemble    host only: header_points (zkpoa_zkey_header) + summed partials + r, s -> proof.
 * RCCL has no elliptic-curve reduction operator, so "all-reduce of partial sums" = all-gather + local add. */
int zkpoa_zkey_load_shard(zkpoa_context* ctx, const void* zkey_buffer, unsigned long zkey_size,
                          uint64_t rank, uint64_t world, zkpoa_zkey** zkey);
/* Shard flags (zkpoa_zkey_load_shard_ex, and the `split` argument of zkpoa_zkey_load_device_shard):
 *   ZKPOA_SHARD_SPLIT_CHAIN      the H-scalar chain is split over the ranks too (what zkpoa_zkey_load_shard_split does);
 *   ZKPOA_SHARD_BLOCK_CYCLIC(L)  sections 5-8 are dealt out in blocks of 2^L consecutive items (wires for A / B1 / B2,
 *                                section indices for C), block b to rank b mod world, instead of one contiguous range
 *                                per rank: real witnesses cluster (runs of bits, runs of full-width limbs), and equal
 *                                index ranges are then unequal work. Every block is still one contiguous byte range of
 *                                the file. L in 4..24; ZKPOA_SHARD_BLOCK_DEFAULT = blocks of 2^16.
 * The multi-GPU path of groth16_prover_zkey_file (env ZKPOA_DEVICES) loads its shards with both. */
#define ZKPOA_SHARD_SPLIT_CHAIN 0x1
#define ZKPOA_SHARD_BLOCK_CYCLIC(L) (((L) & 0xff) << 8)
#define ZKPOA_SHARD_BLOCK_LOG(flags) ((unsigned)(((flags) >> 8) & 0xff))
#define ZKPOA_SHARD_BLOCK_DEFAULT ZKPOA_SHARD_BLOCK_CYCLIC(16)
int zkpoa_zkey_load_shard_ex(zkpoa_context* ctx, const void* zkey_buffer, unsigned long zkey_size,
                             uint64_t rank, uint64_t world, int flags, zkpoa_zkey** zkey);
int zkpoa_zkey_set_shard(zkpoa_zkey* zkey, uint64_t rank, uint64_t world);
int zkpoa_zkey_header(const zkpoa_zkey* zkey, uint8_t header_points[448]);
int zkpoa_prove_partials(zkpoa_context* ctx, const zkpoa_zkey* zkey, const void* wtns_buffer, unsigned long wtns_size,
                         uint8_t partials[384], uint8_t* public_le, unsigned long public_capacity);
int zkpoa_prove_partials_device(zkpoa_context* ctx, const zkpoa_zkey* zkey, const void* d_witness,
                                uint8_t partials[384]);
int zkpoa_prove_assemble(const uint8_t header_points[448], const uint8_t partial_sums[384],
                         const uint8_t* r_le, const uint8_t* s_le, uint8_t proof_points[256]);

/* ---- the H-scalar chain split over the same ranks (SURVEY.md 8e rows NTT / buildABC / joinABC) -------
 * Replaces, per rank, 1/world of snarkjs groth16_prove.js buildABC1 + 3 x (Fr.ifft, batchApplyKey, Fr.fft)
 * + joinABC. world = G in {2, 4, 8}, G^2 <= domain n, M = n / G, Q = M / G.
 * Rank g owns the constraint rows c = g (mod G) and ends with the H scalars of the odd-coset indices
 * i = g (mod G); its H points are the cyclic shard H[t*G + g], so no scalar ever moves after stage 3.
 * Each transform is a four-step NTT with ONE all-to-all (2 per proof for ifft -> shift -> fft of all three
 * polynomials together):
 *   zkpoa_witness_load       parse a .wtns and upload it into the key's witness buffer (every rank: replicated)
 *   zkpoa_split_stage1       buildABC on the rank's rows + size-M inverse DIF of A, B, C -> d_exchange
 *   [caller: ONE all-to-all with equal splits over the whole buffer (RCCL all_to_all_single)]
 *   zkpoa_split_stage2       twiddle, size-G DFT, coset scale inc^k / n, size-G DFT, twiddle: d_received -> d_exchange
 *   [caller: the same all-to-all again]
 *   zkpoa_split_stage3       size-M forward DIT of A, B, C + joinABC -> H scalars kept on the key handle
 *   zkpoa_prove_partials_device(ctx, key, NULL, partials)   the five MSMs of the shard (H: cyclic shard)
 * d_exchange / d_received: caller-owned device buffers of 3 * M * 32 bytes laid out [G ranks][3 polynomials A, B, C]
 * [Q elements]: the contiguous chunk h (3 * Q * 32 bytes) is what rank h receives, e.g. the tensors handed to RCCL.
 * The three stages ENQUEUE their kernels on the context's lane-0 stream and return (errors of the launch itself are
 * reported; execution errors surface at the next synchronising call): run the collectives on that same stream
 * (zkpoa_context_stream: e.g. torch.cuda.ExternalStream) and no host synchronisation is needed anywhere in the chain,
 * or call zkpoa_context_synchronize before touching the buffers from another stream. The witness MSMs of
 * zkpoa_prove_partials_device run on other lanes and overlap the chain. d_witness NULL = the witness already resident. */
void* zkpoa_context_stream(zkpoa_context* ctx, int lane);   /* hipStream_t of lane 0..5 (NULL on error) */
int zkpoa_context_synchronize(zkpoa_context* ctx);          /* waits for lane 0's stream */
int zkpoa_zkey_load_shard_split(zkpoa_context* ctx, const void* zkey_buffer, unsigned long zkey_size,
                                uint64_t rank, uint64_t world, zkpoa_zkey** zkey);
int zkpoa_zkey_set_shard_split(zkpoa_context* ctx, zkpoa_zkey* zkey, uint64_t rank, uint64_t world);
int zkpoa_witness_load(zkpoa_context* ctx, const zkpoa_zkey* zkey, const void* wtns_buffer, unsigned long wtns_size,
                       uint8_t* public_le, unsigned long public_capacity);
int zkpoa_split_stage1(zkpoa_context* ctx, const zkpoa_zkey* zkey, const void* d_witness, void* d_exchange);
int zkpoa_split_stage2(zkpoa_context* ctx, const zkpoa_zkey* zkey, const void* d_received, void* d_exchange);
int zkpoa_split_stage3(zkpoa_context* ctx, const zkpoa_zkey* zkey, void* d_received);

/* Fixed-base tables for a resident key (zkpoa_msm_table_build applied to sections 9, 8 and the A / B queries, in
 * that order while they fit budget_bytes; 0 = half of the HBM free at the call). Later proves on the handle use
 * them; proofs are bit-identical with and without. groth16_prover_zkey_file's key cache does this by itself the
 * second time a key is used only with env ZKPOA_PRECOMP=eager; by default from zkpoa_idle_work (below: never inside a request). used_bytes (optional) <- HBM taken by the tables.
 * A shard handle (zkpoa_zkey_load_shard*, _load_device_shard) gets the tables of its own ranges -- 1/world of the
 * memory per GPU -- incl. the cyclic H shard of a split handle; a resident key re-pointed with zkpoa_zkey_set_shard*
 * uses its tables only while its range is the whole array they were built from. */
int zkpoa_zkey_precompute(zkpoa_context* ctx, zkpoa_zkey* zkey, uint64_t budget_bytes, uint64_t* used_bytes);

/* The H-MSM scalars of the LAST prove on this key handle (joinABC output, groth16_prove.js; domain x 32 B standard
 * form, or domain / world for a split shard: odd-coset indices i = rank mod world), copied to the host. Parity
 * tests use it to check pi_c at sizes where no CPU transform is affordable (oracle quotient identity). */
int zkpoa_zkey_read_h_scalars(zkpoa_context* ctx, const zkpoa_zkey* zkey, void* out, unsigned long capacity);

/* proof_points / public -> JSON text. style 0 = rapidsnark bytes, 1 = snarkjs bytes
 * (SURVEY.md 8a row a11). Size protocol as groth16_prover. */
int zkpoa_proof_to_json(const uint8_t proof_points[256], int style, char* buffer, unsigned long* size);
int zkpoa_public_to_json(const uint8_t* public_le, unsigned long n_public, int style, char* buffer,
                         unsigned long* size);

/* ---- stages of the path, host buffers in / out (upload + compute + download) -------------- */
/* G1.multiExpAffine / G2.multiExpAffine (snarkjs groth16_prove.js; rapidsnark ParallelMultiexp) */
int zkpoa_msm_g1(zkpoa_context* ctx, const void* bases, const void* scalars, uint64_t n, uint8_t out[64]);
int zkpoa_msm_g2(zkpoa_context* ctx, const void* bases, const void* scalars, uint64_t n, uint8_t out[128]);
/* Fr.fft / Fr.ifft: n = 2^log_n Montgomery-form elements, natural order in and out, in place */
int zkpoa_ntt(zkpoa_context* ctx, void* data, unsigned log_n, int inverse);
/* The H-scalar chain: buildABC1 + 3 x (ifft, batchApplyKey(inc), fft) + joinABC. coeffs is the
 * payload of zkey section 4 (u32 nCoefs, then 44-byte records), witness n_vars x 32 B;
 * out = domain_size x 32 B standard form. */
int zkpoa_h_scalars(zkpoa_context* ctx, const void* coeffs, unsigned long coeffs_size, const void* witness,
                    uint64_t n_vars, unsigned log_domain, void* out);

/* ---- same stages on device-resident data (what bench.py times; pointers are HIP device ptrs) */
int zkpoa_msm_g1_device(zkpoa_context* ctx, const void* d_bases, const void* d_scalars, uint64_t n, uint8_t out[64]);
int zkpoa_msm_g2_device(zkpoa_context* ctx, const void* d_bases, const void* d_scalars, uint64_t n, uint8_t out[128]);
int zkpoa_ntt_device(zkpoa_context* ctx, void* d_data, unsigned log_n, int inverse);
/* G1 MSM on an explicit lane (0..5: an independent HIP stream + workspace each): lets a caller keep
 * several MSMs in flight from several host threads, as zkpoa_prove does internally with its five MSMs.
 * Calls on the same lane must not overlap. zkpoa_last_ms_lane: id 0 = whole MSM (ms), 1 = its accumulation kernel (ms),
 * 2 = that kernel's mixed additions in millions (the non-zero digits of the scalars: the work the VALU roofline counts). */
int zkpoa_msm_g1_device_lane(zkpoa_context* ctx, int lane, const void* d_bases, const void* d_scalars, uint64_t n,
                             uint8_t out[64]);
float zkpoa_last_ms_lane(const zkpoa_context* ctx, int lane, int id);

/* Fixed-base form of the same MSMs for bases that stay resident (a proving key's sections 5-9 never change, and
 * 288 GB of HBM has room): zkpoa_msm_table_build stores 2^(c*j) * P_i for every window j of width c = window_bits
 * (0 = cost model) once, window-major, in the zkey wire format; zkpoa_msm_table_run_lane then computes
 * sum k_i * P_i for n scalars with ALL windows sharing one bucket set (fewer, wider windows: ~12-15 % fewer group
 * additions, 1/W of the bucket-reduction work). Results are bit-identical to zkpoa_msm_g1/g2_device on the
 * original bases. group: 1 = G1 (64-B points, out 64 B), 2 = G2 (128 B). info: out = {n, window_bits, windows, bytes}.
 * The prover builds the same tables for a resident key: zkpoa_zkey_precompute. */
typedef struct zkpoa_msm_table zkpoa_msm_table;
int zkpoa_msm_table_build(zkpoa_context* ctx, int group, const void* d_bases, uint64_t n, int window_bits,
                          zkpoa_msm_table** table);
void zkpoa_msm_table_free(zkpoa_context* ctx, zkpoa_msm_table* table);
int zkpoa_msm_table_info(const zkpoa_msm_table* table, uint64_t out[4]);
int zkpoa_msm_table_run_lane(zkpoa_context* ctx, int lane, const zkpoa_msm_table* table, const void* d_scalars,
                             uint8_t* out);

/* Synthetic bases for benchmarks at sizes where no CPU generator is affordable:
 * P_i = (a + i*b) * G, i in [i0, i0+n), written affine/Montgomery into d_out (n*64 or n*128 B).
 * a_le, b_le: 32-byte LE standard-form scalars. Known discrete logs make an O(n) field-only
 * check of any MSM result possible. */
int zkpoa_gen_bases_g1_device(zkpoa_context* ctx, const uint8_t a_le[32], const uint8_t b_le[32], uint64_t i0,
                              uint64_t n, void* d_out);
int zkpoa_gen_bases_g2_device(zkpoa_context* ctx, const uint8_t a_le[32], const uint8_t b_le[32], uint64_t i0,
                              uint64_t n, void* d_out);

/* Sum of affine points (the "all-reduce of partial sums" step of a sharded MSM, done on the host:
 * SURVEY.md 8e). in: count x 64/128 B, out: 64/128 B. No GPU needed. */
int zkpoa_g1_sum(const void* points, uint64_t count, uint8_t out[64]);
int zkpoa_g2_sum(const void* points, uint64_t count, uint8_t out[128]);
/* k * P on the host (used to check known-dlog MSM results). */
int zkpoa_g1_mul(const uint8_t point[64], const uint8_t scalar_le[32], uint8_t out[64]);
int zkpoa_g2_mul(const uint8_t point[128], const uint8_t scalar_le[32], uint8_t out[128]);

/* ---- phase-2 setup arithmetic: the point sections of `snarkjs zkey new`, scripts/g16_setup.sh:243-246 ----
 * out[s] = sum over the entries e with signal[e] == s of coefs[e] * points[point_index[e]], s < n_signals: one call per
 * zkey section -- A (section 5): the A-matrix coefficients over the Lagrange-form tau*G1 points of the prepared .ptau;
 * B1 / B2 (6, 7): the B matrix over tau*G1 resp. tau*G2; IC + C (3, 8): A over beta*tau*G1, B over alpha*tau*G1 and
 * C over tau*G1 in one call (concatenate the three point arrays and offset the indices). Everything on the device:
 * points in the zkey / ptau wire format (affine Montgomery, 64 B G1, 128 B G2; group = 1 | 2), coefs nnz x 32 B
 * little-endian standard form (< r, as an .r1cs file stores them), indices u32; out n_signals points, wire format,
 * signals without an entry = the point at infinity (all zero). Entries may come in any order. */
int zkpoa_setup_accumulate(zkpoa_context* ctx, int group, const void* d_points, uint64_t n_points, const void* d_coefs,
                           const uint32_t* d_point_index, const uint32_t* d_signal, uint64_t nnz, uint64_t n_signals,
                           void* d_out);
/* `snarkjs zkey new <circuit.r1cs> <pot.ptau> <circuit_0.zkey>` (= `snarkjs groth16 setup`; g16_setup.sh:243-252) on
 * files: reads the R1CS (iden3 binary format) and, from a .ptau prepared for phase 2, only the Lagrange-form point
 * ranges of the circuit's domain; computes sections 3 and 5-8 with zkpoa_setup_accumulate, section 9 (H) as the odd
 * points of the size-2n Lagrange basis, section 4 as snarkjs stores it (A and B terms per constraint ascending by
 * signal, then the nPublic + 1 public rows; values scaled by R^2), header with gamma2 = delta2 = the G2 generator
 * and delta1 = the G1 generator. Section 10 holds a zero circuit hash and no contributions ("no transcript"); see
 * zkpoa_zkey_new_ex for a key with one. The `zkpoa-setup` executable takes snarkjs' argument order.
 * Errors: zkpoa_last_error. */
int zkpoa_zkey_new(zkpoa_context* ctx, const char* r1cs_path, const char* ptau_path, const char* zkey_path);
/* ---- the phase-2 transcript (section 10; DESIGN.md "Phase-2 transcript") ------------------------------------------------
 * The publicly checkable trail of phase 2 as snarkjs lays it out: a circuit hash (Blake2b-512 over the initial key's
 * points) and one record per contribution or beacon (public key of its secret, transcript hash). It is opt-in: the
 * functions above keep writing and accepting keys without one.
 * No file made by snarkjs exists on this machine or in the reference. Interoperability with `snarkjs zkey verify` is
 * therefore NOT exercised. What is tested is self-consistency, plus every primitive against an independent
 * implementation.
 * zkpoa_zkey_new_ex with ZKPOA_SETUP_TRANSCRIPT writes the same key as zkpoa_zkey_new with the circuit hash filled in
 * (the ptau must hold section 2, tau^i G1 for i < 2n - 1). flags = 0 is zkpoa_zkey_new. */
#define ZKPOA_SETUP_TRANSCRIPT 0x1u
int zkpoa_zkey_new_ex(zkpoa_context* ctx, const char* r1cs_path, const char* ptau_path, const char* zkey_path,
                      uint32_t flags);
/* zkpoa_zkey_contribute on a key that carries a transcript (an error otherwise): the same arithmetic, and a type-0 record
 * appended: deltaAfter, g1_s = s * G1 (s from /dev/urandom), g1_sx = d * g1_s, g2_spx = d * hashToG2(transcript hash),
 * the optional name (at most 255 bytes). ZKPOA_PHASE2_S in the environment fixes s (tests only; a warning is printed). */
int zkpoa_zkey_contribute_ex(zkpoa_context* ctx, const char* zkey_in_path, const char* zkey_out_path,
                             const uint8_t* delta_le, const char* name);
/* `snarkjs zkey beacon <in> <out> <beaconHash> <numIterationsExp>` (g16_setup.sh:269-278): a contribution whose secret
 * and g1_s come from a ChaCha generator keyed by SHA-256 iterated 2^num_iterations_exp times over the beacon bytes, so
 * that any verifier recomputes them; a type-1 record. The input must carry a transcript. Exponents above 30 are refused
 * (2^30 hashes take minutes; more would not finish); beacon_len at most 255. */
int zkpoa_zkey_beacon(zkpoa_context* ctx, const char* zkey_in_path, const char* zkey_out_path, const uint8_t* beacon,
                      unsigned long beacon_len, uint32_t num_iterations_exp, const char* name);
/* Host only: *has_transcript <- the circuit hash is not zero, *count <- the records of section 10, text (optional) <- one
 * line "contribution <name>" or "beacon <name>" per record. PROVER_ERROR for an unreadable file or section 10. */
int zkpoa_zkey_contributions(const char* zkey_path, int* has_transcript, uint32_t* count, char* text, unsigned long cap);
/* Test hooks of the transcript's device work. zkpoa_hash_form: n points of group 1 | 2 (host, wire form) -> their hash
 * form (uncompressed big-endian standard form, Fq2 as c1 then c0, infinity = 0x40 then zeros), converted on the device
 * in pieces of piece_points (0 = default) through double-buffered pinned staging; digest <- Blake2b-512 of the stream,
 * out_bytes (optional) <- the stream itself. zkpoa_h_diff: out[i] = points[i + n] - points[i], i < n - 1, over 2n - 1
 * G1 points (the H part of the circuit hash over ptau section 2). */
int zkpoa_hash_form(zkpoa_context* ctx, int group, const void* points, uint64_t n, uint64_t piece_points, void* out_bytes,
                    uint8_t digest[64]);
int zkpoa_h_diff(zkpoa_context* ctx, const void* points, uint64_t n, void* out);
/* Host-only primitives of the transcript (csrc/phase2.hpp), exported for the tests. Field elements and scalars are 32 B
 * little-endian standard form unless a point's wire form (Montgomery) is named; ChaCha keys are eight u32 words. */
int zkpoa_blake2b512(const void* data, unsigned long len, uint8_t out[64]);
void* zkpoa_blake2b_new(void);
int zkpoa_blake2b_update(void* state, const void* data, unsigned long len);
int zkpoa_blake2b_final(void* state, uint8_t out[64]);          /* also frees the state */
int zkpoa_sha256(const void* data, unsigned long len, uint8_t out[32]);
void* zkpoa_chacha_new(const uint32_t key[8]);
uint32_t zkpoa_chacha_next_u32(void* rng);
uint64_t zkpoa_chacha_next_u64(void* rng);                       /* high word first */
int zkpoa_chacha_next_bool(void* rng);
void zkpoa_chacha_free(void* rng);
int zkpoa_fq_sqrt(const uint8_t a[32], uint8_t root[32]);        /* 1 = a root was written, 0 = not a square */
int zkpoa_fq2_sqrt(const uint8_t a[64], uint8_t root[64]);
int zkpoa_fr_from_rng(const uint32_t key[8], uint8_t out[32]);
int zkpoa_g1_from_rng(const uint32_t key[8], uint8_t out[64]);   /* wire form */
int zkpoa_g2_from_rng(const uint32_t key[8], uint8_t out[128]);  /* wire form, cofactor cleared */
int zkpoa_hash_to_g2(const uint8_t hash[64], uint8_t out[128]);
int zkpoa_beacon_key(const uint8_t* beacon, unsigned long len, uint32_t num_iterations_exp, uint32_t key[8]);
/* For a one-shot command only (zkpoa-setup): on != 0 leaves the large host arrays of zkpoa_zkey_new to the process's
 * exit instead of freeing them before the call returns (giving ~100 GB back page by page takes seconds at the
 * layer-three shape). A long-lived caller leaves this off. */
void zkpoa_setup_defer_host_frees(int on);
/* The arithmetic of `snarkjs zkey contribute <in.zkey> <out.zkey>` (g16_setup.sh:262-266): with a secret d (delta_le:
 * 32 B little-endian in [1, r); NULL = drawn from /dev/urandom), delta1, delta2 <- d * delta1, d * delta2 and every
 * point of sections 8 (C) and 9 (H) <- (1/d) * point (device; one scalar for all points, so no lane diverges). All
 * other sections are copied, section 10 included: no contribution record is written (zkpoa_zkey_contribute_ex writes
 * one). On a key that carries a transcript this leaves a stale trail, which zkpoa_zkey_verify reports as CONTRIBUTIONS. */
int zkpoa_zkey_contribute(zkpoa_context* ctx, const char* zkey_in_path, const char* zkey_out_path, const uint8_t* delta_le);
/* `snarkjs wtns check <circuit.r1cs> <witness.wtns>` (scripts/g16_verify.sh:205-210): every constraint's
 * <A, w> * <B, w> == <C, w> on the device. *violated <- how many constraints fail (0 = "WITNESS IS CORRECT"),
 * *first_violated (optional) <- the smallest failing constraint index. PROVER_ERROR for malformed files. */
int zkpoa_wtns_check(zkpoa_context* ctx, const char* r1cs_path, const char* wtns_path, uint64_t* violated,
                     uint64_t* first_violated);
/* `snarkjs zkey verify <circuit.r1cs> <pot.ptau> <circuit.zkey>` (scripts/g16_verify.sh -z): does the key belong to this
 * circuit and this ceremony? Restates the formulas of zkpoa_zkey_new / zkpoa_zkey_contribute and checks them with
 * random weights (rho over the wires, sigma over the domain, 253 bits each from /dev/urandom: a wrong key passes a check
 * with probability about 2^-128 or less): random combinations of the point sections (MSMs on the device) against the
 * same combinations of the ptau's Lagrange-form points, weighted by the r1cs' folds a = A rho, b = B rho, c = C rho.
 * PROVER_OK: both files were read and every check ran; *failed_checks <- a bitmask of ZKPOA_ZKEY_* (0 = the key is good).
 *   HEADER  protocol groth16 and BN254 moduli; alpha1, beta1, beta2 equal the ptau's; gamma2 is the G2 generator
 *   POINTS  every key point on its curve or the all-zero infinity; B2, beta2, gamma2, delta2 in G2; delta1 != O
 *   DELTA   e(delta1, G2) = e(G1, delta2)
 *   COEFFS  section 4's records in range, and its folds equal the r1cs' (A with the nPublic + 1 public rows, B)
 *   A, B1, B2  sum rho_i X_i = sum_j (a or b)_j L_j over the matching ptau range
 *   ICCH    e(sum_{i<=l} rho_i IC_i - Q, G2) e(sum_{i>l} rho_i C_i + sum_j sigma_j H_j, delta2) = 1,
 *           Q = sum_j a_j beta*L_j + b_j alpha*L_j + c_j L_j + sigma_j (odd point j of the 2n basis)
 * PROVER_ERROR (zkpoa_last_error) for a malformed file: bad magic, a missing section, a length that contradicts the
 * header, a key whose nVars / nPublic / domain differ from the circuit's, a field element >= its modulus, a ptau too
 * small for the domain or with a point off its curve, a truncated or over-long section 10.
 * A key whose circuit hash is zero carries no transcript: section 10 is not looked at further. Otherwise two more checks:
 *   CSHASH         the circuit hash, recomputed from the r1cs, the ptau and the key's A, B1, B2, IC
 *   CONTRIBUTIONS  every record, against the recomputed circuit hash: its transcript hash; e(g1_s, g2_spx) =
 *                  e(g1_sx, g2_sp); e(deltaAfter_k, g2_sp) = e(deltaAfter_{k-1}, g2_spx) with deltaAfter_0 = G1; the last
 *                  deltaAfter equals delta1; a beacon's g1_s and g1_sx recomputed from its beacon bytes
 * These are this project's formulas: a key made by snarkjs passes as far as snarkjs computes the same sections. */
#define ZKPOA_ZKEY_HEADER 0x01u
#define ZKPOA_ZKEY_POINTS 0x02u
#define ZKPOA_ZKEY_DELTA 0x04u
#define ZKPOA_ZKEY_COEFFS 0x08u
#define ZKPOA_ZKEY_A 0x10u
#define ZKPOA_ZKEY_B1 0x20u
#define ZKPOA_ZKEY_B2 0x40u
#define ZKPOA_ZKEY_ICCH 0x80u
#define ZKPOA_ZKEY_CSHASH 0x100u
#define ZKPOA_ZKEY_CONTRIBUTIONS 0x200u
int zkpoa_zkey_verify(zkpoa_context* ctx, const char* r1cs_path, const char* ptau_path, const char* zkey_path,
                      uint32_t* failed_checks);
/* `snarkjs powersoftau verify <pot.ptau>` (the reference's TODO at scripts/g16_setup.sh:201, g16_verify.sh:164): do the
 * powers of a ceremony file belong to one tau, alpha, beta, and does its Lagrange form (sections 12-15, what
 * zkpoa_zkey_new reads) agree with them? Power p, N = 2^p; T = section 2 (2N - 1 G1 points), U = section 3 (N G2), A, B
 * = sections 4, 5 (N G1), beta2 = section 6. Random weights (from /dev/urandom, drawn after the file is read): one rho
 * per power section, one rho_l per Lagrange level; a wrong file passes a check with probability about 2^-220 or less.
 * PROVER_OK: the file was read and every check ran; *failed_checks <- a bitmask of ZKPOA_PTAU_* (0 = the file is good):
 *   POINTS   every point on its curve or the all-zero infinity; U, beta2 and section 13 in G2; T_0 and U_0 the
 *            generators; T_1, A_0, B_0, beta2 != O
 *   TAU_G1   e(sum_{i<2N-2} rho^i T_i, U_1) = e(sum_{i<2N-2} rho^i T_{i+1}, G2) and e(T_1, G2) = e(G1, U_1)
 *   TAU_G2   e(T_1, sum_{i<N-1} rho^i U_i) = e(G1, sum_{i<N-1} rho^i U_{i+1})
 *   ALPHA, BETA  the ratio check of TAU_G1 on A, on B against U_1; BETA also e(B_0, G2) = e(G1, beta2)
 *   LAGRANGE_TAU_G1 / _TAU_G2 / _ALPHA / _BETA  section 12 / 13 / 14 / 15 agrees with section 2 / 3 / 4 / 5: per level
 *            of n points, sum_j P(w_n^j) L_j = sum_{i<n} rho_l^i X_i for P(x) = sum_{i<n} (rho_l x)^i (the top level
 *            p+1 of section 12 on the 2N - 1 powers that exist: P of degree 2N - 2)
 *   CONTRIBUTIONS  section 7 (DESIGN.md "Phase-1 transcript") holds one or more records and they do not verify. With
 *            prev = the generators and the challenge of a fresh file for record 0, for every record: a beacon's secrets
 *            and g1_s recomputed from its bytes; e(g1_s, g2_spx) = e(g1_sx, g2_sp) for tau, alpha, beta (g2_sp from
 *            the previous record's nextChallenge); tauG1, alphaG1, betaG1 against prev's with the key's ratio over
 *            (g2_sp, g2_spx), tauG2 and betaG2 over (g1_s, g1_sx). For the last record: its five points are T_1, U_1,
 *            A_0, B_0, beta2, and nextChallenge = Blake2b(response hash finished from partialHash and the key |
 *            hash form of the file's sections 2-6, made on the device). A file with no record passes.
 * info[4] <- power, ceremony power, prepared (sections 12-15 present; 0 = only the powers were checked), the number of
 * contribution records in section 7.
 * piece_points: points per upload as the sections stream through HBM (0 = derived from free HBM).
 * PROVER_ERROR (zkpoa_last_error) for a malformed file: bad magic or version, a non-BN254 header, a missing section 1-7,
 * a power outside [1, 28] (27 when prepared), a section whose length does not fit the power, only some of 12-15, a
 * coordinate >= q, a section 7 that ends inside a record, has bytes left over, an unknown parameter tag or a type
 * above 1. */
#define ZKPOA_PTAU_POINTS 0x001u
#define ZKPOA_PTAU_TAU_G1 0x002u
#define ZKPOA_PTAU_TAU_G2 0x004u
#define ZKPOA_PTAU_ALPHA 0x008u
#define ZKPOA_PTAU_BETA 0x010u
#define ZKPOA_PTAU_LAGRANGE_TAU_G1 0x020u
#define ZKPOA_PTAU_LAGRANGE_TAU_G2 0x040u
#define ZKPOA_PTAU_LAGRANGE_ALPHA 0x080u
#define ZKPOA_PTAU_LAGRANGE_BETA 0x100u
#define ZKPOA_PTAU_CONTRIBUTIONS 0x200u
int zkpoa_ptau_verify(zkpoa_context* ctx, const char* ptau_path, uint64_t piece_points, uint32_t* failed_checks,
                      uint32_t info[4]);
/* The inverse NTT whose elements are curve points (ffjavascript's G.ifft), the arithmetic of `powersoftau prepare
 * phase2`. Device pointers, wire format in and out (affine, Montgomery, G1 64 B / G2 128 B per point, infinity
 * all-zero, coordinates < q on output); w_n is the 2^log_n-th root of unity of zkpoa_ntt. log_n <= 28. Complete for
 * every input: equal points, opposite points, points at infinity. Every size takes the same kernels (one butterfly per
 * thread, workgroups of 64): there is no size threshold to set. */
/* d_out[j] = sum_i (w_n^(-ij) / n) * d_in[i], n = 2^log_n points in wire format (group = 1 | 2); d_out may equal d_in */
int zkpoa_ec_intt_device(zkpoa_context* ctx, int group, const void* d_in, uint32_t log_n, void* d_out);
/* `snarkjs powersoftau prepare phase2 <in.ptau> <out.ptau>`; info[4] as zkpoa_ptau_verify */
/* Writes in.ptau's sections 1-7 byte for byte, then sections 12-15 made from sections 2-5: level l (2^l points from
 * point 2^l - 1 on) is zkpoa_ec_intt_device of the section's first 2^l points; levels 0..power+1 for section 12 (the
 * top level over the 2N - 1 powers and one point at infinity), 0..power for 13-15. Sections 12-15 already in the input
 * are ignored (info[2] says whether it had them). The input is validated as zkpoa_ptau_verify validates it -- header,
 * lengths, every point on its curve with coordinates < q, sections 3 and 6 in G2 -- but not checked with pairings: run
 * zkpoa_ptau_verify on the result for that. PROVER_ERROR (zkpoa_last_error) for a malformed file (there a bad point is
 * an error too), a power of 28 (no root of unity for the top level), an output path that names the input file, or a
 * largest level whose buffers (about 700 B per point of 2^power) do not fit in free device memory. The output is
 * written under a temporary name and renamed when complete: a failure leaves nothing behind and a file already at
 * out_path untouched. */
int zkpoa_ptau_prepare_phase2(zkpoa_context* ctx, const char* in_path, const char* out_path, uint32_t info[4]);
/* ---- making and extending a ceremony file: `snarkjs powersoftau new / contribute / beacon` (DESIGN.md "Phase-1
 * transcript"). The layout of section 7 follows snarkjs as far as it is known to this project; no file made by snarkjs
 * has been read or written against, so interoperability is not exercised.
 * zkpoa_scalar_mul_each_device: d_out[i] = k_i * P_i, i < n < 2^32. Device pointers; points in wire format (affine,
 *   Montgomery, coordinates < q, infinity all-zero; group = 1 | 2), scalars 32 B little-endian standard form < r (a
 *   larger one is PROVER_ERROR), output wire format with canonical coordinates; d_out may equal d_points. Complete for
 *   P = O, k = 0 and every coincidence inside the walk. Every lane walks 64 signed 4-bit windows whatever its scalar.
 * zkpoa_power_scalars_device: d_out[i] = first * ratio^(i0 + i), i < n, 32 B little-endian standard form (device).
 * zkpoa_compressed_form: as zkpoa_hash_form, in the compressed form of a point: x alone (big-endian standard form, Fq2
 *   as c1 then c0; 32 B for G1, 64 B for G2), bit 7 of byte 0 set when y is the negative root (above (q - 1) / 2; for
 *   Fq2 by c1, by c0 when c1 = 0), infinity = 0x40 then zeros. */
int zkpoa_scalar_mul_each_device(zkpoa_context* ctx, int group, const void* d_points, const void* d_scalars, uint64_t n,
                                 void* d_out);
int zkpoa_power_scalars_device(zkpoa_context* ctx, const uint8_t first_le[32], const uint8_t ratio_le[32], uint64_t i0,
                               uint64_t n, void* d_out);
int zkpoa_compressed_form(zkpoa_context* ctx, int group, const void* points, uint64_t n, uint64_t piece_points,
                          void* out_bytes, uint8_t digest[64]);
/* `powersoftau new bn128 <power> <out>`: sections 1-6 with every point the generator, section 7 with no record;
 * power in [1, 28]. */
int zkpoa_ptau_new(zkpoa_context* ctx, uint32_t power, const char* out_path);
/* `powersoftau contribute <in> <out>`: point i of section 2 and 3 times tau^i, of section 4 times alpha tau^i, of
 * section 5 times beta tau^i, section 6 times beta (zkpoa_power_scalars_device, zkpoa_scalar_mul_each_device), the
 * sections streamed through device memory in pieces (option "ptau_piece_points"; 0 = from free memory), and one record
 * appended to section 7. secrets_le: tau | alpha | beta, 3 x 32 B little-endian in [1, r), or NULL = /dev/urandom.
 * ZKPOA_PHASE1_S in the environment ("s_tau,s_alpha,s_beta", decimal or 0x hex) fixes the s of the key's g1_s = s G1
 * (tests only; a warning is printed). The input is validated as zkpoa_ptau_prepare_phase2 validates it; its sections
 * 12-15 are dropped (a notice on stderr). The output appears under its name only when complete; an output path that
 * names the input is refused. name: optional, at most 255 bytes. */
int zkpoa_ptau_contribute(zkpoa_context* ctx, const char* in_path, const char* out_path, const uint8_t* secrets_le,
                          const char* name);
/* `powersoftau beacon <in> <out> <beaconHash> <numIterationsExp>`: a contribution whose secrets and g1_s come from the
 * ChaCha generator of zkpoa_beacon_key (per key tau, alpha, beta: the secret, then g1_s); a type-1 record. Exponents
 * above 30 and beacons above 255 bytes are refused. */
int zkpoa_ptau_beacon(zkpoa_context* ctx, const char* in_path, const char* out_path, const uint8_t* beacon,
                      unsigned long beacon_len, uint32_t num_iterations_exp, const char* name);
/* ---- challenge and response files: `snarkjs powersoftau export challenge / challenge contribute / import response`
 * (DESIGN.md "Phase-1 transcript", "Challenge and response files"; N = 2^power).
 *   challenge file: 64 B, the response hash of the ceremony file's last record (Blake2b-512 of the empty string for a
 *     file without records) | the hash form of sections 2-6. Its Blake2b-512 is the ceremony file's challenge.
 *   response file: 64 B, the challenge | the compressed form of the new sections 2-6 | the nine points of the key in
 *     hash form (768 B). Its Blake2b-512 is the record's response hash.
 * The formats follow snarkjs as far as they are known to this project; acceptance by snarkjs is not exercised.
 * zkpoa_sqrt_device: n elements of Fq (field 0, 32 B) or Fq2 (field 2, 64 B, c0 then c1) in wire form (Montgomery,
 *   little-endian, below q; host buffers) -> roots[i] = the root of a[i] that is not negative (not above (q - 1) / 2; for
 *   Fq2 by c1, by c0 when c1 = 0), all-zero when a[i] is no square, and is_square[i] = 1 | 0. Every element takes the
 *   same exponentiations: one in Fq, two in Fq2.
 * zkpoa_decompressed_form: the inverse of zkpoa_compressed_form. n points of group 1 | 2 in compressed form (host) ->
 *   out_points in wire form (host, 64 | 128 B each), converted on the device in pieces of piece_points (0 = 2^18).
 *   PROVER_ERROR naming the first offending point's index for: both flag bits set, 0x40 followed by anything but zeros,
 *   an x not below q, an x for which x^3 + b is no square. Subgroup membership is not checked here.
 * zkpoa_from_hash_form: the inverse of zkpoa_hash_form, the same way. PROVER_ERROR naming the point's index for: bit 7
 *   of its first byte set, 0x40 followed by anything but zeros, a coordinate not below q. Neither the curve equation nor
 *   subgroup membership is checked here. */
int zkpoa_sqrt_device(zkpoa_context* ctx, int field, const void* a, uint64_t n, void* roots, uint8_t* is_square);
int zkpoa_decompressed_form(zkpoa_context* ctx, int group, const void* bytes, uint64_t n, uint64_t piece_points,
                            void* out_points);
int zkpoa_from_hash_form(zkpoa_context* ctx, int group, const void* bytes, uint64_t n, uint64_t piece_points,
                         void* out_points);
/* `powersoftau export challenge <in.ptau> <challenge>`: writes the challenge file of ptau_path; challenge_hash
 * (optional) <- its Blake2b-512. Refused, with nothing left behind, when that hash is not the file's challenge (the
 * nextChallenge of its last record; of a file without records, the challenge of the generators): the sections are then
 * not the ones the last record describes. An output path that names the input is refused. */
int zkpoa_ptau_export_challenge(zkpoa_context* ctx, const char* ptau_path, const char* challenge_path,
                                uint8_t challenge_hash[64]);
/* `powersoftau challenge contribute bn128 <challenge> <response>`: zkpoa_ptau_contribute's arithmetic on a challenge
 * file. The power comes from the file's size (any other size is refused), the challenge is the Blake2b-512 of the
 * whole file; the points are read back from hash form, checked (curve, G2 subgroup), multiplied and written in
 * compressed form, in pieces (option "ptau_piece_points"). secrets_le and ZKPOA_PHASE1_S as zkpoa_ptau_contribute.
 * response_hash (optional) <- the Blake2b-512 of the response file. */
int zkpoa_ptau_challenge_contribute(zkpoa_context* ctx, const char* challenge_path, const char* response_path,
                                    const uint8_t* secrets_le, uint8_t response_hash[64]);
/* `powersoftau import response <old.ptau> <response> <new.ptau>`: new_path <- old_path's header, the response's
 * sections decompressed on the device, and section 7 with one more record (type 0, `name`, the key from the response).
 * Refused, with nothing left behind: a response whose size does not fit the old file's power or whose first 64 bytes
 * are not the old file's challenge; a point that does not decompress (the message names section and index), is off
 * its curve or outside G2; a record that does not verify against the old file's last record as zkpoa_ptau_verify checks
 * it (the key's pairings, the ratios of tau, alpha and beta). That the sections are one chain of powers is NOT checked
 * here: zkpoa_ptau_verify on the result does that. Sections 12-15 of the old file are dropped (a notice on stderr). */
int zkpoa_ptau_import_response(zkpoa_context* ctx, const char* old_path, const char* response_path, const char* new_path,
                               const char* name);
/* Host only: *count <- the records of section 7, text (optional) <- one line "contribution <name> <response hash, hex>"
 * or "beacon <name> <response hash, hex>" per record. PROVER_ERROR for an unreadable file or a malformed section 7. */
int zkpoa_ptau_contributions(const char* ptau_path, uint32_t* count, char* text, unsigned long cap);
/* The Blake2b state a record's partialHash holds (216 B: h[8], t[2], the 128-byte buffer, its fill; little-endian u64,
 * buffer bytes past the fill zero). zkpoa_blake2b_restore: a new state to update / final, or NULL for a fill above 128. */
int zkpoa_blake2b_state(void* state, uint8_t out[216]);
void* zkpoa_blake2b_restore(const uint8_t saved[216]);

/* ---- the step after the path; host only, no GPU ----------------------------------------
 * zkpoa_groth16_verify: `npx snarkjs groth16 verify <vkey> <public> <proof>` (scripts/g16_verify.sh:213-216)
 *   on the three JSON texts. Returns PROVER_OK (valid), ZKPOA_VERIFY_INVALID_PROOF, or PROVER_ERROR (malformed).
 * zkpoa_sanitize_proof: `python scripts/sanitize_groth16_proof.py` (sanitize_groth16_proof.py:39-124): the
 *   text of sanitized_proof.json (43-bit x 6 limbs; e(-alpha1, beta2) as negalfa1xbeta2), byte-identical to the
 *   reference's output. Size protocol as groth16_prover. */
#define ZKPOA_VERIFY_INVALID_PROOF 0x10
int zkpoa_groth16_verify(const char* vkey_json, const char* public_json, const char* proof_json,
                         char* error_msg, unsigned long error_msg_maxsize);
int zkpoa_sanitize_proof(const char* vkey_json, const char* public_json, const char* proof_json,
                         char* buffer, unsigned long* size, char* error_msg, unsigned long error_msg_maxsize);
/* The same verification on wire-format points, no JSON. vkey_points = alpha1(64) beta2(128) gamma2(128) delta2(128)
 * then IC[(n_public+1) x 64] -- exactly the verification key a .zkey carries in sections 2 and 3 (what
 * `snarkjs zkey export verificationkey`, scripts/g16_setup.sh:287-293, turns into <circuit>_vkey.json);
 * proof_points as zkpoa_prove returns them; public_le = n_public x 32 B standard form. Same return codes.
 * zkpoa_zkey_vkey copies that key out of a resident proving key (size protocol as groth16_prover; PROVER_ERROR
 * when the handle has none: zkpoa_zkey_load_device keys). */
int zkpoa_groth16_verify_points(const uint8_t* vkey_points, unsigned long vkey_size, const uint8_t proof_points[256],
                                const uint8_t* public_le, unsigned long n_public, char* error_msg,
                                unsigned long error_msg_maxsize);
int zkpoa_zkey_vkey(const zkpoa_zkey* zkey, uint8_t* buffer, unsigned long* size);
/* `snarkjs zkey export verificationkey <zkey> <vkey.json>` (scripts/g16_setup.sh:287-293), host only: the text of
 * <circuit>_vkey.json from the zkey image's sections 1-3, byte for byte what snarkjs writes (1-space indent,
 * vk_alphabeta_12 included); pinned on the reference's committed *_vkey.json. Size protocol as groth16_prover.
 * CLI: `zkpoa-verify --export-vkey <zkey> <vkey.json>`. */
int zkpoa_zkey_export_vkey(const void* zkey_buffer, unsigned long zkey_size, char* buffer, unsigned long* size,
                           char* error_msg, unsigned long error_msg_maxsize);

/* ---- the anonymity-set Merkle tree; GPU ------------------------------------------------------
 * Stands in for the reference's Rust binary `merkle-tree` (scripts/merkle_tree.rs, run at
 * scripts/full_workflow.sh:371-380): circomlib Poseidon(2) over Fr (light-poseidon `new_circom(2)`), leaf =
 * H(address, balance), zero-valued leaves up to the next power of two, node = H(left, right).
 * All field elements: 32 B little-endian standard form (the Rust code's big-endian byte arrays reversed).
 * zkpoa_poseidon2: n independent hashes out[i] = H(left[i], right[i]).
 * zkpoa_merkle_build: the whole tree for n (address, balance) pairs, kept in HBM; info: out = {n, path length
 * (= rs_merkle depth() - 1), nodes}; root; stored leaves (hashes; zero for padding) for locating owned addresses
 * (merkle_tree.rs:329-346); path: the sibling hashes of a leaf from the leaves up + the index bit per level, i.e. one
 * entry of merkle_proofs.json's path_elements / path_indices (merkle_tree.rs:354-376).
 * zkpoa_poseidon_params (host only, no GPU): the hash parameters as this library generates them (Grain LFSR), standard
 * form: 195 round constants, then the 3 x 3 MDS matrix row-major. */
typedef struct zkpoa_merkle zkpoa_merkle;
int zkpoa_poseidon_params(uint8_t out[204 * 32]);
int zkpoa_poseidon2(zkpoa_context* ctx, const void* left, const void* right, uint64_t n, void* out);
int zkpoa_poseidon2_device(zkpoa_context* ctx, const void* d_left, const void* d_right, uint64_t n, void* d_out);
int zkpoa_merkle_build(zkpoa_context* ctx, const void* addresses, const void* balances, uint64_t n, zkpoa_merkle** tree);
int zkpoa_merkle_build_device(zkpoa_context* ctx, const void* d_addresses, const void* d_balances, uint64_t n,
                              zkpoa_merkle** tree);
void zkpoa_merkle_free(zkpoa_context* ctx, zkpoa_merkle* tree);
int zkpoa_merkle_info(const zkpoa_merkle* tree, uint64_t out[3]);
int zkpoa_merkle_root(zkpoa_context* ctx, const zkpoa_merkle* tree, uint8_t root_le[32]);
int zkpoa_merkle_leaves(zkpoa_context* ctx, const zkpoa_merkle* tree, uint64_t first, uint64_t count, void* out);
int zkpoa_merkle_path(zkpoa_context* ctx, const zkpoa_merkle* tree, uint64_t leaf_index, uint8_t* path_le,
                      uint8_t* path_indices);

/* ---- ECDSA -> ECDSA*: secp256k1 recovery, Keccak-256, Ethereum addresses; GPU ----------------------------------
 * Stands in for the arithmetic of the reference's scripts/ecdsa_sigs_parser.ts + scripts/lib/ecdsa_star.ts (run at
 * scripts/full_workflow.sh:354-357 with ethers and noble-secp256k1). Host buffers, nothing kept between calls.
 * Byte order: every 32-byte integer of these three entry points (r, s, msghash, r', x, y) is BIG-endian, as the hex
 * strings of a signatures file spell it and as Keccak takes a public key; digests and addresses are in their own order.
 * zkpoa_ecdsa_star: n signatures. r, s, msghash: n x 32 B; v: n bytes (27 / 28); address20: n x 20 B, the address each
 * signer claims. Out: r' (n x 32 B; the y coordinate of the nonce point R = (r, r'), parity by v), the recovered key
 * Q = r^-1 (s R - z G) as x || y (n x 64 B), the address derived from it (n x 20 B) and a status byte per signature,
 * the first that applies: 0 ok; 1 v is not 27 or 28; 2 r or s is zero or not below the group order; 3 s >= 2^255;
 * 4 r^3 + 7 is not a square; 5 the key is the point at infinity; 6 the derived address differs from the one given.
 * Statuses 1-5 come with zeros in every output, status 6 with what was derived. Only recovery ids 0 and 1 exist (an r
 * that would need r + n is not tried). Returns PROVER_OK when it ran, whatever the statuses; n = 0 is a no-op.
 * zkpoa_keccak256: n messages of one common length message_len (0..4096 bytes) packed back to back -> n x 32 B.
 * zkpoa_eth_address: ethers.computeAddress for n uncompressed keys (x || y, n x 64 B): the 20 address bytes and the
 * EIP-55 text, "0x" + 40 characters per key (n x 42 B, no terminator). */
int zkpoa_ecdsa_star(zkpoa_context* ctx, uint64_t n, const void* r, const void* s, const void* msghash, const uint8_t* v,
                     const void* address20, void* out_rprime, void* out_pubkey_xy, void* out_address20, uint8_t* out_status);
int zkpoa_keccak256(zkpoa_context* ctx, const void* messages, uint64_t message_len, uint64_t n, void* out32);
int zkpoa_eth_address(zkpoa_context* ctx, const void* pubkey_xy, uint64_t n, void* out_address20, void* out_checksum42);

/* ---- the other direction: batched SHA-256, public keys, RFC 6979 nonces and ECDSA signatures; GPU -----------------
 * What `ecdsa-sigs-parser sign` and `anon-set` compute (the reference's tests/generate_ecdsa_signatures.ts and
 * tests/generate_anon_set.ts): five entry points, declared in a header of their own next to this one. */
#include "zkpoa_ecdsa_sign.h"

/* ---- HD-wallet key sources: BIP-32 children of one parent, batched SHA-512 / HMAC-SHA512; GPU, and host helpers ------
 * Where `ecdsa-sigs-parser sign`, `anon-set` and `hd-list` take the keys of a mnemonic, an xprv or an xpub from: nine
 * entry points, declared in a header of their own next to this one. */
#include "zkpoa_hd_wallet.h"

/* ---- the input steps after the proofs; host only, no context, no GPU -------------------------------------------
 * The Poseidon of any circomlib width, the sponge of input_prep_for_layer_two.ts and the ed25519 Pedersen commitment
 * of pedersen_commitment_checker.ts: four entry points, declared in a header of their own next to this one. */
#include "zkpoa_layer_inputs.h"

/* ---- the verifier's side: the published set's duplicate check (a stable device sort of its addresses), the commitment
 * the layer-three signals spell, and the whole check of set, root, commitment and proof in one call (`zkpoa-audit`):
 * four entry points, declared in a header of their own next to this one. */
#include "zkpoa_audit.h"

/* ---- the owned leaves at the prover's scale: a lookup through that stable index (any order, exact), the same over a
 * resident tree, and the sibling paths of any number of leaves gathered by one kernel, where the single-leaf path entry
 * point above copies 32 bytes per level: four entry points, declared in a header of their own next to this one. */
#include "zkpoa_merkle_paths.h"

/* ---- the anonymity set against an Ethereum state root: Merkle-Patricia account proofs (what `eth_getProof` returns)
 * hashed and walked on the device, a block header's hash and state root, and the whole check of a set's balances
 * against a file of such proofs: four entry points, declared in a header of their own next to this one. */
#include "zkpoa_state_proof.h"

/* ---- measurement -------------------------------------------------------------------------- */
/* Timings (ms, HIP events on the stream that ran the kernels) of the last call on this context.
 * id: 0 = whole device part of last MSM, 1 = its bucket-accumulation kernel (dominant kernel),
 *     2 = last NTT, 3 = last prove: ABC+NTT chain, 4 = last prove: all MSMs, 5 = last prove: total,
 *     6 = last prove: self-check (host pairing check; 0 when it did not run), 7 = last Merkle tree build,
 *     8 = last zkpoa_ecdsa_star, zkpoa_ecdsa_sign, zkpoa_bip32_children, zkpoa_bip32_tweak, zkpoa_mpt_verify or
 *         zkpoa_eth_account_proofs: its kernels (after zkpoa_anon_set_state_check_file: those of all its slabs),
 *     9 = last zkpoa_anon_set_index_device or zkpoa_anon_set_audit: its kernels,
 *     10 = last zkpoa_anon_set_find_device, zkpoa_merkle_find, zkpoa_merkle_paths or zkpoa_merkle_paths_device: its kernels.
 * Also: tuning knobs. key "msm_c" forces the Pippenger window (0 = auto); key "msm_max_points" sets the
 * number of points one bucket sort may take (0 = 2^27; larger MSMs run in chunks -- tests force small values);
 * key "prove_serial" = 1 runs the stages of a prove one after the other (solo device times for the roofline);
 * key "lane_workspace_max_mb" caps the workspace of every MSM lane (0 = none).
 * Memory pressure: an MSM's workspace grows with the points it sorts at once (~0.4 GB per million at 2^26). When a
 * lane's workspace does not fit -- HBM full (a 2^27 key, another process on the card) or over the cap above -- the MSM
 * is not failed: it goes through its points in pieces of half the size (again halved if need be, down to 2^16), the
 * context remembers the size that fitted, and the result is the same point. zkpoa_msm_points_limit() returns the
 * number of points one MSM of this context sorts at once right now (2^27 until something did not fit). */
float zkpoa_last_ms(const zkpoa_context* ctx, int id);
int zkpoa_set_option(zkpoa_context* ctx, const char* key, long value);
uint64_t zkpoa_msm_points_limit(const zkpoa_context* ctx);

/* ---- element-wise device hooks used by the parity tests ----------------------------------- */
/* field: 0 = Fq, 1 = Fr. op: 0 = Montgomery mul, 1 = add, 2 = sub, 3 = inverse (b ignored),
 * 4 = to Montgomery, 5 = from Montgomery. a, b, out: n x 32 B host buffers. */
int zkpoa_field_op(zkpoa_context* ctx, int field, int op, const void* a, const void* b, void* out, uint64_t n);
/* group: 1 = G1, 2 = G2. out[i] = a[i] + b[i] (affine in, affine out, all exceptional cases). */
int zkpoa_group_add(zkpoa_context* ctx, int group, const void* a, const void* b, void* out, uint64_t n);
/* The field layer's own primitives on raw lazy values (Montgomery form, each in [0, 2p) unless the op says more).
 * field: 0 = Fq, 1 = Fr (32-byte elements), 2 = Fq2 (64 bytes: c0, c1). in: the op's operand arrays of n elements
 * back to back; out: its result arrays likewise. raw != 0 stores results exactly as computed (lazy form), else
 * canonical. Fq / Fr op (operands -> results): 0 = mul (a, b), 1 = sqr (a), 2 = add (a, b), 3 = sub (a, b),
 * 4 = neg (a), 5 = neg_2p (a), 6 = dbl (a), 7 = canon (a), 8 = reduce_2p (a < 4p), 9 = inv (a),
 * 10 = dot2 (a0, b0, a1, b1; b1 may be 2p), 11 = dot3 (a0, b0, a1, b1, a2, b2; every b < p),
 * 12 = mul_pair (a, b, c, d -> ab, cd), 13 = sqr_pair (a, b -> a^2, b^2),
 * 14 = dot2_pair (a0, b0, a1, b1, c0, d0, c1, d1 -> two dot2), 15 = is_zero (a), 16 = a == b;
 * is_zero and == store 0 / 1 in limb 0. Fq2 op: 0 = mul, 1 = sqr, 2 = add, 3 = sub, 4 = neg, 5 = inv. */
int zkpoa_field_prim(zkpoa_context* ctx, int field, int op, const void* in, void* out, uint64_t n, int raw);
/* The group layer's own XYZZ primitives. group: 1 = G1, 2 = G2. a: n XYZZ points (x, y, zz, zzz; Montgomery;
 * coordinates in [0, 2p); infinity = zz equal to 0 mod p); b: n affine points (zkey wire form) or, for op 0, n XYZZ
 * points; k: n u32 negate flags (op 1) or multipliers (op 4). out: n XYZZ, stored as computed.
 * op: 0 = a + b (xyzz_add), 1 = a + (k ? -b : b) (xyzz_add_affine), 2 = 2a (xyzz_dbl), 3 = 2b for b not infinity
 * (xyzz_dbl_affine), 4 = k a (xyzz_mul_small). Arguments an op does not use may be NULL. */
int zkpoa_curve_prim(zkpoa_context* ctx, int group, int op, const void* a, const void* b, const uint32_t* k,
                     void* out, uint64_t n);
/* The G1 accumulation's field: Fq in 9 limbs of 29 bits, Montgomery radix 2^261 (csrc/fq29.hip.h). Elements of n
 * records of 32-bit words, in and out. Ops 0-3 and 7 take each operand as 9 limbs exactly as given when raw != 0 (so
 * operands at the edge of the header's bounds can be fed), as 8 words re-limbed on load otherwise, and return 9 limbs
 * as computed: 0 = mul (a, b), 1 = sqr (a), 2 = dot2 (a0, b0, a1, b1), 3 = norm(a + (4q - b)),
 * 7 = norm(a + (14q - b)). 4 = re-limb: 8 words -> 9 limbs, then the 8 words made from them (17 out).
 * 5 = mixed addition as the accumulation kernel does it: XYZZ (32 words, wire form, infinity = zz 0), affine base
 * (16 words), negate flag (1 word) -> canonical XYZZ (32 words). 6 = full addition: two XYZZ -> canonical XYZZ.
 * 8 = a piece as msm_accum0_kernel sums it: 8 x (affine base, negate flag) = 136 words -> canonical XYZZ.
 * The packed partial sums of the G1 MSM (128 bytes: the four coordinates times 2^261, each below 2^256; infinity =
 * all zero): 10 = packed + packed -> packed (32 words), then one word that is 1 when the generic sum was poisoned
 * and the exact addition redid it, then 3 zero words; 11 = a piece as op 8 -> packed, same 36 words out;
 * 12 = packed -> canonical wire XYZZ. There is no op 9. raw is ignored by ops 4-6 and 8-12. */
int zkpoa_fq29_prim(zkpoa_context* ctx, int op, const void* in, void* out, uint64_t n, int raw);
/* The secp256k1 layer's own functions (csrc/secp256k1.hip.h: Fp, Sc, recode_signed4, to_affine, fixed_mul, double_mul) on
 * raw 8-word values, one record per lane: one entry point, declared with its op numbers in a header of its own next to
 * this one. */
#include "zkpoa_secp_prim.h"
/* The NTT's other forms on a host buffer, in place (parity tests). form: 0 = ntt_dif (natural in, bit-reversed out),
 * 1 = ntt_dit (bit-reversed in, natural out), 2 = ntt_to_odd_coset (inverse ignored). No 1/n in forms 0 and 1.
 * batch vectors of 2^log_n elements start stride elements apart (stride >= 2^log_n); elements between them are not
 * touched. data holds ((batch - 1) * stride + 2^log_n) * 32 bytes. */
int zkpoa_ntt_form(zkpoa_context* ctx, void* data, unsigned log_n, int form, int inverse, unsigned batch, uint64_t stride);
/* The NTT's pass plan for 2^log_n elements (test hook; needs no context, no GPU and reads no environment variable).
 * tile_log: 0 = the tile size that log_n takes by default, 10 or 11 = that tile. Writes seven words per pass, in DIT
 * order: s_lo, B, logT, grid.x, threads, dynamic LDS bytes, direct boundary table 0 / 1; passes that do not fit in cap
 * words are left out. Returns the pass count, or -1 for log_n > 28 or any other tile_log. */
int zkpoa_test_ntt_plan(unsigned log_n, unsigned tile_log, uint32_t* out, unsigned cap);
/* The plan of one MSM and the lane workspace it takes (test hook; needs no context, no GPU and reads no environment
 * variable). The arguments are the whole request: n points (at most 2^28) sorted at once; c = the forced or the table's
 * window width, 0 or a value outside 4..22 (merged: 4..25) = the cost model; merged = the fixed-base form; for_g2 = the
 * sort feeds a G2 accumulation; density32_or_null = non-zero digits per scalar indexed by the window width (32 doubles,
 * 4..25 are read), null = uniform scalars; k0 = the forced level-0 piece length, outside 8..512 = the rule. Writes
 * thirteen words: c, W, Wb, ne, TB, K0, K, logS, logRows; sparse 0 / 1; bytes of the sort's, the G1 accumulation's and
 * the G2 accumulation's workspace (0 for n == 0; the sizes without the guards that ZKPOA_WS_GUARD=1, a test hook of the
 * environment, puts behind every region of a lane's workspace to catch a kernel writing past its region: an MSM then
 * fails with an error naming the region); words that do not fit in cap are left out. Returns 13, or -1 for
 * n > 2^28, c outside 0..31, a flag that is not 0 / 1, k0 < 0 or a null out with cap > 0. */
int zkpoa_test_msm_plan(uint64_t n, int c, int merged, int for_g2, const double* density32_or_null, int k0, uint64_t* out,
                        unsigned cap);
/* Phase A of one MSM -- digits or the compact entry list, the counting-sort passes, the scans, the piece ordering --
 * on n host scalars (32 B little-endian), run on lane `lane` through the prover's own entry, and what it hands the
 * accumulation (test hook). n .. k0 are the request, as in zkpoa_test_msm_plan. Writes plan: the thirteen words of
 * zkpoa_test_msm_plan; totals: non-zero digits (entries), the largest bucket, level-0 pieces; and seven arrays of 32-bit
 * words, out[i] with room for cap[i] words: 0 = counts[TB] (entries per bucket), 1 = off0[TB + 1] (their exclusive sum),
 * 2 = po_a[TB + 1] (exclusive sum of the buckets' piece counts), 3 = sorted[entries] (point index, merged form: table
 * index w * n + i, | sign << 31, grouped by bucket in off0's order), 4 = pbkt[pieces] (bucket of each piece),
 * 5 = order[pieces] (piece ids, longest first), 6 = len_hist[K0 + 1] (pieces of each length, as the scan left them).
 * Returns PROVER_ERROR_SHORT_BUFFER when a capacity is too small: plan and totals are written, none of the arrays is.
 * PROVER_ERROR for arguments out of range (as zkpoa_test_msm_plan; lane outside 0..11) or a device failure. */
int zkpoa_test_msm_sort(zkpoa_context* ctx, int lane, const void* scalars, uint64_t n, int c, int merged, int for_g2,
                        const double* density32_or_null, int k0, uint64_t plan[13], uint32_t totals[3],
                        uint32_t* const out[7], const uint64_t cap[7]);
/* The digit density the prover measures on a witness (test hook), on n host scalars: for c = 4..25 out[c] = the sum of
 * ceil(bit length of min(s, r - s) / c) over the scalars, divided by n; elsewhere, and everywhere for n = 0, the
 * uniform default ceil(254 / max(c, 4)). */
int zkpoa_test_msm_density(zkpoa_context* ctx, const void* scalars, uint64_t n, double out[32]);

#ifdef __cplusplus
}
#endif
#endif /* ZKPOA_PROVER_H */
