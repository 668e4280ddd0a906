/* libzkpoa_prover.so -- test hook: the secp256k1 layer's own functions one by one on the GPU.
 *
 * csrc/secp256k1.hip.h (Fp, Sc, recode_signed4, to_affine, fixed_mul, double_mul) is otherwise reached only through whole
 * recoveries and signatures, whose inner values are uniformly random whatever the inputs are; this entry point feeds each
 * function the operands a test chooses. One record per GPU lane. Host buffers, nothing kept between calls.
 *
 * Every value is eight 32-bit words, least significant first (NOT the big-endian bytes of zkpoa_ecdsa_star), taken and
 * stored exactly as given and as computed: no range fix-up on either side. in: the op's operand arrays of n values back
 * to back (as zkpoa_field_prim); out: its result arrays likewise, 8-word arrays first, then the array of the op's extra
 * words (one or two per record) where it has them.
 *
 *   op  function                     operands               results
 *    0  Fp *                         a, b                   r
 *    1  Fp sqr                       a                      r
 *    2  Fp +                         a, b                   r
 *    3  Fp -                         a, b                   r
 *    4  Fp neg                       a                      r
 *    5  Fp dbl                       a                      r
 *    6  Fp inv                       a                      r
 *    7  Fp sqrt_candidate            a                      r
 *    8  Fp ge_p                      a                      one word, 0 / 1
 *    9  Sc *                         a, b                   r
 *   10  sc_add                       a, b                   r
 *   11  Sc neg                       a                      r
 *   12  Sc inv                       a                      r
 *   13  Sc reduce_once               a                      r
 *   14  key_from_hash                h                      r
 *   15  Sc ge_n                      a                      one word, 0 / 1
 *   16  Sc is_high                   a                      one word, 0 / 1
 *   17  recode_signed4               k                      mag (8 words), then sgn (two words, low first)
 *   18  to_affine                    x, y, zz, zzz          x, y
 *   19  fixed_mul                    k                      x, y, zz, zzz as computed
 *   20  double_mul = u2 R + u1 G     R.x, R.y, u2, u1       x, y, zz, zzz as computed, then one word: is_inf 0 / 1
 *
 * Ops 19 and 20 use the library's own tables: the fixed-base table of zkpoa_ecdsa_sign, and for op 20 the 1G .. 8G table
 * of zkpoa_ecdsa_star plus a table of the lane's own in a buffer of this call. u2 and u1 must be below the group order, as
 * double_mul asks; nothing else is asked of any operand. n is at most 2^16. An op outside 0 .. 20 is PROVER_ERROR, also
 * for n = 0; otherwise n = 0 is PROVER_OK and touches nothing.
 *
 * include/zkpoa_prover.h includes this file beside its other test hooks.
 */
#ifndef ZKPOA_SECP_PRIM_H
#define ZKPOA_SECP_PRIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct zkpoa_context;

int zkpoa_secp_prim(struct zkpoa_context* ctx, int op, const void* in, void* out, uint64_t n);

#ifdef __cplusplus
}
#endif
#endif /* ZKPOA_SECP_PRIM_H */
