// BN254 base field in 9 limbs of 29 bits, Montgomery radix R' = 2^261: the G1 bucket accumulation's field.
//
// Fp<> (bn254_field.hip.h) multiplies 8 x 32-bit limbs: a column of partial products needs 67 bits, so every
// v_mad_u64_u32 is followed by a v_addc into a third accumulator word -- half of the product's instructions carry
// bits. With 29-bit limbs a whole column fits ONE 64-bit accumulator, the product is mads and one shift per column,
// and the 7 spare bits of the radix (2^261 / q > 169.28) make every conditional subtraction unnecessary.
//
// Plain C++ and one empty asm statement (device builds only, see COLUMN CHAINS): the same text compiles for the device
// (hipcc) and for the host (g++, tools/limb29_check.cpp, where -DZKPOA_LIMB29_CHECK counts column overflows).
//
// OPERAND CLASSES (a value is sum l[i] 2^(29 i); it is a field element only modulo q, never reduced below q here)
//   N  product output        limbs 0..7 < 2^29 ("normalised"), value < 3q
//   X  accumulator X         normalised, value < 13q
//   W  re-limbed 8-word value normalised, value < 2^256 (< 5.3q), limb 8 < 2^24: a wire word, or a word of a PACKED
//                            partial sum (below) -- any of its four coordinates
//   D  difference, sum       NOT normalised: every limb < 3 * 2^29, value < 17q
//   a normalised value V has limb 8 = V >> 232, < 2^26 for V < 17q.
// RULES
//   * a product takes at most ONE class-D operand (dot2: one per product); a D that is squared or meets another D is
//     normalised first (norm: one carry pass, value unchanged).
//   * operand values satisfy va * vb <= 338 q^2 (dot2: the sum of its two products).
// COLUMNS. Column k of a product adds at most 9 a_i b_(k-i), 9 m_i q_(k-i) and the carry of column k-1 (< 2^35).
// mul and sqr keep their quotient limbs m_0..m_7 UNMASKED (32 bits, see QUOTIENT LIMBS), so their m part is bounded
// through q: sum m_i q_(k-i) < 2^32 * (q_0 + ... + q_8) = 2^32 * 1616751127 < 0.377 * 2^64 in any column. Both
// operands normalised: a b part 9 * 2^58 = 0.141 * 2^64, total < 0.52 * 2^64. One operand D, or the negated base
// C6 - W (limbs < 2^30): a b part at most 27 * 2^58 = 0.422 * 2^64, total < 0.80 * 2^64. The square doubles its cross
// terms by doubling one limb (< 2^30): the same sum as the product of two normalised operands.
// dot2 MASKS every m_i (< 2^29); as the mixed addition uses it (r * d + ny * ppp: r, ppp normalised, d < 3 * 2^29,
// ny < 2 * 2^29 per limb): 27 * 2^58 + 18 * 2^58 + 9 * 2^58 = 54 * 2^58; with two D operands of 3 * 2^29:
// 63 * 2^58 + 2^35 < 2^64. (Unmasked, its m part alone would add 0.377 * 2^64 to 54 * 2^58 = 0.844 * 2^64: it keeps
// its masks.) No column reaches 2^64.
// QUOTIENT LIMBS. Column k < 9 needs an m_k with acc + m_k q_0 = 0 (mod 2^29). mt_k = lo32(acc) * INV mod 2^32 is
// such a value: mt_k = m_k (mod 2^29), m_k = mt_k & M the masked one. What mt_k has above bit 29 is a multiple of
// 2^29 q added to the column, i.e. a multiple of q one column up, and column k + 1 computes its own m from the
// accumulator that holds it: every column's low 29 bits still vanish and the sum is still a b + Mt q with
// Mt = sum mt_k 2^(29 k). So the mask (one v_and per column) is spent only where the SIZE of Mt matters: on m_8.
// With m_8 < 2^29 and the others < 2^32, Mt < 2^261 + 2^32 (2^232 - 1) / (2^29 - 1) < 2^261 + 2^235.1.
// Eight masks less in each of the mixed addition's six products and two squares: 64 of its 177 v_and_b32, 2015 -> 1951
// instructions with the same 1467 mads (profiles/loop_mix_quotient_mask_{parent,change}.txt).
// COLUMN CHAINS. A column is written as one chain: acc >>= 29, then acc += a_i b_j ... . v_mad_u64_u32 takes its 64-bit
// addend for free, so the shifted carry can be the addend of the column's first product. Left alone, the compiler's
// reassociation ranks the carry last: it starts every column at 0 beside the tail of the column before and joins the
// two with "v_lshl_add_u64 x, y, 0, x" -- 16 plain 64-bit adds per product, 144 of the 2152 instructions of one mixed
// addition (1467 of them mads), and the accumulation kernel runs at the issue rate of that stream. So on the device
// fq29_mac ends with an empty asm that READS acc: every partial sum then has a second use, sums with two uses are not
// reassociated, and each column stays the one chain it is written as. The mixed addition is 2015 instructions with
// the same 1467 mads and no 64-bit add (profiles/loop_mix_{parent,change}.txt; 16.4 -> 17.8 G additions/s at 3 waves
// per SIMD, profiles/microbench_limb29_column_chain.txt). Two lighter forms were measured and dropped: the marker on a
// column's first product only leaves the rest of the column to be summed from 0 and joined (144 -> 54); an asm that
// also WRITES acc ("+v") removes every join but the hazard pass then puts an s_nop after every mad (1284 in the
// addition: 15.8 G/s, slower than the parent). Reading costs no instruction and no register. The one product that
// opens a chain from acc = 0 with another product behind it (dot2, column 0) carries no marker: it has no carry to
// keep in front, and marked, it is computed twice (the compiler commutes the pair). COLUMNS, VALUES and the operand
// classes are untouched: the same products are added, in the order written, to the same accumulator.
// VALUES. The output is (a b + Mt q) / 2^261 with Mt < 2^261 (1 + 2^-25.9) (dot2: < 2^261):
// < va vb / 2^261 + q (1 + 2^-25.9) <= 338 q^2 / (169.28 q) + 1.00000002 q < 2.9967 q + 0.00000002 q < 3q.
// So N is closed under every product the rules allow; the largest in the mixed addition is 17q * 17q = 289 q^2.
// SUBTRACTION is a + (C - b) per limb, C = k q in a "borrowed" representation whose limbs are all >= the largest
// limb b can have (limbs 0..7: d_i + 2^29 - 1 with a borrow of one from the limb above; limb 8: d_8 - 1, which has to
// be >= b >> 232, i.e. k q exceeds b's value bound by 2^232): nothing goes negative, per limb or in value.
//   C4  = 4q   subtrahend N (< 3q);          limbs < 2^30
//   C6  = 6q   subtrahend W (< 2^256);       limbs < 2^30
//   C14 = 14q  subtrahend X (< 13q);         limbs < 2^30
//   C10 = 10q  subtrahend ppp + 2 Q (limbs < 3 * 2^29, value < 9q): borrow of 4, limbs < 5 * 2^29
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ZK29 __host__ __device__ __forceinline__
#else
#define ZK29 inline
#endif

namespace zkpoa {

#if defined(ZKPOA_LIMB29_CHECK)
static uint64_t limb29_overflows = 0;   // host builds only: columns that left 64 bits
#endif

struct Fq29 {
  uint32_t l[9];
};

struct Fq29P {
  static constexpr uint32_t M = 0x1fffffffu;
  static constexpr uint32_t INV = 0x04866389u;   // -q^-1 mod 2^29
  static constexpr uint32_t Q[9] = {0x187cfd47u, 0x010460b6u, 0x1c72a34fu, 0x02d522d0u, 0x1585d978u,
                                    0x02db40c0u, 0x00a6e141u, 0x0e5c2634u, 0x0030644eu};
};
struct Fq29Q2 {   // 2q, normalised
  static constexpr uint32_t v[9] = {0x10f9fa8eu, 0x0208c16du, 0x18e5469eu, 0x05aa45a1u, 0x0b0bb2f0u,
                                    0x05b68181u, 0x014dc282u, 0x1cb84c68u, 0x0060c89cu};
};
struct Fq29C4 {
  static constexpr uint32_t v[9] = {0x21f3f51cu, 0x241182dau, 0x31ca8d3bu, 0x2b548b42u, 0x361765dfu,
                                    0x2b6d0301u, 0x229b8503u, 0x397098cfu, 0x00c19138u};
};
struct Fq29C6 {
  static constexpr uint32_t v[9] = {0x32edefaau, 0x261a4447u, 0x2aafd3d9u, 0x30fed0e4u, 0x212318cfu,
                                    0x31238483u, 0x23e94785u, 0x3628e537u, 0x012259d5u};
};
struct Fq29C10 {
  static constexpr uint32_t v[9] = {0x94e1e4c6u, 0x8a2bc71fu, 0x9c7a6112u, 0x9c535c24u, 0x973a7eacu,
                                    0x9c908782u, 0x8684cc86u, 0x8f997e04u, 0x01e3eb0cu};
};
struct Fq29C14 {
  static constexpr uint32_t v[9] = {0x36d5d9e2u, 0x2e3d49fdu, 0x2e44ee51u, 0x27a7e76bu, 0x2d51e490u,
                                    0x27fd8a88u, 0x2920518eu, 0x290a16d7u, 0x02a57c49u};
};
// 2^e mod q, normalised: domain changes by one product (x 2^e / 2^261)
struct Fq29K266 {
  static constexpr uint32_t v[9] = {0x13349ca1u, 0x1a5d84a8u, 0x0a3e5cacu, 0x100249e0u, 0x12b951e8u,
                                    0x0e92d304u, 0x14cb95b3u, 0x041b9d3du, 0x00058003u};
};
struct Fq29K271 {
  static constexpr uint32_t v[9] = {0x1d1c9c4bu, 0x08a372eeu, 0x1273abadu, 0x17c9d397u, 0x1698b0a7u,
                                    0x09c89e50u, 0x177e12abu, 0x185f3518u, 0x001ed378u};
};
struct Fq29K256 {
  static constexpr uint32_t v[9] = {0x058f0d9du, 0x1aea1c6eu, 0x11c2cf74u, 0x11d651ebu, 0x1462c0a7u,
                                    0x11b7bc3cu, 0x1cbd99bau, 0x183340fbu, 0x000e0a77u};
};
struct Fq29K251 {
  static constexpr uint32_t v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0x00080000u};
};

template <class C>
ZK29 Fq29 fq29_const() {
  Fq29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = C::v[i];
  return r;
}

// acc += a * b: one v_mad_u64_u32, no carry-out (see COLUMNS). The product that opens a column chain with nothing in
// front of it (acc = 0) where another product follows at once: no use to mark, see COLUMN CHAINS.
ZK29 void fq29_mac_open(uint64_t& acc, uint32_t a, uint32_t b) {
#if defined(ZKPOA_LIMB29_CHECK)
  if (__builtin_add_overflow(acc, (uint64_t)a * b, &acc)) limb29_overflows++;
#else
  acc += (uint64_t)a * b;
#endif
}
// The same, and the sum is USED a second time on the device (an empty asm that reads it: no instruction): see COLUMN
// CHAINS. On the host this is fq29_mac_open.
ZK29 void fq29_mac(uint64_t& acc, uint32_t a, uint32_t b) {
  fq29_mac_open(acc, a, b);
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : : "v"(acc));
#endif
}

// ---- 8 x 32 <-> 9 x 29: bit slicing only -------------------------------------------------------------------------
ZK29 Fq29 fq29_from_words(const uint32_t* w) {   // any 256-bit value -> class W
  Fq29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const int bo = 29 * i, wd = bo >> 5, sh = bo & 31;
    uint64_t two = w[wd];
    if (wd + 1 < 8) two |= (uint64_t)w[wd + 1] << 32;
    r.l[i] = (uint32_t)(two >> sh) & Fq29P::M;
  }
  return r;
}
ZK29 void fq29_to_words(const Fq29& a, uint32_t* w) {   // normalised, value < 2^256
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int i0 = (32 * j) / 29, off = 32 * j - 29 * i0;
    uint64_t t = a.l[i0] >> off;
    t |= (uint64_t)a.l[i0 + 1] << (29 - off);
    if (i0 + 2 < 9) t |= (uint64_t)a.l[i0 + 2] << (58 - off);
    w[j] = (uint32_t)t;
  }
}

// value = 0 (mod q) for a class-N value: 0, q or 2q
ZK29 bool fq29_is_zero_mod_q(const Fq29& a) {
  uint32_t d0 = 0, d1 = 0, d2 = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    d0 |= a.l[i];
    d1 |= a.l[i] ^ Fq29P::Q[i];
    d2 |= a.l[i] ^ Fq29Q2::v[i];
  }
  return d0 == 0 || d1 == 0 || d2 == 0;
}
// class X (any normalised value with limb 8 < 2^26) -> the same field element below 2^256, normalised, by a quotient
// estimate: k = limb 8 / ((q >> 232) + 1) never exceeds value / q, so value - k q >= 0, and limb 8 < (k + 1)(q8 + 1)
// leaves value - k q < (q8 + k + 1) 2^232 < q + 14 * 2^232. Nine multiply-adds and one division by a constant; the
// alternative, a product by 2^261 mod q, is a whole Montgomery product (162).
ZK29 Fq29 fq29_below_2p256(const Fq29& a) {
  const uint32_t k = a.l[8] / ((Fq29P::Q[8]) + 1u);
  Fq29 r;
  int64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (int64_t)a.l[i] - (int64_t)((uint64_t)k * Fq29P::Q[i]);
    r.l[i] = (uint32_t)c & Fq29P::M;
    c >>= 29;
  }
  r.l[8] = (uint32_t)((int64_t)a.l[8] - (int64_t)((uint64_t)k * Fq29P::Q[8]) + c);
  return r;
}

// 32 a for a of class W or the negated base C6 - W (limbs < 2^30, value < 6q: 32 a < 192q does not fit 2^261, its limb
// 8 needs 31 bits), brought below q (1 + 2^-13): normalised, class N and class X at once. This is the product by
// 2^266 mod q (a wire word into the accumulator's X, Y domain) without a product. The limbs are shifted in place,
// t_i = (a_i mod 2^24) 2^5 + (a_(i-1) >> 24) < 2^29 + 64 and t_8 = 32 a_8 + (a_7 >> 24) < 2^30 + 64 (a_8 < 6 (q_8 + 1)
// < 2^25), nothing carried; then the quotient estimate of fq29_below_2p256, k = t_8 / (q_8 + 1) <= 192: k q <
// k (q_8 + 1) 2^232 <= t_8 2^232 <= 32 a, so nothing goes negative, and with t_8 + 1 <= (k + 1)(q_8 + 1) and the limbs
// below t_8 summing to less than 2^232 (1 + 2^-22), 32 a - k q < (q_8 + k + 1 + 2^-22) 2^232 < q + 194 * 2^232.
// The subtraction's carry pass normalises. 9 multiply-adds, against the product's 162.
ZK29 Fq29 fq29_times32(const Fq29& a) {
  uint32_t t[9];
  t[0] = (a.l[0] & 0xffffffu) << 5;
#pragma unroll
  for (int i = 1; i < 8; i++) t[i] = ((a.l[i] & 0xffffffu) << 5) + (a.l[i - 1] >> 24);
  t[8] = (a.l[8] << 5) + (a.l[7] >> 24);
  const uint32_t k = t[8] / ((Fq29P::Q[8]) + 1u);
  Fq29 r;
  int64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (int64_t)t[i] - (int64_t)((uint64_t)k * Fq29P::Q[i]);
    r.l[i] = (uint32_t)c & Fq29P::M;
    c >>= 29;
  }
  r.l[8] = (uint32_t)((int64_t)t[8] - (int64_t)((uint64_t)k * Fq29P::Q[8]) + c);
  return r;
}
// a / 32 for a normalised a: one 5-bit Montgomery step, (a + m q) >> 5 with m = a_0 * INV mod 32 (INV = -1/q mod 2^29
// is -1/q mod 32 as well), value (a + m q) / 32 < (va + 31 q) / 32: class N (< 3q) gives < 1.0625 q, normalised. This
// is the product by 2^256 mod q (2^266 to 2^261) without a product. a = 0 (mod q), i.e. j q with j <= 2, gives
// (j + m) q / 32 with j + m <= 33 a multiple of 32: 0 or q, never another representative. The shift is folded into the
// carry pass: limb i enters at bit 29 i - 5 = 29 (i - 1) + 24, so the accumulator stays below 2^60.
ZK29 Fq29 fq29_div32(const Fq29& a) {
  const uint32_t m = (a.l[0] * Fq29P::INV) & 31u;
  Fq29 r;
  uint64_t acc = ((uint64_t)a.l[0] + (uint64_t)m * Fq29P::Q[0]) >> 5;
#pragma unroll
  for (int i = 1; i < 9; i++) {
    acc += ((uint64_t)a.l[i] + (uint64_t)m * Fq29P::Q[i]) << 24;
    r.l[i - 1] = (uint32_t)acc & Fq29P::M;
    acc >>= 29;
  }
  r.l[8] = (uint32_t)acc;
  return r;
}

// ---- sums and differences (class D results) ---------------------------------------------------------------------
ZK29 Fq29 fq29_norm(const Fq29& a) {   // one carry pass: limbs 0..7 < 2^29, value unchanged
  Fq29 r;
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint32_t t = a.l[i] + c;
    r.l[i] = t & Fq29P::M;
    c = t >> 29;
  }
  r.l[8] = a.l[8] + c;
  return r;
}
template <class C>
ZK29 Fq29 fq29_sub(const Fq29& a, const Fq29& b) {   // a + (C - b): b of the class C is made for
  Fq29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = a.l[i] + (C::v[i] - b.l[i]);
  return r;
}
template <class C>
ZK29 Fq29 fq29_neg(const Fq29& b) {   // C - b
  Fq29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = C::v[i] - b.l[i];
  return r;
}

// ---- Montgomery products, radix 2^261, product scanning ---------------------------------------------------------
// column k < 9 fixes m_k so that the column's low 29 bits vanish (mul, sqr: m_0..m_7 unmasked, see QUOTIENT LIMBS);
// columns 9..16 leave limbs 0..7 and what remains of the accumulator is limb 8. No final subtraction (see VALUES).
ZK29 Fq29 fq29_mul(const Fq29& a, const Fq29& b) {
  uint64_t acc = 0;
  uint32_t m[9];
  Fq29 r;
#pragma unroll
  for (int k = 0; k < 9; k++) {
#pragma unroll
    for (int i = 0; i <= k; i++) fq29_mac(acc, a.l[i], b.l[k - i]);
#pragma unroll
    for (int i = 0; i < k; i++) fq29_mac(acc, m[i], Fq29P::Q[k - i]);
    m[k] = (uint32_t)acc * Fq29P::INV;
    if (k == 8) m[k] &= Fq29P::M;
    fq29_mac(acc, m[k], Fq29P::Q[0]);
    acc >>= 29;
  }
#pragma unroll
  for (int k = 9; k < 17; k++) {
#pragma unroll
    for (int i = k - 8; i < 9; i++) fq29_mac(acc, a.l[i], b.l[k - i]);
#pragma unroll
    for (int i = k - 8; i < 9; i++) fq29_mac(acc, m[i], Fq29P::Q[k - i]);
    r.l[k - 9] = (uint32_t)acc & Fq29P::M;
    acc >>= 29;
  }
  r.l[8] = (uint32_t)acc;
  return r;
}
// a^2: the 36 cross products once, against a doubled limb (45 + 81 mads instead of 81 + 81). a normalised.
ZK29 Fq29 fq29_sqr(const Fq29& a) {
  uint32_t d[9];
#pragma unroll
  for (int i = 0; i < 9; i++) d[i] = a.l[i] << 1;
  uint64_t acc = 0;
  uint32_t m[9];
  Fq29 r;
#pragma unroll
  for (int k = 0; k < 9; k++) {
#pragma unroll
    for (int i = 0; 2 * i < k; i++) fq29_mac(acc, a.l[i], d[k - i]);
    if ((k & 1) == 0) fq29_mac(acc, a.l[k / 2], a.l[k / 2]);
#pragma unroll
    for (int i = 0; i < k; i++) fq29_mac(acc, m[i], Fq29P::Q[k - i]);
    m[k] = (uint32_t)acc * Fq29P::INV;
    if (k == 8) m[k] &= Fq29P::M;
    fq29_mac(acc, m[k], Fq29P::Q[0]);
    acc >>= 29;
  }
#pragma unroll
  for (int k = 9; k < 17; k++) {
#pragma unroll
    for (int i = k - 8; 2 * i < k; i++) fq29_mac(acc, a.l[i], d[k - i]);
    if ((k & 1) == 0) fq29_mac(acc, a.l[k / 2], a.l[k / 2]);
#pragma unroll
    for (int i = k - 8; i < 9; i++) fq29_mac(acc, m[i], Fq29P::Q[k - i]);
    r.l[k - 9] = (uint32_t)acc & Fq29P::M;
    acc >>= 29;
  }
  r.l[8] = (uint32_t)acc;
  return r;
}
// (a0 b0 + a1 b1) / 2^261 under one reduction
ZK29 Fq29 fq29_dot2(const Fq29& a0, const Fq29& b0, const Fq29& a1, const Fq29& b1) {
  uint64_t acc = 0;
  uint32_t m[9];
  Fq29 r;
#pragma unroll
  for (int k = 0; k < 9; k++) {
#pragma unroll
    for (int i = 0; i <= k; i++) {
      if (k == 0) fq29_mac_open(acc, a0.l[0], b0.l[0]);
      else fq29_mac(acc, a0.l[i], b0.l[k - i]);
      fq29_mac(acc, a1.l[i], b1.l[k - i]);
    }
#pragma unroll
    for (int i = 0; i < k; i++) fq29_mac(acc, m[i], Fq29P::Q[k - i]);
    m[k] = ((uint32_t)acc * Fq29P::INV) & Fq29P::M;
    fq29_mac(acc, m[k], Fq29P::Q[0]);
    acc >>= 29;
  }
#pragma unroll
  for (int k = 9; k < 17; k++) {
#pragma unroll
    for (int i = k - 8; i < 9; i++) {
      fq29_mac(acc, a0.l[i], b0.l[k - i]);
      fq29_mac(acc, a1.l[i], b1.l[k - i]);
    }
#pragma unroll
    for (int i = k - 8; i < 9; i++) fq29_mac(acc, m[i], Fq29P::Q[k - i]);
    r.l[k - 9] = (uint32_t)acc & Fq29P::M;
    acc >>= 29;
  }
  r.l[8] = (uint32_t)acc;
  return r;
}

// ---- G1 accumulator ---------------------------------------------------------------------------------------------
// Point (X / ZZ, Y / ZZZ) with X, Y held times 2^261 and ZZ, ZZZ times 2^266. A wire base (x 2^256, y 2^256) then
// needs no conversion: (x 2^256)(ZZ 2^266) / 2^261 = x ZZ 2^261 lands in X's domain, and every later product of
// madd-2008-s closes: pp, ppp, q in 2^261; ZZ pp, ZZZ ppp in 2^266. x, y: class X and N; zz, zzz: class N.
struct Xyzz29 {
  Fq29 x, y, zz, zzz;
};

// acc = (bx, by): bx class W, by class W or C6 - W. 2^256 to 2^261 is a factor of 32: no product (fq29_times32);
// X and Y come out normalised and below q (1 + 2^-13), inside class X and class N.
ZK29 void xyzz29_open(Xyzz29& acc, const Fq29& bx, const Fq29& by) {
  const Fq29 k = fq29_const<Fq29K266>();
  acc.x = fq29_times32(bx);
  acc.y = fq29_times32(by);
  acc.zz = k;
  acc.zzz = k;
}
// acc from wire XYZZ words (class W each), any representative of a non-infinity point
ZK29 void xyzz29_from_wire(Xyzz29& acc, const Fq29& x, const Fq29& y, const Fq29& zz, const Fq29& zzz) {
  const Fq29 k0 = fq29_const<Fq29K266>(), k1 = fq29_const<Fq29K271>();
  acc.x = fq29_mul(x, k0);
  acc.y = fq29_mul(y, k0);
  acc.zz = fq29_mul(zz, k1);
  acc.zzz = fq29_mul(zzz, k1);
}
// back to the wire domain (2^256), class N: the caller re-limbs and stores canonically
ZK29 void xyzz29_to_wire(const Xyzz29& acc, Fq29& x, Fq29& y, Fq29& zz, Fq29& zzz) {
  const Fq29 k0 = fq29_const<Fq29K256>(), k1 = fq29_const<Fq29K251>();
  x = fq29_mul(acc.x, k0);
  y = fq29_mul(acc.y, k0);
  zz = fq29_mul(acc.zz, k1);
  zzz = fq29_mul(acc.zzz, k1);
}

// acc += (bx, by), generic case only [madd-2008-s]: no test for acc = +-base. There pp_ = 0 (mod q), so ZZ becomes
// 0 (mod q) and STAYS 0 through every later addition: the caller tests ZZ once at the end and redoes the piece with
// the exact xyzz_add_affine. bx class W; by class W, or C6 - W for a negated base (limbs < 2^30, value < 6q).
// Value products: u2 5.3 * 3, s2 6 * 3, pp 17^2 = 289, rr 7^2, ppp 17 * 3, q 13 * 3, y 7 * 17 + 4 * 3 = 131, zz 9.
ZK29 void xyzz29_madd(Xyzz29& acc, const Fq29& bx, const Fq29& by) {
  const Fq29 u2 = fq29_mul(bx, acc.zz);
  const Fq29 s2 = fq29_mul(by, acc.zzz);
  const Fq29 p = fq29_norm(fq29_sub<Fq29C14>(u2, acc.x));   // < 3q + 14q
  const Fq29 r = fq29_norm(fq29_sub<Fq29C4>(s2, acc.y));    // < 3q + 4q
  const Fq29 pp = fq29_sqr(p);
  const Fq29 rr = fq29_sqr(r);
  const Fq29 ppp = fq29_mul(p, pp);
  const Fq29 q = fq29_mul(acc.x, pp);
  Fq29 t;   // x3 = rr - ppp - 2q = rr + (C10 - (ppp + 2q)): limbs < 6 * 2^29, value < 3q + 10q
#pragma unroll
  for (int i = 0; i < 9; i++) t.l[i] = rr.l[i] + (Fq29C10::v[i] - (ppp.l[i] + 2u * q.l[i]));
  const Fq29 x3 = fq29_norm(t);
  // y3 = r (q - x3) - y1 ppp, one reduction: q - x3 class D (< 3q + 14q), -y1 = C4 - y1 (limbs < 2^30, < 4q)
  acc.y = fq29_dot2(r, fq29_sub<Fq29C14>(q, x3), fq29_neg<Fq29C4>(acc.y), ppp);
  acc.x = x3;
  acc.zz = fq29_mul(acc.zz, pp);
  acc.zzz = fq29_mul(acc.zzz, ppp);
}

// One piece of a bucket: a sum of wire-format affine bases (x then y, 8 words each, all-zero = infinity).
struct G1Piece29 {
  Xyzz29 a;
  bool empty;
};
ZK29 void g1piece29_add(G1Piece29& s, const uint32_t* xw, const uint32_t* yw, bool negate) {
  uint32_t any = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) any |= xw[i] | yw[i];
  if (any == 0) return;   // infinity base
  const Fq29 bx = fq29_from_words(xw);
  Fq29 by = fq29_from_words(yw);
#pragma unroll
  for (int i = 0; i < 9; i++) by.l[i] = negate ? Fq29C6::v[i] - by.l[i] : by.l[i];
  if (s.empty) {
    xyzz29_open(s.a, bx, by);
    s.empty = false;
  } else {
    xyzz29_madd(s.a, bx, by);
  }
}
// wire XYZZ words of the sum, each < 3q and NOT canonical; all zero for an empty piece. A result whose ZZ is
// 0 (mod q) is not a sum: the piece met acc = +-base and has to be redone with the exact addition.
ZK29 void g1piece29_finish(const G1Piece29& s, uint32_t* out32) {
  if (s.empty) {
#pragma unroll
    for (int i = 0; i < 32; i++) out32[i] = 0;
    return;
  }
  Fq29 x, y, zz, zzz;
  xyzz29_to_wire(s.a, x, y, zz, zzz);
  fq29_to_words(x, out32);
  fq29_to_words(y, out32 + 8);
  fq29_to_words(zz, out32 + 16);
  fq29_to_words(zzz, out32 + 24);
}

// acc += b, generic case only [add-2008-s], both in ONE domain (all four coordinates times 2^261: the domain the
// partial sums keep between the kernels, packed form below). acc = +-b leaves ZZ = 0 (mod q), as above.
struct Xyzz29S {
  Fq29 x, y, zz, zzz;   // x class X, the others class N
};
ZK29 void xyzz29s_from_wire(Xyzz29S& a, const Fq29& x, const Fq29& y, const Fq29& zz, const Fq29& zzz) {
  const Fq29 k = fq29_const<Fq29K266>();
  a.x = fq29_mul(x, k);
  a.y = fq29_mul(y, k);
  a.zz = fq29_mul(zz, k);
  a.zzz = fq29_mul(zzz, k);
}
ZK29 void xyzz29s_to_wire(const Xyzz29S& a, Fq29& x, Fq29& y, Fq29& zz, Fq29& zzz) {
  const Fq29 k = fq29_const<Fq29K256>();
  x = fq29_mul(a.x, k);
  y = fq29_mul(a.y, k);
  zz = fq29_mul(a.zz, k);
  zzz = fq29_mul(a.zzz, k);
}
// Value products: u1 13 * 3, u2 13 * 3, s1, s2 9, pp 7^2, ppp 7 * 3, q 9, y 7 * 17 + 4 * 3, zz 9.
// With operands loaded from the packed form (below) any coordinate may be class W (< 5.3q) instead of N, and x is X or
// W: u1, u2 13 * 5.3 = 69, s1, s2 5.3^2 = 28.1, zz1 zz2 and zzz1 zzz2 28.1; everything after the first four products
// sees product outputs only (u1, s1, p, r: as above), so the largest stays y at 131 <= 338. COLUMNS: every loaded
// limb is normalised (limbs 0..7 < 2^29 by the slicing, limb 8 < 2^24), so the products that take loaded operands
// are "both operands normalised" (< 18 * 2^58); the D operands are the same three as above.
ZK29 void xyzz29s_add(Xyzz29S& acc, const Xyzz29S& b) {
  // (order: each input coordinate dies as early as it can -- at most 7 field elements live besides the product at work)
  const Fq29 u1 = fq29_mul(acc.x, b.zz);
  const Fq29 u2 = fq29_mul(b.x, acc.zz);
  const Fq29 zz12 = fq29_mul(acc.zz, b.zz);
  const Fq29 p = fq29_norm(fq29_sub<Fq29C4>(u2, u1));
  const Fq29 s1 = fq29_mul(acc.y, b.zzz);
  const Fq29 s2 = fq29_mul(b.y, acc.zzz);
  const Fq29 zzz12 = fq29_mul(acc.zzz, b.zzz);
  const Fq29 r = fq29_norm(fq29_sub<Fq29C4>(s2, s1));
  const Fq29 pp = fq29_sqr(p);
  const Fq29 rr = fq29_sqr(r);
  const Fq29 ppp = fq29_mul(p, pp);
  const Fq29 q = fq29_mul(u1, pp);
  Fq29 t;
#pragma unroll
  for (int i = 0; i < 9; i++) t.l[i] = rr.l[i] + (Fq29C10::v[i] - (ppp.l[i] + 2u * q.l[i]));
  const Fq29 x3 = fq29_norm(t);
  acc.y = fq29_dot2(r, fq29_sub<Fq29C14>(q, x3), fq29_neg<Fq29C4>(s1), ppp);
  acc.x = x3;
  acc.zz = fq29_mul(zz12, pp);
  acc.zzz = fq29_mul(zzz12, ppp);
}


// ---- packed partial sums: 128 bytes, the form between the kernels ------------------------------------------------
// A G1 partial sum in HBM is its Xyzz29S (all four coordinates times 2^261) with every coordinate brought below 2^256
// and re-limbed into 8 words: x then y, zz, zzz. Infinity is 32 zero words (a sum's ZZ is never 0 as a value: poison
// is not stored, and a non-infinity ZZ is a non-zero field element). y, zz, zzz are class N or W and fit as they
// are; x is class X and is reduced by fq29_below_2p256. Loading is bit slicing only: every coordinate comes back class W.
// A stored ZZ is always class N (< 3q) -- a piece's closing division by 32 (< 1.0625 q), an addition's or a conversion's
// product output, or such a word loaded and stored again unchanged -- which is what lets fq29_is_zero_mod_q test a
// sum's ZZ against 0, q, 2q.
ZK29 void xyzz29s_pack(const Xyzz29S& a, uint32_t* w32) {
  fq29_to_words(fq29_below_2p256(a.x), w32);
  fq29_to_words(a.y, w32 + 8);
  fq29_to_words(a.zz, w32 + 16);
  fq29_to_words(a.zzz, w32 + 24);
}
ZK29 void xyzz29s_unpack(Xyzz29S& a, const uint32_t* w32) {
  a.x = fq29_from_words(w32);
  a.y = fq29_from_words(w32 + 8);
  a.zz = fq29_from_words(w32 + 16);
  a.zzz = fq29_from_words(w32 + 24);
}
// the piece's sum in the single domain: ZZ, ZZZ from 2^266 to 2^261 (a division by 32 each: fq29_div32, no product;
// class N in, normalised and below 1.0625 q out), X and Y as they are. False if it is not a sum (ZZ = 0 mod q: the
// piece met acc = +-base, and a ZZ of 0, q or 2q divides to 0 or q); the piece must not be empty.
ZK29 bool g1piece29_close(const G1Piece29& s, Xyzz29S& out) {
  out.x = s.a.x;
  out.y = s.a.y;
  out.zz = fq29_div32(s.a.zz);
  out.zzz = fq29_div32(s.a.zzz);
  return !fq29_is_zero_mod_q(out.zz);
}

}  // namespace zkpoa
