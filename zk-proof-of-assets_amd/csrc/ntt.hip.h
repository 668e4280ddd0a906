// Radix-2 number-theoretic transform over the BN254 scalar field Fr for gfx950, LDS-staged.
//
// Replaces Fr.fft / Fr.ifft / Fr.batchApplyKey of ffjavascript as used by snarkjs
// groth16_prove.js and rapidsnark's fft.hpp: six size-n
// transforms per proof, w = w[log2 n] (5^((r-1)/2^28) squared down), elements in Montgomery form.
//
// Structure: the log2(n) butterfly stages are cut into passes of B <= 11 consecutive stages.
// One workgroup stages a tile of 2^B rows x T columns (2048 elements, 64 KiB; 1024 from 2^23 up) in LDS, runs
// the B stages there, two per barrier, and writes the tile back: every pass reads and
// writes each element once (HBM-bound part), all butterflies run out of LDS.
//   * DIF (Gentleman-Sande) passes go from the top stage down: natural order in, bit-reversed out.
//   * DIT (Cooley-Tukey) passes go from stage 0 up: bit-reversed in, natural order out.
// Between passes the four-step twiddle W_n^((n/N') * ka * rev_B(m)) is applied on the way out
// (DIF) or in (DIT), looked up as Hi[e >> L] * Lo[e & (2^L - 1)] from two small tables, so inside
// a pass every butterfly twiddle is a plain 2^B-th root from a 2^(B-1)-entry table.
// The prover chain ifft -> coset shift -> fft is DIF(w^-1) -> DIT(w) with the coset factor inc^j / n multiplied in
// as the forward transform's first pass loads its tile: no bit-reversal permutation and no scaling pass at all.
// The natural-order API (Fr.fft / Fr.ifft) stores its last pass at the bit-reversed position (times 1/n).
// Boundary twiddles of a pass whose table fits the cache (2^21 entries) are read as ONE value per element.
#pragma once
#include "bn254_field.hip.h"
#include "host_field.hpp"
#include "zkpoa_internal.hpp"

#include <deque>
#include <memory>
#include <vector>

namespace zkpoa {

constexpr uint32_t kNttStridedB = 8;  // at most 2^8 rows per tile where the strided stages take several passes
constexpr uint32_t kNttDirectMaxLog = 21;  // boundary twiddles as one table up to 2^21 entries (64 MiB, cache-resident)
// threads per 2048-element tile: 8 waves share the 64 KiB tile, so with 2 tiles per CU every SIMD has 4 waves
// to cover the multiply latency and the per-stage barriers (measured at 2^26: 256 threads +10 %, 1024 +10 %)
constexpr uint32_t kNttThreads = 512;

// T[i] = scale * base^(i * step) for i < count  (all Montgomery)
static __global__ __launch_bounds__(256) void fr_pow_table_kernel(Fr base, Fr scale, uint32_t count, void* out) {
  uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= count) return;
  Fr acc = scale, b = base;
  uint32_t e = i;
  while (e) {
    if (e & 1u) acc = acc * b;
    b = b.sqr();
    e >>= 1;
  }
  store_field(reinterpret_cast<char*>(out) + 32 * (size_t)i, acc);
}

// W^e from the two-level table: e = eh * 2^L + el
ZK_DEV Fr tw_lookup(const void* __restrict__ hi, const void* __restrict__ lo, uint32_t L, uint32_t e) {
  Fr a = load_field<Fr>(reinterpret_cast<const char*>(hi) + 32 * (size_t)(e >> L));
  Fr b = load_field<Fr>(reinterpret_cast<const char*>(lo) + 32 * (size_t)(e & ((1u << L) - 1u)));
  return a * b;
}

// The tile lives in LDS as two planes of 16-byte halves (low limbs of every element, then high limbs): consecutive
// lanes then touch consecutive 16-byte words. With the halves interleaved (32-byte stride) lanes i and i + 8 of a
// ds_read_b128 group fall on the same banks: a two-way conflict on every access of every stage.
ZK_DEV Fr lds_load(const uint4* lds, uint32_t plane, uint32_t idx) {
  uint4 a = lds[idx], b = lds[plane + idx];
  Fr r;
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
  r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
  return r;
}
ZK_DEV void lds_store(uint4* lds, uint32_t plane, uint32_t idx, const Fr& v) {
  lds[idx] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  lds[plane + idx] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

// What a pass folds into its load / store besides the butterflies (each saves a whole 64 B/element round trip):
//   kPassPlain      nothing
//   kPassPreScale   DIT pass over stages [0, B): every element is multiplied on load by X^j, j = bitrev_k(p), from a
//                   two-level table (the coset shift inc^j / n between the inverse and the forward transform)
//   kPassBitrevOut  DIF pass over stages [0, B): the result is stored at bitrev_k(p), times `post` (1/n of the
//                   inverse; one) -- the natural-order output of Fr.fft / Fr.ifft without a permutation kernel
enum NttPassMode { kPassPlain = 0, kPassPreScale = 1, kPassBitrevOut = 2 };

// boundary twiddle table of a strided pass laid out like the tile rows: D[(r << s_lo) + col] = W^((col * r) << shift)
static __global__ __launch_bounds__(256) void ntt_direct_table_kernel(void* __restrict__ out, uint32_t s_lo, uint32_t B,
                                                                      uint32_t shift, const void* __restrict__ hi,
                                                                      const void* __restrict__ lo, uint32_t L) {
  uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >> (s_lo + B)) return;
  uint32_t col = i & ((1u << s_lo) - 1u), r = i >> s_lo;
  store_field(reinterpret_cast<char*>(out) + 32 * (size_t)i, tw_lookup(hi, lo, L, (col * r) << shift));
}

// v times the four-step twiddle W^((col * r) << shift) of tile row m (r = bitrev_B(m)) and column `col` of a pass over
// stages [s_lo, s_lo + B): one value from the pass's direct table where it has one, else hi * lo. DIT passes apply it as
// they load, DIF passes as they store.
ZK_DEV Fr times_boundary_twiddle(const Fr& v, const void* __restrict__ direct, const void* __restrict__ hi,
                                 const void* __restrict__ lo, uint32_t L, uint32_t s_lo, uint32_t B, uint32_t shift,
                                 uint32_t m, uint32_t col) {
  const uint32_t r = __brev(m) >> (32u - B);
  if (direct) return v * load_field<Fr>(reinterpret_cast<const char*>(direct) + 32 * (((size_t)r << s_lo) + col));
  return v * tw_lookup(hi, lo, L, (col * r) << shift);
}

// One pass over stages [s_lo, s_lo + B). Tile: 2^B rows (stride 2^s_lo elements) x 2^logT columns
// (consecutive elements); requires logT <= s_lo. grid.x = n / 2^(B+logT). tw_direct (optional): the boundary
// twiddles of this pass as one table (a single multiplication per element instead of hi * lo and then the product).
// blockIdx.y = which of `batch` equally sized vectors, `batch_stride` bytes apart (the prover transforms A, B and C
// of a proof together: a third of the launches, three times the workgroups per launch, one set of twiddle tables).
// Two butterfly stages per barrier: every thread takes the four rows of a radix-4 group through both stages in
// registers (half the LDS round trips and barriers; the multiplication count is unchanged: in a prime field the
// "free" rotation by i of a complex radix-4 butterfly is an ordinary product). An odd B ends with one radix-2 stage.
template <bool DIF, int MODE>
static __global__ __launch_bounds__(kNttThreads) void ntt_pass_kernel(const void* src, void* dst, size_t batch_stride,
                                                              uint32_t k, uint32_t s_lo,
                                                              uint32_t B, uint32_t logT,
                                                              const void* __restrict__ small_tw,
                                                              const void* __restrict__ tw_hi,
                                                              const void* __restrict__ tw_lo, uint32_t L,
                                                              const void* __restrict__ tw_direct,
                                                              const void* __restrict__ sc_hi,
                                                              const void* __restrict__ sc_lo, uint32_t Lc, Fr post) {
  extern __shared__ __attribute__((aligned(16))) uint4 lds[];
  const uint32_t T = 1u << logT, tile = 1u << (B + logT), tid = threadIdx.x, nthr = blockDim.x;
  const uint32_t cg_count = (1u << s_lo) >> logT;
  const uint32_t cg = blockIdx.x % cg_count;
  const uint64_t U = blockIdx.x / cg_count;
  const uint64_t base = (U << (s_lo + B)) + (uint64_t)cg * T;
  const uint32_t shift = k - (s_lo + B);  // log2(n / N')
  const char* sp = reinterpret_cast<const char*>(src) + (size_t)blockIdx.y * batch_stride;
  char* d = reinterpret_cast<char*>(dst) + (size_t)blockIdx.y * batch_stride;

  for (uint32_t e = tid; e < tile; e += nthr) {
    uint32_t c = e & (T - 1u), m = e >> logT;
    uint64_t p = base + ((uint64_t)m << s_lo) + c;
    Fr v = load_field<Fr>(sp + 32 * p);
    if (!DIF && s_lo > 0) v = times_boundary_twiddle(v, tw_direct, tw_hi, tw_lo, L, s_lo, B, shift, m, cg * T + c);
    if (MODE == kPassPreScale) v = v * tw_lookup(sc_hi, sc_lo, Lc, __brev((uint32_t)p) >> (32u - k));
    lds_store(lds, tile, e, v);
  }
  __syncthreads();

  const char* stw = reinterpret_cast<const char*>(small_tw);
  uint32_t it = 0;
  while (it < B) {
    if (B - it >= 2u) {
      // stages (sl, sl + 1), sl = the lower one: rows m0 + {0, h, 2h, 3h}, h = 2^sl, j = m0 mod h.
      // twiddles: t1 = W_{2h}^j (stage sl, both pairs), t2 = W_{4h}^j and t3 = W_{4h}^(j + h) (stage sl + 1)
      const uint32_t sl = DIF ? (B - 2u - it) : it;
      const uint32_t h = 1u << sl;
      for (uint32_t q = tid; q < (tile >> 2); q += nthr) {
        const uint32_t c = q & (T - 1u), mq = q >> logT;
        const uint32_t j = mq & (h - 1u);
        const uint32_t m0 = ((mq >> sl) << (sl + 2u)) | j;
        const uint32_t i0 = (m0 << logT) + c, st = h << logT;
        Fr x0 = lds_load(lds, tile, i0), x1 = lds_load(lds, tile, i0 + st), x2 = lds_load(lds, tile, i0 + 2u * st),
           x3 = lds_load(lds, tile, i0 + 3u * st);
        if (DIF) {
          Fr a0 = x0 + x2, a2 = x0 - x2, a1 = x1 + x3, a3 = x1 - x3;
          a3 = a3 * load_field<Fr>(stw + 32 * (size_t)((j + h) << (B - 2u - sl)));
          if (sl) {   // sl == 0: j = 0, so t2 = t1 = 1 (uniform branch)
            a2 = a2 * load_field<Fr>(stw + 32 * (size_t)(j << (B - 2u - sl)));
            const Fr t1 = load_field<Fr>(stw + 32 * (size_t)(j << (B - 1u - sl)));
            lds_store(lds, tile, i0, a0 + a1);
            lds_store(lds, tile, i0 + st, (a0 - a1) * t1);
            lds_store(lds, tile, i0 + 2u * st, a2 + a3);
            lds_store(lds, tile, i0 + 3u * st, (a2 - a3) * t1);
          } else {
            lds_store(lds, tile, i0, a0 + a1);
            lds_store(lds, tile, i0 + st, a0 - a1);
            lds_store(lds, tile, i0 + 2u * st, a2 + a3);
            lds_store(lds, tile, i0 + 3u * st, a2 - a3);
          }
        } else {
          if (sl) {
            const Fr t1 = load_field<Fr>(stw + 32 * (size_t)(j << (B - 1u - sl)));
            x1 = x1 * t1;
            x3 = x3 * t1;
          }
          Fr a0 = x0 + x1, a1 = x0 - x1, a2 = x2 + x3, a3 = x2 - x3;
          if (sl) a2 = a2 * load_field<Fr>(stw + 32 * (size_t)(j << (B - 2u - sl)));
          a3 = a3 * load_field<Fr>(stw + 32 * (size_t)((j + h) << (B - 2u - sl)));
          lds_store(lds, tile, i0, a0 + a2);
          lds_store(lds, tile, i0 + st, a1 + a3);
          lds_store(lds, tile, i0 + 2u * st, a0 - a2);
          lds_store(lds, tile, i0 + 3u * st, a1 - a3);
        }
      }
      it += 2u;
    } else {
      const uint32_t sl = DIF ? (B - 1u - it) : it;
      const uint32_t half = 1u << sl;
      for (uint32_t b = tid; b < (tile >> 1); b += nthr) {
        uint32_t c = b & (T - 1u), mb = b >> logT;
        uint32_t j = mb & (half - 1u);
        uint32_t m0 = ((mb >> sl) << (sl + 1u)) | j;
        uint32_t i0 = (m0 << logT) + c, i1 = i0 + (half << logT);
        Fr u = lds_load(lds, tile, i0), v = lds_load(lds, tile, i1);
        if (sl == 0u) {  // tile-local stage 0: every twiddle is W^0 = 1, no multiplication (uniform branch)
          lds_store(lds, tile, i0, u + v);
          lds_store(lds, tile, i1, u - v);
        } else {
          Fr tw = load_field<Fr>(stw + 32 * (size_t)(j << (B - 1u - sl)));
          if (DIF) {
            lds_store(lds, tile, i0, u + v);
            lds_store(lds, tile, i1, (u - v) * tw);
          } else {
            v = v * tw;
            lds_store(lds, tile, i0, u + v);
            lds_store(lds, tile, i1, u - v);
          }
        }
      }
      it += 1u;
    }
    __syncthreads();
  }

  for (uint32_t e = tid; e < tile; e += nthr) {
    uint32_t c = e & (T - 1u), m = e >> logT;
    uint64_t p = base + ((uint64_t)m << s_lo) + c;
    Fr v = lds_load(lds, tile, e);
    if (DIF && s_lo > 0) v = times_boundary_twiddle(v, tw_direct, tw_hi, tw_lo, L, s_lo, B, shift, m, cg * T + c);
    if (MODE == kPassBitrevOut) {
      // the images of different tiles interleave: with more than one tile, dst must not be the buffer being read
      v = v * post;
      store_field(d + 32 * (size_t)(__brev((uint32_t)p) >> (32u - k)), v);
    } else {
      store_field(d + 32 * p, v);
    }
  }
}

// ---- H-scalar chain split over G ranks (NTT row) -----------------------------------------
// n = G * M. Rank g holds X[g + G t] (cyclic rows), runs a size-M DIF with root w^-G (slot p = bitrev(k1)),
// and the ranks exchange so that rank h owns slots [h*Q, (h+1)*Q), Q = M / G, of every rank's transform.
// This kernel is everything between the two exchanges, per slot p (k1 = bitrev_M(p)):
//   v[g]  = in[g][p] * w^-(g k1)                       four-step twiddle of the inverse transform
//   a[k2] = sum_g v[g] * (w^-M)^(g k2)                 size-G DFT: coefficient k = k1 + M k2 (unscaled)
//   a[k2] *= inc^k / n                                  batchApplyKey(1, inc) and the 1/n of the ifft
//   b[i2] = sum_k2 a[k2] * (w^M)^(k2 i2)               size-G DFT of the forward transform
//   out[i2][p] = b[i2] * w^(k1 i2)                      its four-step twiddle
// after the second exchange rank i2 holds slot-ordered input of a size-M DIT whose output t is the
// evaluation at odd-coset index t*G + i2. G <= 8, so the two size-G DFTs are direct sums.
struct SplitRoots {
  Fr inv[8];   // (w^-M)^e, e < G
  Fr fwd[8];   // (w^M)^e
};

// in / out: rank g's (resp. i2's) Q slots start at element g * rank_stride (exchange buffers are laid out
// [rank][polynomial][Q], so rank_stride = 3 Q and the caller offsets the pointers by polynomial * Q).
template <uint32_t G>
static __global__ __launch_bounds__(256) void ntt_split_mid_kernel(const void* __restrict__ in, void* __restrict__ out,
                                                                   uint32_t Q, uint32_t rank_stride, uint32_t slot0,
                                                                   uint32_t logM,
                                                                   SplitRoots roots, const void* __restrict__ inv_hi,
                                                                   const void* __restrict__ inv_lo,
                                                                   const void* __restrict__ fwd_hi,
                                                                   const void* __restrict__ fwd_lo, uint32_t L,
                                                                   const void* __restrict__ cos_hi,
                                                                   const void* __restrict__ cos_lo, uint32_t Lc) {
  uint32_t pl = blockIdx.x * 256u + threadIdx.x;
  if (pl >= Q) return;
  const uint32_t p = slot0 + pl;
  const uint32_t k1 = logM ? (__brev(p) >> (32u - logM)) : 0u;
  const char* src = reinterpret_cast<const char*>(in);
  char* dst = reinterpret_cast<char*>(out);
  Fr v[G], a[G];
#pragma unroll
  for (uint32_t g = 0; g < G; g++) v[g] = load_field<Fr>(src + 32 * ((size_t)g * rank_stride + pl));
  {
    Fr t = tw_lookup(inv_hi, inv_lo, L, k1), pw = t;
#pragma unroll
    for (uint32_t g = 1; g < G; g++) {
      v[g] = v[g] * pw;
      if (g + 1 < G) pw = pw * t;
    }
  }
#pragma unroll
  for (uint32_t k2 = 0; k2 < G; k2++) {
    Fr acc = v[0];
#pragma unroll
    for (uint32_t g = 1; g < G; g++) acc = acc + v[g] * roots.inv[(g * k2) & (G - 1u)];
    a[k2] = acc * tw_lookup(cos_hi, cos_lo, Lc, k1 + (k2 << logM));
  }
  Fr t = tw_lookup(fwd_hi, fwd_lo, L, k1), pw = Fr::one();
#pragma unroll
  for (uint32_t i2 = 0; i2 < G; i2++) {
    Fr acc = a[0];
#pragma unroll
    for (uint32_t k2 = 1; k2 < G; k2++) acc = acc + a[k2] * roots.fwd[(k2 * i2) & (G - 1u)];
    if (i2) acc = acc * pw;
    store_field(dst + 32 * ((size_t)i2 * rank_stride + pl), acc);
    pw = pw * t;
  }
}

// ---- host side ---------------------------------------------------------------------------------
// One pass, complete: its stages, its tile and its launch geometry.
struct NttPass {
  uint32_t s_lo, B, logT;   // stages [s_lo, s_lo + B); tile = 2^B rows x 2^logT columns
  uint32_t grid;            // grid.x = n / tile
  uint32_t threads;         // a quarter of the tile (one radix-4 group per thread and stage pair), 64 .. kNttThreads
  uint32_t lds_bytes;       // 32 B per tile element
  bool direct;              // its boundary twiddles fit one table: s_lo > 0 && s_lo + B <= kNttDirectMaxLog
};

// Tile size of a transform: 2048 elements (64 KiB: two workgroups of 512 threads per CU) up to 2^22, where it makes
// the transform two passes; above that 1024 elements (32 KiB: FOUR workgroups of 256 threads per CU). The pass count
// is the same there (2^26 = 10 + 8 + 8 stages instead of 11 + 8 + 7), and a workgroup's load -> butterflies -> store
// phases do not overlap with each other, only with the other workgroups of the CU: four of them out of step keep the
// multipliers busy while one loads or stores.
constexpr uint32_t ntt_tile_log_by_size(uint32_t k) { return k >= 23 ? 10u : 11u; }
// ZKPOA_NTT_TILE=10|11 forces either (measurement, and the tests' way to the large-size plan at a small k)
inline uint32_t ntt_tile_log(uint32_t k) {
  const long forced = opt_long(O_NTT_TILE);
  return forced ? (uint32_t)forced : ntt_tile_log_by_size(k);
}

// The passes of a size-2^k transform on tiles of 2^tile_log elements, in DIT order (stage 0 upwards; DIF runs them in
// reverse). A function of its two arguments alone.
inline std::vector<NttPass> ntt_plan(uint32_t k, uint32_t tile_log) {
  std::vector<NttPass> v;
  auto add = [&](uint32_t s_lo, uint32_t B, uint32_t logT) {
    const uint32_t t = B + logT;
    v.push_back({s_lo, B, logT, 1u << (k - t), t >= 8 ? (t >= 11 ? kNttThreads : 1u << (t - 2)) : 64u, 32u << t,
                 s_lo > 0 && s_lo + B <= kNttDirectMaxLog});
  };
  if (k == 0) return v;
  const uint32_t b0 = k < tile_log ? k : tile_log, rest = k - b0;
  add(0, b0, 0);
  if (rest && rest < tile_log) {
    // one strided pass of `rest` stages: tile = 2^rest rows x 2^(tile_log - rest) columns (>= 64-B row segments).
    // Fewer columns coalesce less well, but a whole pass (64 B/element of traffic + one boundary twiddle,
    // 2 modmuls/element) disappears; these sizes (n <= 2^21) also sit in the Infinity Cache.
    add(b0, rest, tile_log - rest);
  } else if (rest) {
    const uint32_t npass = (rest + kNttStridedB - 1) / kNttStridedB;
    for (uint32_t i = 0, s = b0; i < npass; i++) {
      const uint32_t b = rest / npass + (i < rest % npass ? 1 : 0);
      // always a full tile: fewer rows = more columns (r02 kept 8 columns, so a 5- or 6-stage pass ran on 256- or
      // 512-element tiles with most of the workgroup idle: 2^22 and 2^24 were off the curve)
      add(s, b, tile_log - b);
      s += b;
    }
  }
  return v;
}

inline HFr hfr_root_of_unity(uint32_t k) {  // w[k], Montgomery
  // w[28] = 5^((r-1)/2^28)
  static const uint64_t e28[4] = {0x9b9709143e1f593full, 0x181585d2833e8487ull, 0x131a029b85045b68ull,
                                  0x000000030644e72eull};
  HFr w = HFr::from_u64(5).pow(e28);
  for (uint32_t i = 28; i > k; i--) w = w.sqr();
  return w;
}

inline HFr hfr_pow2(HFr x, uint32_t times) {  // x^(2^times)
  for (uint32_t i = 0; i < times; i++) x = x.sqr();
  return x;
}

// the shift between the inverse and the forward transform of the prover's chain: coefficient j times inc^j / n,
// inc = w[k + 1] (the odd coset of the domain of twice the size; Fr has no w[29], so 2^28 shifts by the generator's 25)
struct NttCosetShift {
  HFr inc, ninv;
};
inline NttCosetShift ntt_coset_shift(uint32_t k) {
  return {k == 28 ? HFr::from_u64(25) : hfr_root_of_unity(k + 1), HFr::from_u64(1ull << k).inv()};
}

inline Fr to_dev(const HFr& h) {
  Fr f;
  memcpy(&f, &h, 32);
  return f;
}

inline void build_pow_table(hipStream_t st, const HFr& base, const HFr& scale, uint32_t count, void* out) {
  hipLaunchKernelGGL(fr_pow_table_kernel, dim3((count + 255) / 256), dim3(256), 0, st, to_dev(base), to_dev(scale),
                     count, out);
}

// Everything a transform of 2^k elements needs, built whole on the first use of that k: the plan and the device tables
// its passes read. `mem` owns the tables, so a build that fails midway gives back what it had allocated.
struct NttSize {
  struct Twiddles {                       // of one direction: W = w[k] or its inverse
    const void *hi, *lo;                  // W^(i * 2^L), i < 2^(k-L);  W^i, i < 2^L
    std::vector<const void*> small;       // per pass: W_{2^B}^t, t < 2^(B-1) (passes of equal B share one)
    std::vector<const void*> direct;      // per pass: its boundary twiddles as one table, nullptr where it has none
  };
  uint32_t k, L;                          // L = (k + 1) / 2: the split of every two-level table of this size
  std::vector<NttPass> plan;
  Twiddles tw[2];                         // [inverse]
  const void *cos_hi, *cos_lo;            // inc^j / n, two-level like hi / lo
  Fr ninv;                                // 1/n
  std::deque<DevBuf> mem;

  void* table(size_t count) { return mem.emplace_back(count * 32).p; }

  NttSize(hipStream_t st, uint32_t k_) : k(k_), L((k_ + 1) / 2), plan(ntt_plan(k_, ntt_tile_log(k_))) {
    const uint32_t nlo = 1u << L, nhi = 1u << (k - L);
    for (int inverse = 0; inverse < 2; inverse++) {
      Twiddles& t = tw[inverse];
      const HFr w = inverse ? hfr_root_of_unity(k).inv() : hfr_root_of_unity(k);
      void *hi = table(nhi), *lo = table(nlo);
      build_pow_table(st, hfr_pow2(w, L), HFr::one(), nhi, hi);
      build_pow_table(st, w, HFr::one(), nlo, lo);
      t.hi = hi;
      t.lo = lo;
      for (size_t i = 0; i < plan.size(); i++) {
        const NttPass& ps = plan[i];
        size_t same = 0;
        while (plan[same].B != ps.B) same++;
        if (same < i) {
          t.small.push_back(t.small[same]);
        } else {
          void* p = table(1u << (ps.B - 1));
          build_pow_table(st, hfr_pow2(w, k - ps.B), HFr::one(), 1u << (ps.B - 1), p);  // W_{2^B} = W^(2^(k-B))
          t.small.push_back(p);
        }
        void* d = nullptr;
        if (ps.direct) {
          const uint32_t cnt = 1u << (ps.s_lo + ps.B);
          d = table(cnt);
          hipLaunchKernelGGL(ntt_direct_table_kernel, dim3((cnt + 255) / 256), dim3(256), 0, st, d, ps.s_lo, ps.B,
                             k - (ps.s_lo + ps.B), t.hi, t.lo, L);
        }
        t.direct.push_back(d);
      }
    }
    const NttCosetShift sh = ntt_coset_shift(k);
    void *hi = table(nhi), *lo = table(nlo);
    build_pow_table(st, hfr_pow2(sh.inc, L), HFr::one(), nhi, hi);
    build_pow_table(st, sh.inc, sh.ninv, nlo, lo);
    cos_hi = hi;
    cos_lo = lo;
    ninv = to_dev(sh.ninv);
  }
};

// What a transform does besides the butterflies, each folded into the pass over stages [0, B):
//   kNttDif      natural -> bit-reversed (Gentleman-Sande passes from the top stage down)
//   kNttDit      bit-reversed -> natural (Cooley-Tukey passes from stage 0 up)
//   kNttNatural  Fr.fft / Fr.ifft: natural order in and out. DIF passes, the last one kPassBitrevOut (times 1/n in the
//                inverse); multi-pass sizes go d -> scratch ... -> d. One vector at a time.
//   kNttCoset    DIT passes, the first one kPassPreScale with the size's coset table
enum NttForm { kNttDif, kNttDit, kNttNatural, kNttCoset };

struct NttEngine {
  std::unique_ptr<NttSize> sizes[29];
  // scratch of the natural form, n elements (grow-only: smaller sizes reuse it)
  std::unique_ptr<DevBuf> nat_tmp;
  size_t nat_tmp_bytes = 0;

  const NttSize& size(hipStream_t st, uint32_t k) {
    if (k > 28) throw HipError("ntt: log_n > 28 (two-adicity of Fr)");
    if (!sizes[k]) sizes[k] = std::make_unique<NttSize>(st, k);
    return *sizes[k];
  }

  template <bool DIF, int MODE>
  static void launch(hipStream_t st, const NttSize& sz, bool inverse, size_t i, const void* src, void* dst, uint32_t batch,
                     size_t batch_stride, const Fr& post) {
    const NttPass& ps = sz.plan[i];
    const NttSize::Twiddles& t = sz.tw[inverse];
    hipLaunchKernelGGL((ntt_pass_kernel<DIF, MODE>), dim3(ps.grid, batch), dim3(ps.threads), ps.lds_bytes, st, src, dst,
                       batch_stride, sz.k, ps.s_lo, ps.B, ps.logT, t.small[i], t.hi, t.lo, sz.L, t.direct[i], sz.cos_hi,
                       sz.cos_lo, sz.L, post);
  }

  // `batch` vectors of 2^k elements, batch_stride bytes apart, go through every pass together (grid.y = batch)
  void run(hipStream_t st, const NttSize& sz, NttForm form, bool inverse, void* d, uint32_t batch = 1,
           size_t batch_stride = 0) {
    const size_t np = sz.plan.size();
    if (np == 0 || batch == 0) return;
    const bool natural = form == kNttNatural, dif = natural || form == kNttDif;
    if (natural && batch != 1) throw HipError("ntt: the natural-order form takes one vector at a time");
    const size_t bytes = (size_t)32 << sz.k;
    if (natural && np > 1 && nat_tmp_bytes < bytes) {
      ZK_HIP(hipStreamSynchronize(st));
      nat_tmp_bytes = 0;
      nat_tmp.reset();
      nat_tmp = std::make_unique<DevBuf>(bytes);
      nat_tmp_bytes = bytes;
    }
    const Fr post = natural && inverse ? sz.ninv : to_dev(HFr::one());
    for (size_t idx = 0; idx < np; idx++) {
      const size_t i = dif ? np - 1 - idx : idx;
      const void* src = d;
      void* dst = d;
      if (natural && np > 1) {   // d -> tmp, tmp -> tmp ..., tmp -> d (bit-reversed positions)
        src = idx == 0 ? d : nat_tmp->p;
        dst = idx + 1 == np ? d : nat_tmp->p;
      }
      const bool folded = i == 0 && (natural || form == kNttCoset);
      if (folded && natural) launch<true, kPassBitrevOut>(st, sz, inverse, i, src, dst, batch, batch_stride, post);
      else if (folded) launch<false, kPassPreScale>(st, sz, inverse, i, src, dst, batch, batch_stride, post);
      else if (dif) launch<true, kPassPlain>(st, sz, inverse, i, src, dst, batch, batch_stride, post);
      else launch<false, kPassPlain>(st, sz, inverse, i, src, dst, batch, batch_stride, post);
    }
  }

  // evaluations on the domain -> evaluations on the odd coset (ifft, batchApplyKey(1, inc), fft): the coset shift
  // inc^j / n is applied by the forward transform's first pass as it loads (no separate scaling pass)
  void to_odd_coset(hipStream_t st, void* d, uint32_t k, uint32_t batch = 1, size_t stride = 0) {
    const NttSize& sz = size(st, k);
    run(st, sz, kNttDif, true, d, batch, stride);
    run(st, sz, kNttCoset, false, d, batch, stride);
  }

  // the part of to_odd_coset between the two exchanges when the transform is split over G ranks
  // (ntt_split_mid_kernel); k = log2 n of the whole domain, h = this rank, in/out: G blocks of M / G elements,
  // `rank_stride` elements apart.
  void split_mid(hipStream_t st, const void* in, void* out, uint32_t k, uint32_t G, uint32_t h, uint32_t rank_stride) {
    uint32_t lg = 0;
    while ((1u << lg) < G) lg++;
    const uint32_t logM = k - lg, Q = (1u << logM) / G;
    const NttSize& sz = size(st, k);
    SplitRoots roots;
    HFr wf = hfr_pow2(hfr_root_of_unity(k), logM), wi = wf.inv(), af = HFr::one(), ai = HFr::one();
    for (uint32_t e = 0; e < 8; e++) {
      roots.fwd[e] = to_dev(af);
      roots.inv[e] = to_dev(ai);
      af = af * wf;
      ai = ai * wi;
    }
    dim3 grid((Q + 255) / 256), block(256);
#define ZK_SPLIT_MID(GG)                                                                                           \
  hipLaunchKernelGGL((ntt_split_mid_kernel<GG>), grid, block, 0, st, in, out, Q, rank_stride, h * Q, logM, roots,  \
                     sz.tw[1].hi, sz.tw[1].lo, sz.tw[0].hi, sz.tw[0].lo, sz.L, sz.cos_hi, sz.cos_lo, sz.L)
    if (G == 2) ZK_SPLIT_MID(2);
    else if (G == 4) ZK_SPLIT_MID(4);
    else ZK_SPLIT_MID(8);
#undef ZK_SPLIT_MID
  }
};

}  // namespace zkpoa
