// Every host-side decision about one MSM, as a pure function of its request: window width, piece length, bucket
// matrix, entry form. Plain C++ (no HIP): msm.hip.h runs the plan, tests/test_msm_plan.py pins it without a GPU
// (zkpoa_test_msm_plan against tests/golden/gen/msm_plan.json).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zkpoa {

constexpr uint32_t kMaxPieceLenPlan = 512;   // = kMaxPieceLen of the piece-ordering kernels
constexpr int kDensityLo = 4, kDensityHi = 25;

// What a plan is made from -- all of it: there is no ambient input. Whoever builds the request resolves each field once.
struct MsmRequest {
  uint64_t n = 0;        // points sorted at once (a chunk of a chunked MSM)
  int c = 0;             // window width: the fixed-base table's (merged), else the forced one (option "msm_c"), else 0 =
                         // the cost model below; a value outside 4..22 (merged: 4..25) is ignored
  bool merged = false;   // fixed-base form (MsmTable, msm.hip.h): all windows in one bucket set
  bool for_g2 = false;   // the sort (also) feeds a G2 accumulation: shorter pieces
  // density[c] = expected non-zero digits per scalar at window width c, kDensityLo <= c <= kDensityHi (32 doubles
  // indexed by c), measured on a witness (msm_density_kernel); nullptr = uniform scalars (every digit non-zero). Real
  // witnesses are mostly bits and short limbs, so a witness MSM has a fraction of the n * W entries of a uniform one
  // -- and a window sized for n * W entries then pays for millions of near-empty buckets (2^26 shape: the A query took
  // 34 ms for 10 ms of additions). Only read while the plan is made; the array outlives every plan that records it
  // (it belongs to the key handle).
  const double* density = nullptr;
  int k0 = 0;            // level-0 piece length (option "msm_k0", experiments): 8..kMaxPieceLenPlan, else the rule below
};

struct MsmPlan {
  MsmRequest req;   // what this plan was made from
  uint32_t n = 0;   // points
  uint32_t c = 0;   // window bits
  uint32_t W = 0;   // digit windows per scalar
  uint32_t Nb = 0;  // buckets per bucket set = 2^(c-1)
  // Fixed-base form (MsmTable, msm.hip.h): the bases 2^(c*j) * P_i of every window j are precomputed, so the digits of
  // ALL windows fall into ONE bucket set: Wb = 1 and the (point, window) entry w * n + i is itself the index into
  // the table. Classic form: one bucket set per window, Wb = W.
  bool merged = false;
  uint32_t Wb = 0;  // bucket sets
  uint32_t ne = 0;  // entries per bucket set: n (classic) or n * W (merged)
  uint32_t TB = 0;  // total buckets = Wb * Nb
  uint32_t K0 = 0;  // level-0 piece length
  uint32_t K = 4;   // fan-in per thread for levels >= 1: hot buckets (witness bits) are latency-bound chains of full
                    // additions, so a small fan-in with more levels beats 64 sequential additions per thread
  // bucket reduction: the Nb buckets of a window form a rows x S matrix, b = hi * S + lo
  uint32_t logS = 0, logRows = 0;
  // sparse scalars in the fixed-base form (a witness through its tables): the sort takes a compact entry list instead
  // of the dense digit array (msm_sort.hip.h msm_entries_kernel)
  bool sparse = false;
};

inline uint32_t msm_windows(uint32_t c) { return (254 + c - 1) / c; }

// Window width. Costs in units of one mixed addition: every (point, window) entry is one; a bucket costs ~3 in the
// reduction (a row and a column full addition at 1.4 each + tree levels); one counting-sort pass moves ~20 B per
// entry at ~3 TB/s, i.e. ~0.03 of an addition per entry and pass (measured per-kernel times at 2^20, r02).
inline MsmPlan msm_make_plan(const MsmRequest& r) {
  MsmPlan p;
  p.req = r;
  p.n = (uint32_t)r.n;
  p.merged = r.merged;
  const size_t n = (size_t)r.n;
  const bool merged = r.merged;
  int best_c = 4;
  double best = 1e300;
  const double* density = r.density;   // merged form: the width is the table's (r.c) at run time, but a table for
                                       // witness scalars is SIZED with the density of a witness
  for (int c = 4; c <= (merged ? 25 : 22); c++) {
    double W = (double)msm_windows((uint32_t)c);
    double sets = merged ? 1.0 : W;
    double passes = (double)((c - 1 + 7) / 8);
    // entries that exist; the dense n x W digit matrix is still written once and read twice (0.04 of an addition
    // per slot), and every bucket costs a slot in the piece list besides its two additions in the reduction
    double entries = density ? density[c] * (double)n : W * (double)n;
    double cost = entries * (1.0 + 0.03 * passes) + (density ? 0.04 * W * (double)n : 0.0) +
                  (density ? 5.0 : 3.0) * sets * (double)(1u << (c - 1));
    if (cost < best) {
      best = cost;
      best_c = c;
    }
  }
  if (r.c >= 4 && r.c <= (merged ? 25 : 22)) best_c = r.c;
  p.c = best_c;
  p.W = msm_windows(p.c);
  p.Nb = 1u << (p.c - 1);
  p.Wb = merged ? 1u : p.W;
  p.ne = merged ? p.n * p.W : p.n;
  p.TB = p.Wb * p.Nb;
  p.logS = (uint32_t)(p.c - 1 + 1) / 2;
  p.logRows = (uint32_t)(p.c - 1) - p.logS;
  // Level-0 piece length. One thread adds one piece sequentially: about twice the mean bucket occupancy, so
  // most buckets are a single piece (uniform scalars: 128 at 2^20, 256 at 2^26). The kernel cannot end before
  // K0 dependent mixed additions have run, and a G2 addition is ~15 us for a lone wave (256 of them: 4 ms), so
  // a sort whose result also feeds a G2 accumulation (the prover's B query) uses a quarter of that; buckets
  // longer than K0 continue in the partial-sum levels.
  const double dens_entries = density ? density[p.c] * (double)p.n : (double)p.n * p.W;
  double avg = (merged ? dens_entries : dens_entries / p.W) / (double)p.Nb;
  uint32_t k0 = 32;
  while (k0 < 2 * avg && k0 < 256) k0 <<= 1;
  if (r.for_g2 && k0 > 32) k0 = k0 >= 128 ? k0 / 4 : 32;
  // ... and short enough that the pieces fill the chip about 2.5 times over (256 CUs x 12 waves x 64 lanes at the
  // accumulation kernel's 3 waves per SIMD; 2 for G2): with fewer, longer pieces the grid is one partial wave of
  // work and the CUs idle behind its longest pieces (2^20 points: 128-long pieces ran at 0.84 of the ALU ceiling,
  // 32-long ones at 0.95-1.0; the extra partial sums cost ~3 % more additions).
  const double fill = dens_entries / (2.5 * 256.0 * (r.for_g2 ? 8.0 : 12.0) * 64.0);
  while (k0 > 32 && (double)k0 > fill) k0 >>= 1;
  if (r.k0 >= 8 && r.k0 <= (int)kMaxPieceLenPlan) k0 = (uint32_t)r.k0;
  p.K0 = k0;
  p.sparse = merged && p.n && density && density[p.c] < 0.6 * (double)p.W;
  return p;
}

}  // namespace zkpoa
