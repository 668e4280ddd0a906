// Phase-2 setup arithmetic on the device (first half): the point sections of a fresh proving key.
//
// `snarkjs zkey new circuit.r1cs pot.ptau circuit_0000.zkey` (scripts/g16_setup.sh:243-246; "34 h" for the layer-three
// circuit, README.md:179) is, for every signal s, a sum over the R1CS coefficients that mention it:
//   A[s]  = sum_{(c, k) in A column s}  k * L_c(tau) G1                              (zkey section 5)
//   B1[s], B2[s]: the same over the B matrix, in G1 and in G2                        (sections 6, 7)
//   IC / C[s] = sum_A k * beta L_c(tau) G1 + sum_B k * alpha L_c(tau) G1 + sum_C k * L_c(tau) G1   (sections 3, 8)
// with L_c(tau) G the powers-of-tau points in Lagrange form (the prepared .ptau's sections 12-15). snarkjs is not
// vendored in the reference (package.json dependency); this restates the published algorithm (snarkjs zkey_new.js).
// Each sum is a transposed sparse-matrix x point-vector product: the coefficients are mostly 1, -1 and small
// constants, the columns short except for a few signals (the constant 1) that occur in a large part of the rows.
//
// Device mapping (one call per section; zkpoa_setup_accumulate):
//   1. histogram of the entries by signal (atomics), exclusive scan -> segment offsets, scatter of the entry ids;
//   2. one lane per entry: k * P by MSB-first double-and-add on the sign-normalised coefficient (k > r/2 ->
//      (r - k) * (-P): "-1" is one addition, not 254 doublings), XYZZ result into the entry's slot in segment order;
//      lanes take the entries sorted by coefficient length, so a wave's lanes run equally long;
//   3. the MSM's partial-sum levels (msm_accumN_kernel, fan-in 4: a hot segment is a chain of full additions, so
//      depth matters) until every segment is one point; 4. XYZZ -> affine, zkey wire format.
// The order inside a segment depends on the atomics; the sum does not, and the affine output is canonical.
#include "abc.hip.h"
#include "msm.hip.h"
#include "hooks.hip.h"
#include "pairing.hpp"
#include "phase2_dev.hip.h"
#include "setup_common.hip.h"
#include "zkpoa_internal.hpp"

using namespace zkpoa;

namespace {

// counts[sig[e]]++; flags |= 1 for an out-of-range index, |= 2 for a coefficient >= r
static __global__ __launch_bounds__(256) void setup_hist_kernel(const uint32_t* __restrict__ sig,
                                                                const uint32_t* __restrict__ pidx,
                                                                const void* __restrict__ coefs, uint32_t nnz,
                                                                uint32_t n_signals, uint32_t n_points,
                                                                uint32_t* __restrict__ counts, uint32_t* __restrict__ flags) {
  uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= nnz) return;
  uint32_t s = sig[e];
  uint32_t k[8];
  load_scalar(coefs, e, k);
  uint32_t bw = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) (void)subb(k[i], FrParams::P[i], bw);
  if (s >= n_signals || pidx[e] >= n_points) {
    atomicOr(flags, 1u);
    return;
  }
  if (!bw) atomicOr(flags, 2u);
  atomicAdd(&counts[s], 1u);
}

static __global__ __launch_bounds__(256) void setup_scatter_kernel(const uint32_t* __restrict__ sig, uint32_t nnz,
                                                                   const uint32_t* __restrict__ off,
                                                                   uint32_t* __restrict__ cursor,
                                                                   uint32_t* __restrict__ order) {
  uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= nnz) return;
  uint32_t s = sig[e];
  order[off[s] + atomicAdd(&cursor[s], 1u)] = e;
}

// bit length (0..254) of the sign-normalised coefficient of entry e: the length of its double-and-add
ZK_DEV uint32_t setup_bitlen(const void* __restrict__ coefs, uint32_t e) {
  uint32_t k[8];
  load_scalar(coefs, e, k);
  (void)scalar_normalize(k);
  uint32_t len = 0;
#pragma unroll
  for (int i = 7; i >= 0; i--)
    if (len == 0 && k[i]) len = 32u * i + (32u - __builtin_clz(k[i]));
  return len;
}
// counting sort of the slots by that length, longest first (256 keys): a wave runs as long as its longest
// coefficient, and an R1CS mixes 1 and -1 (one addition) with full-width constants (254 doublings)
static __global__ __launch_bounds__(256) void setup_len_hist_kernel(const void* __restrict__ coefs,
                                                                    const uint32_t* __restrict__ order, uint32_t nnz,
                                                                    uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j < nnz) atomicAdd(&h[255u - setup_bitlen(coefs, order[j])], 1u);
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}
static __global__ __launch_bounds__(256) void setup_len_scatter_kernel(const void* __restrict__ coefs,
                                                                       const uint32_t* __restrict__ order, uint32_t nnz,
                                                                       const uint32_t* __restrict__ start,
                                                                       uint32_t* __restrict__ cursor,
                                                                       uint32_t* __restrict__ by_len) {
  // most entries share one key (|coefficient| = 1): ranks inside the workgroup through LDS, ONE global atomic per
  // (workgroup, key) -- a global atomic per entry on that one cursor took 37 ms for 4 M entries
  __shared__ uint32_t h[256], base[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  uint32_t key = 0, rank = 0;
  if (j < nnz) {
    key = 255u - setup_bitlen(coefs, order[j]);
    rank = atomicAdd(&h[key], 1u);
  }
  __syncthreads();
  if (h[threadIdx.x]) base[threadIdx.x] = start[threadIdx.x] + atomicAdd(&cursor[threadIdx.x], h[threadIdx.x]);
  __syncthreads();
  if (j < nnz) by_len[base[key] + rank] = j;
}

// thread t takes slot j = by_len[t] (segment order): Q = coef * P; a segment of one entry goes straight to its bucket
template <class F>
static __global__ __launch_bounds__(256) void setup_mul_kernel(const void* __restrict__ points,
                                                               const void* __restrict__ coefs,
                                                               const uint32_t* __restrict__ pidx,
                                                               const uint32_t* __restrict__ sig,
                                                               const uint32_t* __restrict__ order,
                                                               const uint32_t* __restrict__ by_len,
                                                               const uint32_t* __restrict__ off, uint32_t nnz,
                                                               void* __restrict__ buckets, void* __restrict__ items) {
  uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= nnz) return;
  const uint32_t j = by_len[t];
  const uint32_t e = order[j], s = sig[e];
  uint32_t k[8];
  load_scalar(coefs, e, k);
  const bool neg = scalar_normalize(k);
  const Affine<F> p = load_affine<F>(points, pidx[e]);
  int top = -1;
#pragma unroll
  for (int i = 7; i >= 0; i--)
    if (top < 0 && k[i]) top = 32 * i + (31 - __builtin_clz(k[i]));
  XYZZ<F> acc = XYZZ<F>::inf();
  for (int bit = top; bit >= 0; bit--) {   // one doubling site, one addition site
    acc = xyzz_dbl(acc);
    if ((k[bit >> 5] >> (bit & 31)) & 1u) xyzz_add_affine(acc, p, neg);
  }
  if (off[s + 1] - off[s] == 1u) store_xyzz(buckets, s, acc);
  else store_xyzz(items, j, acc);
}

// out[i] = k * in[i] for one scalar k (sign-normalised by the caller: `neg` adds -P), XYZZ into scratch
struct ScalarArg {
  uint32_t l[8];
};
template <class F>
static __global__ __launch_bounds__(256) void setup_scale_kernel(const void* __restrict__ in, uint64_t i0, uint32_t cnt,
                                                                 ScalarArg k, int top, bool neg,
                                                                 void* __restrict__ out_xyzz) {
  uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= cnt) return;
  const Affine<F> p = load_affine<F>(in, i0 + t);
  XYZZ<F> acc = XYZZ<F>::inf();
  for (int bit = top; bit >= 0; bit--) {   // the scalar is the same in every lane: no divergence
    acc = xyzz_dbl(acc);
    if ((k.l[bit >> 5] >> (bit & 31)) & 1u) xyzz_add_affine(acc, p, neg);
  }
  store_xyzz(out_xyzz, t, acc);
}

// d_out[i] = k * d_in[i], i < n, wire format in and out (k: 32 B little-endian standard form, < r)
template <class F>
void setup_scale(zkpoa_context* ctx, const void* d_in, uint64_t n, const uint8_t k_le[32], void* d_out) {
  if (n == 0) return;
  hipStream_t st = ctx->dev.lanes[0].stream;
  HFr kh = HFr::from_bytes(k_le);
  uint64_t half[4] = {0, 0, 0, 0};   // (r - 1) / 2
  {
    uint64_t c = 0;
    for (int i = 3; i >= 0; i--) {
      half[i] = (HFrParams::P[i] >> 1) | (c << 63);
      c = HFrParams::P[i] & 1;
    }
  }
  bool neg = false;
  for (int i = 3; i >= 0; i--) {
    if (kh.l[i] > half[i]) { neg = true; break; }
    if (kh.l[i] < half[i]) break;
  }
  if (neg) {   // k > r / 2: (r - k) * (-P)
    HFr r_minus = HFr{{HFrParams::P[0], HFrParams::P[1], HFrParams::P[2], HFrParams::P[3]}};
    unsigned __int128 bw = 0;
    for (int i = 0; i < 4; i++) {
      unsigned __int128 d = (unsigned __int128)r_minus.l[i] - kh.l[i] - bw;
      kh.l[i] = (uint64_t)d;
      bw = (d >> 64) & 1;
    }
  }
  ScalarArg ka;
  memcpy(ka.l, kh.l, 32);
  int top = -1;
  for (int i = 7; i >= 0 && top < 0; i--)
    if (ka.l[i]) top = 32 * i + (31 - __builtin_clz(ka.l[i]));
  const uint64_t slab = 1ull << 22;
  DevBuf scratch((size_t)(n < slab ? n : slab) * MsmSizes<F>::kXyzz);
  for (uint64_t off = 0; off < n; off += slab) {
    const uint32_t cnt = (uint32_t)(n - off < slab ? n - off : slab);
    hipLaunchKernelGGL((setup_scale_kernel<F>), dim3((cnt + 255) / 256), dim3(256), 0, st, d_in, off, cnt, ka, top, neg,
                       scratch.p);
    hipLaunchKernelGGL((xyzz_to_affine_kernel<F>), dim3((cnt + 255) / 256), dim3(256), 0, st, (const void*)scratch.p,
                       (void*)(reinterpret_cast<char*>(d_out) + off * MsmSizes<F>::kAffine), (uint64_t)cnt);
  }
  ZK_HIP(hipStreamSynchronize(st));
  ZK_HIP(hipGetLastError());
}

template <class F>
void setup_accumulate(zkpoa_context* ctx, const void* d_points, uint64_t n_points, const void* d_coefs,
                      const uint32_t* d_pidx, const uint32_t* d_sig, uint64_t nnz, uint64_t n_signals, void* d_out) {
  if (n_signals == 0) return;
  if (nnz >= (1ull << 31) || n_signals >= (1ull << 31) || n_points >= (1ull << 32))
    throw HipError("setup_accumulate: more than 2^31 entries or signals in one call");
  Lane& lane = ctx->dev.lanes[0];
  hipStream_t st = lane.stream;
  const uint32_t S = (uint32_t)n_signals, N = (uint32_t)nnz;
  constexpr size_t X = MsmSizes<F>::kXyzz;
  DevBuf counts((size_t)S * 4), off(((size_t)S + 1) * 4), po_b(((size_t)S + 1) * 4), po_c(((size_t)S + 1) * 4),
      block_sums(((size_t)S / kScanTile + 2) * 4), misc(64), order((size_t)(N ? N : 1) * 4), buckets((size_t)S * X),
      items((size_t)(N ? N : 1) * X), items2(((size_t)N / 2 + 2) * X), by_len((size_t)(N ? N : 1) * 4), len_hist(1024 * 4);
  uint32_t* m = reinterpret_cast<uint32_t*>(misc.p);   // [0] flags, [1] total, [2] max segment, [3] level total
  ZK_HIP(hipMemsetAsync(counts.p, 0, (size_t)S * 4, st));
  ZK_HIP(hipMemsetAsync(misc.p, 0, 64, st));
  ZK_HIP(hipMemsetAsync(buckets.p, 0, (size_t)S * X, st));   // the all-zero XYZZ is the point at infinity
  const uint32_t grid = (N + 255) / 256;
  if (N)
    hipLaunchKernelGGL(setup_hist_kernel, dim3(grid), dim3(256), 0, st, d_sig, d_pidx, d_coefs, N, S, (uint32_t)n_points,
                       (uint32_t*)counts.p, m);
  scan_u32(st, (const uint32_t*)counts.p, S, 0, 0, (uint32_t*)off.p, (uint32_t*)block_sums.p, m + 1, m + 2);
  msm_read_back(lane, m, 16);
  const uint32_t* hb = lane.pinned.as<const uint32_t>();
  const uint32_t flags = hb[0], total = hb[1], max_seg = hb[2];
  if (flags & 1u) throw HipError("setup_accumulate: signal or point index out of range");
  if (flags & 2u) throw HipError("setup_accumulate: coefficient is not a field element (>= r)");
  if (total != N) throw HipError("setup_accumulate: internal: histogram does not add up");
  if (N) {
    ZK_HIP(hipMemsetAsync(counts.p, 0, (size_t)S * 4, st));   // reused as the scatter cursors
    hipLaunchKernelGGL(setup_scatter_kernel, dim3(grid), dim3(256), 0, st, d_sig, N, (const uint32_t*)off.p,
                       (uint32_t*)counts.p, (uint32_t*)order.p);
    // slots ordered by the length of their double-and-add (256 keys: histogram, 256-entry scan on one wave, scatter)
    uint32_t* lh = reinterpret_cast<uint32_t*>(len_hist.p);   // [0, 256) counts, [256, 513) starts, [520, 776) cursors
    ZK_HIP(hipMemsetAsync(len_hist.p, 0, 1024 * 4, st));
    hipLaunchKernelGGL(setup_len_hist_kernel, dim3(grid), dim3(256), 0, st, d_coefs, (const uint32_t*)order.p, N, lh);
    scan_u32(st, lh, 256, 0, 0, lh + 256, (uint32_t*)block_sums.p, m + 3, nullptr);
    hipLaunchKernelGGL(setup_len_scatter_kernel, dim3(grid), dim3(256), 0, st, d_coefs, (const uint32_t*)order.p, N,
                       (const uint32_t*)(lh + 256), lh + 520, (uint32_t*)by_len.p);
    hipLaunchKernelGGL((setup_mul_kernel<F>), dim3(grid), dim3(256), 0, st, d_points, d_coefs, d_pidx, d_sig,
                       (const uint32_t*)order.p, (const uint32_t*)by_len.p, (const uint32_t*)off.p, N, buckets.p, items.p);
  }
  const uint32_t K = 4;   // partial-sum levels, shared with the MSM (msm_reduce_levels): fan-in 4 until every segment is one point
  auto scan = [&](const uint32_t* in, uint32_t* out) { scan_u32(st, in, S, 3, K, out, (uint32_t*)block_sums.p, m + 3, nullptr); };
  msm_reduce_levels<F>(st, S, K, (const uint32_t*)off.p, (uint32_t*)po_b.p, (uint32_t*)po_c.p, (char*)items.p, N ? N : 1,
                       (char*)items2.p, (size_t)N / 2 + 2, max_seg, N, buckets.p, scan);
  hipLaunchKernelGGL((xyzz_to_affine_kernel<F>), dim3((S + 255) / 256), dim3(256), 0, st, (const void*)buckets.p, d_out,
                     (uint64_t)S);
  ZK_HIP(hipStreamSynchronize(st));
  ZK_HIP(hipGetLastError());
}

}  // namespace

extern "C" int zkpoa_setup_accumulate(zkpoa_context* ctx, int group, const void* d_points, uint64_t n_points,
                                      const void* d_coefs, const uint32_t* d_point_index, const uint32_t* d_signal,
                                      uint64_t nnz, uint64_t n_signals, void* d_out) {
  ZK_API_BEGIN(ctx)
  if (group != 1 && group != 2) throw HipError("setup_accumulate: group must be 1 (G1) or 2 (G2)");
  if ((nnz && (!d_points || !d_coefs || !d_point_index || !d_signal)) || (n_signals && !d_out))
    throw HipError("setup_accumulate: null pointer");
  if (group == 1) setup_accumulate<Fq>(ctx, d_points, n_points, d_coefs, d_point_index, d_signal, nnz, n_signals, d_out);
  else setup_accumulate<Fq2>(ctx, d_points, n_points, d_coefs, d_point_index, d_signal, nnz, n_signals, d_out);
  ZK_API_END(ctx)
}

// ---- `snarkjs zkey new <circuit.r1cs> <pot.ptau> <circuit_0.zkey>` (g16_setup.sh:243-246) on files -----------------------
namespace {

void dev_check_coords(zkpoa_context* ctx, const void* d, uint64_t count32, const char* what) {
  if (!count32) return;
  hipStream_t st = ctx->dev.lanes[0].stream;
  DevBuf flag(64);
  ZK_HIP(hipMemsetAsync(flag.p, 0, 64, st));
  hipLaunchKernelGGL((range_check_kernel<FqParams>), dim3((uint32_t)((count32 + 255) / 256)), dim3(256), 0, st, d, count32,
                     (uint32_t*)flag.p);
  uint32_t bad = 0;
  ZK_HIP(hipMemcpyAsync(&bad, flag.p, 4, hipMemcpyDeviceToHost, st));
  ZK_HIP(hipStreamSynchronize(st));
  ZK_HIP(hipGetLastError());
  if (bad) throw SetupError(std::string(what) + ": a coordinate is not a field element (>= q)");
}

struct Entries {   // one zkpoa_setup_accumulate call; filled in place by several threads (set)
  UVec<uint8_t> coef;
  UVec<uint32_t> pidx, sig;
  void alloc(uint64_t count) {
    coef.alloc(count * 32);
    pidx.alloc(count);
    sig.alloc(count);
  }
  void set(uint64_t i, const Term& t, uint32_t point_offset) {
    memcpy(&coef[i * 32], t.coef, 32);
    pidx[i] = point_offset + t.c;
    sig[i] = t.s;
  }
  void set_one(uint64_t i, uint32_t point, uint32_t signal) {
    memset(&coef[i * 32], 0, 32);
    coef[i * 32] = 1;
    pidx[i] = point;
    sig[i] = signal;
  }
};

// keep: the device copy of the result outlives the call (the circuit hash reads it there)
template <class F>
UVec<uint8_t> run_accumulate(zkpoa_context* ctx, const DevBuf& points, uint64_t n_points, const Entries& e,
                                    uint64_t n_signals, std::unique_ptr<DevBuf>* keep = nullptr) {
  constexpr size_t A = MsmSizes<F>::kAffine;
  const uint64_t nnz = e.sig.size();
  DevBuf coef(nnz * 32), pidx(nnz * 4), sig(nnz * 4);
  std::unique_ptr<DevBuf> out(new DevBuf(n_signals * A));
  coef.up(e.coef.data(), nnz * 32);
  pidx.up(e.pidx.data(), nnz * 4);
  sig.up(e.sig.data(), nnz * 4);
  setup_accumulate<F>(ctx, points.p, n_points, coef.p, (const uint32_t*)pidx.p, (const uint32_t*)sig.p, nnz, n_signals, out->p);
  UVec<uint8_t> host(n_signals * A);
  if (!host.empty()) ZK_HIP(hipMemcpy(host.data(), out->p, host.size(), hipMemcpyDeviceToHost));
  if (keep) *keep = std::move(out);
  return host;
}

// entries of the three accumulations of `zkey new` (+ the nPublic + 1 rows `1 * signal_i` that bind the public inputs);
// eA / eB may be null (`zkey verify` recomputes the initial IC / C only)
void build_entries(const R1cs& r, uint64_t n, Entries* eA, Entries* eB, Entries& eK) {
  const uint64_t nA = r.A.size(), nB = r.B.size(), nCt = r.C.size(), nPub1 = (uint64_t)r.nPublic + 1;
  if (eA) eA->alloc(nA + nPub1);
  if (eB) eB->alloc(nB);
  eK.alloc(nA + nB + nCt + nPub1);
  parallel_ranges(nA, 1u << 16, [&](unsigned, uint64_t lo, uint64_t hi) {
    for (uint64_t i = lo; i < hi; i++) {
      if (eA) eA->set(i, r.A[i], 0);
      eK.set(i, r.A[i], 0);                                      // K: A over beta*L  (points [0, n))
    }
  });
  parallel_ranges(nB, 1u << 16, [&](unsigned, uint64_t lo, uint64_t hi) {
    for (uint64_t i = lo; i < hi; i++) {
      if (eB) eB->set(i, r.B[i], 0);
      eK.set(nA + i, r.B[i], (uint32_t)n);                       //    B over alpha*L ([n, 2n))
    }
  });
  parallel_ranges(nCt, 1u << 16, [&](unsigned, uint64_t lo, uint64_t hi) {
    for (uint64_t i = lo; i < hi; i++) eK.set(nA + nB + i, r.C[i], (uint32_t)(2 * n));   //    C over L       ([2n, 3n))
  });
  for (uint32_t i = 0; i <= r.nPublic; i++) {
    if (eA) eA->set_one(nA + i, r.nConstraints + i, i);
    eK.set_one(nA + nB + nCt + i, r.nConstraints + i, i);
  }
}

// the initial IC | C of a key (m points: sections 3 and 8 before any contribution) on the device, and on the host
UVec<uint8_t> accumulate_k(zkpoa_context* ctx, const PtauRanges& pt, uint64_t n, const Entries& eK, uint64_t m,
                           std::unique_ptr<DevBuf>* keep) {
  DevBuf dK(3 * n * 64);
  dK.up(pt.bL.data(), n * 64, 0);
  dK.up(pt.aL.data(), n * 64, n * 64);
  dK.up(pt.L1.data(), n * 64, 2 * n * 64);
  dev_check_coords(ctx, dK.p, 4 * n, "ptau alpha*tau*G1 / beta*tau*G1 (Lagrange)");
  return run_accumulate<Fq>(ctx, dK, 3 * n, eK, m, keep);
}

// ---- the circuit hash (DESIGN.md "Phase-2 transcript"): Blake2b-512 over the initial key's points in hash form ----------
struct CsHashPoints {   // device pointers, wire form
  const void *IC, *C, *A, *B1, *B2;
  uint64_t l, m, n;
  const uint8_t *alpha1, *beta1, *beta2;   // host, wire form
};
void circuit_hash(zkpoa_context* ctx, const char* ptau_path, const CsHashPoints& k, PhaseTimer& phase, uint8_t out[64]) {
  namespace p2 = zkpoa::phase2;
  // ptau section 2: tau^i G1, i < 2n - 1 (the powers form; section 9 holds the Lagrange-odd points instead)
  DevBuf dT(2 * k.n * 64), dH(k.n * 64);
  {
    MappedFile fp(ptau_path);
    auto ps = bin_sections(fp, "ptau", 1, "ptau");
    if (!ps.count(2) || ps[2].len < (2 * k.n - 1) * 64)
      throw SetupError("ptau: section 2 (tau^i G1) is missing or too short for the transcript's H points");
    UVec<uint8_t> T((2 * k.n - 1) * 64);
    pread_all(fp.fd, T.data(), T.size(), ps[2].off, "tau^i G1");
    dT.up(T.data(), T.size());
    dev_check_coords(ctx, dT.p, 2 * (2 * k.n - 1), "ptau tau^i G1");
  }
  h_diff(ctx, dT.p, k.n, dH.p);
  phase("H-diff (ptau section 2 read, device)");
  p2::Blake2b h;
  uint8_t g1[64], g2[128];
  h_affine_to_bytes<HFq>(host_generator<HFq>(), g1);
  h_affine_to_bytes<HFq2>(host_generator<HFq2>(), g2);
  p2::hash_g1_wire(h, k.alpha1);
  p2::hash_g1_wire(h, k.beta1);
  p2::hash_g2_wire(h, k.beta2);
  p2::hash_g2_wire(h, g2);   // gamma2, delta1, delta2 of the initial key: the generators
  p2::hash_g1_wire(h, g1);
  p2::hash_g2_wire(h, g2);
  HashStream hs(ctx, h, 0);
  hs.points(k.IC, k.l + 1, 1, true);
  hs.points(dH.p, k.n - 1, 1, true);
  hs.points(k.C, k.m - k.l - 1, 1, true);
  hs.points(k.A, k.m, 1, true);
  hs.points(k.B1, k.m, 1, true);
  hs.points(k.B2, k.m, 2, true);
  h.final(out);
  if (phase.verbose) {
    fprintf(stderr, "zkpoa: %s: %-*s %8.1f ms\n", phase.command, phase.width, "circuit hash: convert (host waits for the device)", hs.convert_ms);
    fprintf(stderr, "zkpoa: %s: %-*s %8.1f ms  (%.3f GB, %.2f GB/s)\n", phase.command, phase.width, "circuit hash: hash (Blake2b, one host thread)",
            hs.hash_ms, hs.bytes / 1e9, hs.hash_ms > 0 ? hs.bytes / 1e6 / hs.hash_ms : 0.0);
  }
  phase("circuit hash");
}

constexpr uint32_t kZkeyIds[10] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10};   // a .zkey's sections, in the order snarkjs numbers them

void put32(std::vector<uint8_t>& v, uint32_t x) { v.insert(v.end(), (uint8_t*)&x, (uint8_t*)&x + 4); }
void put64(std::vector<uint8_t>& v, uint64_t x) { v.insert(v.end(), (uint8_t*)&x, (uint8_t*)&x + 8); }

void zkey_new(zkpoa_context* ctx, const char* r1cs_path, const char* ptau_path, const char* zkey_path, uint32_t flags) {
  const bool transcript = (flags & ZKPOA_SETUP_TRANSCRIPT) != 0;
  PhaseTimer phase("zkey new", 38);
  MappedFile fr(r1cs_path);
  const R1cs r = parse_r1cs(fr);
  phase("r1cs parsed");
  const uint32_t cp = domain_log2(r);
  const uint64_t n = 1ull << cp;

  const PtauRanges pt = read_ptau_ranges(ptau_path, cp);
  const UVec<uint8_t>&L1 = pt.L1, &L2 = pt.L2, &Hs = pt.Hs;
  const uint8_t *alpha1 = pt.alpha1, *beta1 = pt.beta1, *beta2 = pt.beta2;
  phase("ptau ranges read");

  Entries eA, eB, eK;
  build_entries(r, n, &eA, &eB, eK);
  phase("entry lists built");
  const uint64_t m = r.nWires;
  // ---- the file: sections 1-10 in the order snarkjs numbers them. Every length follows from the header and the term
  // counts, so the file is sized now and each section is put at its place when it is ready: the host's own sections
  // (header, coefficients, H) by a side thread WHILE the device computes the others.
  const uint64_t nCoefs = r.A.size() + r.B.size() + r.nPublic + 1;
  if (nCoefs > 0xffffffffull) throw SetupError("more than 2^32 coefficients");
  const uint64_t icb = ((uint64_t)r.nPublic + 1) * 64;
  const uint64_t sec_len[10] = {4, kHdrLen, icb, 4 + nCoefs * 44, m * 64, m * 64, m * 128, (m - r.nPublic - 1) * 64, n * 64, 64 + 4};
  SectionFile out(zkey_path, "zkey", kZkeyIds, sec_len, 10);
  auto put_section = [&](uint32_t id, const void* p, uint64_t len) { out.put(id, p, len); };
  double host_ms = 0;
  SideTask host_sections([&] {
    struct timespec h0, h1;
    clock_gettime(CLOCK_MONOTONIC, &h0);
    const uint32_t one_u32 = 1;   // section 1: protocol id 1 = groth16
    put_section(1, &one_u32, 4);
    std::vector<uint8_t> s2, s10(64 + 4, 0);
    put32(s2, 32);
    s2.insert(s2.end(), (const uint8_t*)HFqParams::P, (const uint8_t*)HFqParams::P + 32);
    put32(s2, 32);
    s2.insert(s2.end(), (const uint8_t*)HFrParams::P, (const uint8_t*)HFrParams::P + 32);
    put32(s2, r.nWires);
    put32(s2, r.nPublic);
    put32(s2, (uint32_t)n);
    uint8_t g1[64], g2[128];
    h_affine_to_bytes<HFq>(host_generator<HFq>(), g1);
    h_affine_to_bytes<HFq2>(host_generator<HFq2>(), g2);
    s2.insert(s2.end(), alpha1, alpha1 + 64);
    s2.insert(s2.end(), beta1, beta1 + 64);
    s2.insert(s2.end(), beta2, beta2 + 128);
    s2.insert(s2.end(), g2, g2 + 128);   // gamma2 = the generator until a contribution changes delta
    s2.insert(s2.end(), g1, g1 + 64);    // delta1
    s2.insert(s2.end(), g2, g2 + 128);   // delta2
    put_section(2, s2.data(), s2.size());
    if (!transcript) put_section(10, s10.data(), s10.size());
    // coefficients: A and B terms per constraint, then the public rows; values scaled by R^2
    UVec<uint8_t> s4(4 + nCoefs * 44);
    {
      const uint32_t nc32 = (uint32_t)nCoefs;
      memcpy(s4.data(), &nc32, 4);
    }
    auto rec = [&](uint64_t at, uint32_t mtx, uint32_t c, uint32_t sgn, const uint8_t* coef) {
      uint8_t* o = s4.data() + 4 + at * 44;
      memcpy(o, &mtx, 4);
      memcpy(o + 4, &c, 4);
      memcpy(o + 8, &sgn, 4);
      HFr v = HFr::from_bytes(coef).to_mont();   // limbs = coef * R
      HFr w = v.to_mont();                       // limbs = coef * R^2
      memcpy(o + 12, w.l, 32);
    };
    // constraint ranges in parallel: a range starts at the first A / B term of its first constraint, and its records
    // start at the count of A and B terms before that
    parallel_ranges(r.nConstraints, 1u << 14, [&](unsigned, uint64_t c0, uint64_t c1) {
      auto first = [&](const UVec<Term>& v, uint32_t c) {
        return (size_t)(std::lower_bound(v.begin(), v.end(), c, [](const Term& t, uint32_t key) { return t.c < key; }) - v.begin());
      };
      size_t ia = first(r.A, (uint32_t)c0), ib = first(r.B, (uint32_t)c0);
      uint64_t at = ia + ib;
      for (uint32_t c = (uint32_t)c0; c < (uint32_t)c1; c++) {
        for (; ia < r.A.size() && r.A[ia].c == c; ia++) rec(at++, 0, c, r.A[ia].s, r.A[ia].coef);
        for (; ib < r.B.size() && r.B[ib].c == c; ib++) rec(at++, 1, c, r.B[ib].s, r.B[ib].coef);
      }
    });
    {
      const uint8_t one[32] = {1};
      for (uint32_t i = 0; i <= r.nPublic; i++) rec(r.A.size() + r.B.size() + i, 0, r.nConstraints + i, i, one);
    }
    put_section(4, s4.data(), s4.size());
    UVec<uint8_t> s9(n * 64);
    parallel_ranges(n, 1u << 18, [&](unsigned, uint64_t lo, uint64_t hi) {
      for (uint64_t i = lo; i < hi; i++) memcpy(&s9[i * 64], &Hs[(2 * i + 1) * 64], 64);   // odd points of the 2n basis
    });
    put_section(9, s9.data(), s9.size());
    clock_gettime(CLOCK_MONOTONIC, &h1);
    host_ms = (h1.tv_sec - h0.tv_sec) * 1e3 + (h1.tv_nsec - h0.tv_nsec) / 1e6;
  });
  // a point section is handed to a writer thread as soon as it is back from the device: it goes into the file while the
  // device works on the next one. The section moves into its writer and lives as long as that thread. The device stage
  // below may throw: the tasks are then joined by their destructors, before the file and the inputs declared above go.
  SideTasks writers;
  auto write_async = [&](uint32_t id, UVec<uint8_t>&& sec) {
    writers.start([&, id, sec = std::move(sec)] { put_section(id, sec.data(), sec.size()); });
  };
  std::unique_ptr<DevBuf> dA, dB1, dB2, dKout;   // transcript: the results stay on the device for the circuit hash
  {
    DevBuf dL1(n * 64);
    dL1.up(L1.data(), L1.size());
    dev_check_coords(ctx, dL1.p, 2 * n, "ptau tau*G1 (Lagrange)");
    write_async(5, run_accumulate<Fq>(ctx, dL1, n, eA, m, transcript ? &dA : nullptr));
    write_async(6, run_accumulate<Fq>(ctx, dL1, n, eB, m, transcript ? &dB1 : nullptr));
  }
  {
    DevBuf dL2(n * 128);
    dL2.up(L2.data(), L2.size());
    dev_check_coords(ctx, dL2.p, 4 * n, "ptau tau*G2 (Lagrange)");
    write_async(7, run_accumulate<Fq2>(ctx, dL2, n, eB, m, transcript ? &dB2 : nullptr));
  }
  const UVec<uint8_t> secK = accumulate_k(ctx, pt, n, eK, m, transcript ? &dKout : nullptr);
  phase("point sections (upload, device, download)");
  put_section(3, secK.data(), icb);
  put_section(8, secK.data() + icb, secK.size() - icb);
  if (transcript) {
    uint8_t s10[68] = {0};
    const CsHashPoints k{dKout->p, (const char*)dKout->p + icb, dA->p, dB1->p, dB2->p, r.nPublic, m, n, alpha1, beta1, beta2};
    circuit_hash(ctx, ptau_path, k, phase, s10);
    put_section(10, s10, sizeof s10);
  }
  host_sections.get();   // the host sections' error first, then the writers'
  writers.get();
  if (phase.verbose) fprintf(stderr, "zkpoa: zkey new: (header, coefficient and H sections built and written by a side thread meanwhile: %.1f ms)\n", host_ms);
  out.commit();
  phase("last sections written, key renamed into place");
}

// ---- `snarkjs wtns check <circuit.r1cs> <witness.wtns>` (g16_verify.sh:205-210) ---------------------------------------------
// returns the number of violated constraints; *first_bad = the smallest violated constraint index
uint64_t wtns_check(zkpoa_context* ctx, const char* r1cs_path, const char* wtns_path, uint64_t* first_bad) {
  MappedFile fr(r1cs_path);
  const R1cs r = parse_r1cs(fr);
  MappedFile fw(wtns_path);
  auto ws = bin_sections(fw, "wtns", 2, "wtns");
  if (!ws.count(1) || !ws.count(2)) throw SetupError("wtns: header or data section missing");
  const Sec wh = ws[1], wd = ws[2];
  if (wh.len != 4 + 32 + 4 || rd32(fw.p + wh.off) != 32) throw SetupError("wtns: header has the wrong size");
  for (int i = 0; i < 4; i++)
    if (rd64(fw.p + wh.off + 4 + 8 * i) != HFrParams::P[i]) throw SetupError("wtns: not over the BN254 scalar field");
  const uint64_t nw = rd32(fw.p + wh.off + 36);
  if (nw != r.nWires) throw SetupError("wtns: " + std::to_string(nw) + " values for a circuit of " + std::to_string(r.nWires) + " wires");
  if (wd.len != nw * 32) throw SetupError("wtns: data section has the wrong size");
  const R1csRows rows = r1cs_rows(r);
  const uint64_t nnz = rows.sig.size();
  const std::vector<uint32_t>&row_ptr = rows.row_ptr, &sig = rows.sig;
  const std::vector<uint8_t>& coef = rows.coef;
  hipStream_t st = ctx->dev.lanes[0].stream;
  DevBuf d_rp(row_ptr.size() * 4), d_sig(nnz * 4), d_coef(nnz * 32), d_w(nw * 32), d_flags(64);
  d_rp.up(row_ptr.data(), row_ptr.size() * 4);
  d_sig.up(sig.data(), nnz * 4);
  d_coef.up(coef.data(), nnz * 32);
  d_w.up(fw.p + wd.off, nw * 32);
  const uint32_t init[4] = {0, 0xffffffffu, 0, 0};
  d_flags.up(init, 16);
  uint32_t* fl = reinterpret_cast<uint32_t*>(d_flags.p);
  if (nnz) hipLaunchKernelGGL(fr_to_mont_kernel, dim3((uint32_t)((nnz + 255) / 256)), dim3(256), 0, st, d_coef.p, nnz, fl + 2);
  hipLaunchKernelGGL(fr_to_mont_kernel, dim3((uint32_t)((nw + 255) / 256)), dim3(256), 0, st, d_w.p, nw, fl + 3);
  if (r.nConstraints)
    hipLaunchKernelGGL(wtns_check_kernel, dim3((r.nConstraints + 255) / 256), dim3(256), 0, st, (const uint32_t*)d_rp.p,
                       (const uint32_t*)d_sig.p, (const void*)d_coef.p, (const void*)d_w.p, r.nConstraints, fl,
                       (void*)nullptr, 0u);
  msm_read_back(ctx->dev.lanes[0], fl, 16);
  ZK_HIP(hipGetLastError());
  const uint32_t* hb = ctx->dev.lanes[0].pinned.as<const uint32_t>();
  if (hb[3]) throw SetupError("wtns: a value is not a field element (>= r)");
  if (hb[2]) throw SetupError("r1cs: a coefficient is not a field element (>= r)");
  if (first_bad) *first_bad = hb[1];
  return hb[0];
}

// ---- the arithmetic of `snarkjs zkey contribute` (g16_setup.sh:262-266): delta <- d * delta, C and H <- C, H / d ---------
// rec: null = the arithmetic alone, section 10 copied as it is (zkpoa_zkey_contribute); else the input must carry a
// transcript, and a record is appended. A beacon's delta comes from its generator (delta_le is not read).
void zkey_contribute(zkpoa_context* ctx, const char* in_path, const char* out_path, const uint8_t* delta_le,
                     const zkpoa::phase2::RecordParams* rec) {
  namespace p2 = zkpoa::phase2;
  MappedFile fi(in_path);
  auto secs = bin_sections(fi, "zkey", 1, "zkey");
  for (uint32_t t = 1; t <= 10; t++)
    if (!secs.count(t)) throw SetupError("zkey: section " + std::to_string(t) + " missing");
  const Sec h = secs[2];
  if (h.len != kHdrLen) throw SetupError("zkey: groth16 header has the wrong size");
  const ZkeyHeader zh = read_zkey_header(fi.p + h.off);
  if (zh.n8q != 32 || zh.n8r != 32) throw SetupError("zkey: groth16 header has the wrong size");
  if (!zh.q_ok || !zh.r_ok) throw SetupError("zkey: not a BN254 key");
  const uint64_t nVars = zh.nVars, nPublic = zh.nPublic, domain = zh.domain;
  if (nPublic + 1 > nVars || secs[8].len != (nVars - nPublic - 1) * 64 || secs[9].len != domain * 64)
    throw SetupError("zkey: C or H section has the wrong size");
  p2::Transcript tr;
  uint8_t d[32], g1_s[64];
  if (rec) {
    tr = p2::parse_section10(fi.p + secs[10].off, secs[10].len);
    if (!tr.present()) throw SetupError("zkey: the key carries no transcript (circuit hash is zero): make it with `zkey new --transcript`");
  }
  if (rec && rec->type == 1) {   // d, then g1_s, from the beacon's generator: any verifier recomputes both
    uint32_t key[8];
    p2::beacon_key(rec->beacon.data(), rec->beacon.size(), rec->num_iterations_exp, key);
    p2::ChaCha rng(key);
    p2::beacon_draw(rng, d, g1_s);
  } else {
    if (delta_le) memcpy(d, delta_le, 32);
    else random_scalar(d);
    if (rec) {
      uint8_t sb[1][32];   // ZKPOA_PHASE2_S: the s of g1_s = s * G1
      if (!env_scalars(O_PHASE2_S, sb, 1, "a number in [1, r)", "a secret of the contribution record")) random_scalar(sb[0]);
      h_affine_to_bytes<HFq>(host_generator<HFq>(), g1_s);
      p2::mul_wire<HFq>(g1_s, sb[0], g1_s);
    }
  }
  if (!scalar_in_range(d, true)) throw SetupError("contribute: delta must be in [1, r)");
  HFr dinv = HFr::from_bytes(d).to_mont().inv().from_mont();
  uint8_t dinv_le[32];
  memcpy(dinv_le, dinv.l, 32);

  std::vector<uint8_t> s2(fi.p + h.off, fi.p + h.off + h.len);
  host_check_coords(&s2[kDelta1], 2 + 4, "zkey delta1 / delta2");
  p2::mul_wire<HFq>(&s2[kDelta1], d, &s2[kDelta1]);
  p2::mul_wire<HFq2>(&s2[kDelta2], d, &s2[kDelta2]);
  std::vector<uint8_t> s10(fi.p + secs[10].off, fi.p + secs[10].off + secs[10].len);
  if (rec) {
    p2::Record nr;
    static_cast<p2::RecordParams&>(nr) = *rec;
    memcpy(nr.delta_after, &s2[kDelta1], 64);
    memcpy(nr.g1_s, g1_s, 64);
    p2::mul_wire<HFq>(g1_s, d, nr.g1_sx);
    p2::transcript_hash(tr, tr.records.size(), nr.g1_s, nr.g1_sx, nr.transcript);
    h_affine_to_bytes<HFq2>(p2::hash_to_g2(nr.transcript), nr.g2_spx);
    p2::mul_wire<HFq2>(nr.g2_spx, d, nr.g2_spx);
    tr.records.push_back(nr);
    s10 = p2::write_section10(tr);
  }
  auto scaled = [&](const Sec& sc) {
    UVec<uint8_t> out(sc.len);
    if (sc.len) {
      DevBuf in(sc.len), res(sc.len);
      in.up(fi.p + sc.off, sc.len);
      dev_check_coords(ctx, in.p, sc.len / 32, "zkey C / H section");
      setup_scale<Fq>(ctx, in.p, sc.len / 64, dinv_le, res.p);
      ZK_HIP(hipMemcpy(out.data(), res.p, sc.len, hipMemcpyDeviceToHost));
    }
    return out;
  };
  // the output is sized up front (the section lengths do not change): the sections that are copied as they are go into
  // it from a side thread while the device scales C and H
  uint64_t sec_len[10];
  for (uint32_t t = 1; t <= 10; t++) sec_len[t - 1] = secs[t].len;
  sec_len[9] = s10.size();
  SectionFile out(out_path, "zkey", kZkeyIds, sec_len, 10);   // temporary name + rename: in_path == out_path is fine (the mapping keeps the old inode)
  auto put_section = [&](uint32_t t, const uint8_t* p) { out.put(t, p, out.len(t)); };
  SideTask copier([&] {
    put_section(2, s2.data());
    put_section(10, s10.data());
    for (uint32_t t : {1u, 3u, 4u, 5u, 6u, 7u}) put_section(t, fi.p + secs[t].off);
  });
  {
    const UVec<uint8_t> s8 = scaled(secs[8]);
    put_section(8, s8.data());
  }
  {
    const UVec<uint8_t> s9 = scaled(secs[9]);
    put_section(9, s9.data());
  }
  copier.get();
  out.commit();
}

}  // namespace

// ---- `zkey verify` on a key that carries a transcript: the circuit hash and the contribution records ---------------------
// CSHASH: section 10's circuit hash against the one recomputed from the r1cs and the ptau (the initial IC | C through the
// accumulate path of `zkey new`; the key on disk holds C / delta) and the key's own A, B1, B2 (which `zkey verify` has
// already held to the r1cs and the ptau). CONTRIBUTIONS: every record against the RECOMPUTED circuit hash, so a damaged
// stored hash fails CSHASH alone. The caller has checked the key's shape and the range of its coordinates.
uint32_t zkpoa::phase2_verify(zkpoa_context* ctx, const char* r1cs_path, const char* ptau_path, const char* zkey_path) {
  namespace p2 = zkpoa::phase2;
  PhaseTimer phase("zkey verify", 38);
  MappedFile fk(zkey_path);
  auto ks = bin_sections(fk, "zkey", 1, "zkey");
  p2::Transcript tr = p2::parse_section10(fk.p + ks[10].off, ks[10].len);
  uint32_t failed = 0;
  const uint8_t* hp = fk.p + ks[2].off;
  uint8_t cs[64];
  {
    MappedFile fr(r1cs_path);
    const R1cs r = parse_r1cs(fr);
    const uint32_t cp = domain_log2(r);
    const uint64_t n = 1ull << cp, m = r.nWires, l = r.nPublic;
    const PtauRanges pt = read_ptau_ranges(ptau_path, cp);
    Entries eK;
    build_entries(r, n, nullptr, nullptr, eK);
    std::unique_ptr<DevBuf> dK;
    (void)accumulate_k(ctx, pt, n, eK, m, &dK);
    phase("initial IC | C recomputed");
    DevBuf dIC((l + 1) * 64), dA(m * 64), dB1(m * 64), dB2(m * 128);
    dIC.up(fk.p + ks[3].off, (l + 1) * 64);
    dA.up(fk.p + ks[5].off, m * 64);
    dB1.up(fk.p + ks[6].off, m * 64);
    dB2.up(fk.p + ks[7].off, m * 128);
    const CsHashPoints k{dIC.p, (const char*)dK->p + (l + 1) * 64, dA.p, dB1.p, dB2.p, l, m, n, hp + kAlpha1, hp + kBeta1, hp + kBeta2};
    circuit_hash(ctx, ptau_path, k, phase, cs);
  }
  if (memcmp(cs, tr.cs_hash, 64)) failed |= ZKPOA_ZKEY_CSHASH;
  memcpy(tr.cs_hash, cs, 64);
  // the records: points of their groups, transcript hashes, the two pairing equations, the delta chain, beacons recomputed
  bool ok = true;
  pairing::G1 prev = host_generator<HFq>();
  static const uint64_t kR[4] = {HFrParams::P[0], HFrParams::P[1], HFrParams::P[2], HFrParams::P[3]};
  for (size_t k = 0; k < tr.records.size() && ok; k++) {
    const p2::Record& rc = tr.records[k];
    host_check_coords(rc.delta_after, 2 * 3 + 4, "zkey section 10 points");
    const pairing::G1 da = h_affine_from_bytes<HFq>(rc.delta_after), s = h_affine_from_bytes<HFq>(rc.g1_s),
                      sx = h_affine_from_bytes<HFq>(rc.g1_sx);
    const pairing::G2 spx = h_affine_from_bytes<HFq2>(rc.g2_spx);
    if (da.is_inf() || s.is_inf() || sx.is_inf() || spx.is_inf() || !pairing::g1_on_curve(da) || !pairing::g1_on_curve(s) ||
        !pairing::g1_on_curve(sx) || !pairing::g2_on_curve(spx) || !h_mul(XYZZ<HFq2>::from_affine(spx), kR).is_inf()) {
      ok = false;
      break;
    }
    uint8_t th[64];
    p2::transcript_hash(tr, k, rc.g1_s, rc.g1_sx, th);
    if (memcmp(th, rc.transcript, 64)) ok = false;
    const pairing::G2 sp = p2::hash_to_g2(th);
    if (ok && !pairing::pair_eq(s, spx, sx, sp)) ok = false;      // the same d in g1_sx and g2_spx
    if (ok && !pairing::pair_eq(da, sp, prev, spx)) ok = false;   // deltaAfter_k = d * deltaAfter_{k-1}
    if (ok && rc.type == 1) {
      if (rc.num_iterations_exp > p2::kMaxBeaconExp) ok = false;
      else {
        uint32_t key[8];
        uint8_t d[32], want[64];
        p2::beacon_key(rc.beacon.data(), rc.beacon.size(), rc.num_iterations_exp, key);
        p2::ChaCha rng(key);
        p2::beacon_draw(rng, d, want);
        if (memcmp(want, rc.g1_s, 64)) ok = false;
        p2::mul_wire<HFq>(want, d, want);
        if (memcmp(want, rc.g1_sx, 64)) ok = false;
      }
    }
    prev = da;
  }
  uint8_t last[64];
  h_affine_to_bytes<HFq>(prev, last);
  if (!ok || memcmp(last, hp + kDelta1, 64)) failed |= ZKPOA_ZKEY_CONTRIBUTIONS;
  phase("contribution records");
  return failed;
}

// host only: does the key carry a transcript, how many records, and one line "<type> <name>" per record
extern "C" int zkpoa_zkey_contributions(const char* zkey_path, int* has_transcript, uint32_t* count, char* text,
                                        unsigned long cap) {
  try {
    if (!zkey_path || !has_transcript || !count) return PROVER_ERROR;
    MappedFile fk(zkey_path);
    auto ks = bin_sections(fk, "zkey", 1, "zkey");
    if (!ks.count(10)) return PROVER_ERROR;
    const zkpoa::phase2::Transcript tr = zkpoa::phase2::parse_section10(fk.p + ks[10].off, ks[10].len);
    *has_transcript = tr.present() ? 1 : 0;
    *count = (uint32_t)tr.records.size();
    std::string out;
    for (const auto& r : tr.records) out += std::string(r.type == 1 ? "beacon " : "contribution ") + r.name + "\n";
    if (text && cap) zkpoa::set_err(text, cap, out);
    return PROVER_OK;
  } catch (const std::exception&) {
    return PROVER_ERROR;
  }
}

extern "C" int zkpoa_wtns_check(zkpoa_context* ctx, const char* r1cs_path, const char* wtns_path, uint64_t* violated,
                                uint64_t* first_violated) {
  ZK_API_BEGIN(ctx)
  if (!r1cs_path || !wtns_path || !violated) throw SetupError("wtns check: null argument");
  *violated = wtns_check(ctx, r1cs_path, wtns_path, first_violated);
  ZK_API_END(ctx)
}

extern "C" int zkpoa_zkey_contribute(zkpoa_context* ctx, const char* zkey_in_path, const char* zkey_out_path,
                                     const uint8_t* delta_le) {
  ZK_API_BEGIN(ctx)
  if (!zkey_in_path || !zkey_out_path) throw SetupError("zkey contribute: null path");
  zkey_contribute(ctx, zkey_in_path, zkey_out_path, delta_le, nullptr);
  ZK_API_END(ctx)
}

extern "C" int zkpoa_zkey_contribute_ex(zkpoa_context* ctx, const char* zkey_in_path, const char* zkey_out_path,
                                        const uint8_t* delta_le, const char* name) {
  ZK_API_BEGIN(ctx)
  if (!zkey_in_path || !zkey_out_path) throw SetupError("zkey contribute: null path");
  zkpoa::phase2::RecordParams rec;
  rec.name = name ? name : "";
  rec.check("zkey contribute");
  zkey_contribute(ctx, zkey_in_path, zkey_out_path, delta_le, &rec);
  ZK_API_END(ctx)
}

extern "C" int zkpoa_zkey_beacon(zkpoa_context* ctx, const char* zkey_in_path, const char* zkey_out_path,
                                 const uint8_t* beacon, unsigned long beacon_len, uint32_t num_iterations_exp,
                                 const char* name) {
  ZK_API_BEGIN(ctx)
  if (!zkey_in_path || !zkey_out_path || (!beacon && beacon_len)) throw SetupError("zkey beacon: null argument");
  zkpoa::phase2::RecordParams rec;
  rec.type = 1;
  rec.name = name ? name : "";
  rec.beacon.assign(beacon, beacon + beacon_len);
  rec.num_iterations_exp = num_iterations_exp;
  rec.check("zkey beacon");
  zkey_contribute(ctx, zkey_in_path, zkey_out_path, nullptr, &rec);
  ZK_API_END(ctx)
}

// test hooks of the transcript's device work: the hash form (compressed: csrc/ptau_contribute.hip's hook, the compressed
// form, half the bytes) of n points of group 1 / 2 (host wire form) streamed in pieces of piece_points, its Blake2b-512
// digest, and optionally the bytes. The hash form's coordinates are range-checked on the device, the compressed form's
// on the host. Then T[i + n] - T[i] over 2n - 1 points.
void zkpoa::points_form(zkpoa_context* ctx, int group, const void* points, uint64_t n, uint64_t piece_points, bool compressed,
                        void* out, uint8_t digest[64]) {
  const char* const what = compressed ? "compressed form" : "hash form";
  if ((group != 1 && group != 2) || (n && !points) || !digest) throw SetupError(std::string(what) + ": bad argument");
  const uint64_t unit = group == 1 ? 64 : 128;
  if (compressed) host_check_coords(static_cast<const uint8_t*>(points), n * unit / 32, what);
  DevBuf d(n * unit);
  d.up(points, n * unit);
  if (!compressed) dev_check_coords(ctx, d.p, n * unit / 32, what);
  zkpoa::phase2::Blake2b h;
  HashStream hs(ctx, h, piece_points);
  std::vector<uint8_t> cap;
  if (out) hs.capture = &cap;
  hs.points(d.p, n, group, false, compressed);
  h.final(digest);
  if (out && n) memcpy(out, cap.data(), cap.size());
}
extern "C" int zkpoa_hash_form(zkpoa_context* ctx, int group, const void* points, uint64_t n, uint64_t piece_points,
                               void* out_bytes, uint8_t digest[64]) {
  ZK_API_BEGIN(ctx)
  points_form(ctx, group, points, n, piece_points, false, out_bytes, digest);
  ZK_API_END(ctx)
}

extern "C" int zkpoa_h_diff(zkpoa_context* ctx, const void* points, uint64_t n, void* out) {
  ZK_API_BEGIN(ctx)
  if (n < 2 || !points || !out) throw SetupError("h diff: bad argument");
  DevBuf dT((2 * n - 1) * 64), dH((n - 1) * 64);
  dT.up(points, (2 * n - 1) * 64);
  dev_check_coords(ctx, dT.p, 2 * (2 * n - 1), "h diff");
  h_diff(ctx, dT.p, n, dH.p);
  ZK_HIP(hipMemcpy(out, dH.p, (n - 1) * 64, hipMemcpyDeviceToHost));
  ZK_API_END(ctx)
}

extern "C" void zkpoa_setup_defer_host_frees(int on) { defer_host_frees() = on != 0; }

extern "C" int zkpoa_zkey_new(zkpoa_context* ctx, const char* r1cs_path, const char* ptau_path, const char* zkey_path) {
  ZK_API_BEGIN(ctx)
  if (!r1cs_path || !ptau_path || !zkey_path) throw SetupError("zkey new: null path");
  zkey_new(ctx, r1cs_path, ptau_path, zkey_path, 0);
  ZK_API_END(ctx)
}

extern "C" int zkpoa_zkey_new_ex(zkpoa_context* ctx, const char* r1cs_path, const char* ptau_path, const char* zkey_path,
                                 uint32_t flags) {
  ZK_API_BEGIN(ctx)
  if (!r1cs_path || !ptau_path || !zkey_path) throw SetupError("zkey new: null path");
  if (flags & ~(uint32_t)ZKPOA_SETUP_TRANSCRIPT) throw SetupError("zkey new: unknown flag");
  zkey_new(ctx, r1cs_path, ptau_path, zkey_path, flags);
  ZK_API_END(ctx)
}
