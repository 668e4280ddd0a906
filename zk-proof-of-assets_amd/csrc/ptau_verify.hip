// `snarkjs powersoftau verify <pot.ptau>` on the device: do the powers of a ceremony file belong to one tau, alpha, beta,
// and do its Lagrange-form sections (what `zkey new` reads) agree with them? The reference trusts the file blindly
// (scripts/g16_setup.sh:201 and scripts/g16_verify.sh:164: "TODO verify ptau file").
//
// snarkjs ptau layout, power p, N = 2^p: T = section 2 (2N - 1 G1 points tau^i G1), U = section 3 (N G2 points tau^i G2),
// A = section 4 (alpha tau^i G1), B = section 5 (beta tau^i G1), beta2 = section 6; level l of sections 12-15 starts at
// point 2^l - 1 and holds the 2^l Lagrange-form points L_j(tau) X (section 12: levels 0..p+1, 13-15: 0..p).
//
// Every check is a random linear combination (weights from /dev/urandom, drawn after the file is read):
//   ratio checks, one MSM per power section: M = sum_{i<K} rho^i X_i gives both sides of
//     e(sum_{i<K-1} rho^i X_i, U_1) = e(sum_{i<K-1} rho^i X_{i+1}, G2)   as   M - rho^(K-1) X_{K-1}  and  (M - X_0) / rho
//   Lagrange checks, one MSM per side: for a level of n points and any P(x) = sum_{i<n} u_i x^i,
//     sum_j P(w_n^j) L_j(tau) = P(tau);  with u_i = rho_l^i (one rho_l per level), P(w^j) = (1 - rho_l^n) / (1 - rho_l w^j),
//     summed over all levels: sum_{l,j} P_l(w^j) Lag_{l,j} = sum_i s_i X_i,  s_i = sum_{l : i < 2^l} rho_l^i.
//     The top level p+1 of section 12 would need tau^(2N-1), which the file does not hold: that level is checked on
//     the 2N - 1 powers that exist (u_{2N-1} = 0, P(x) = (1 - (rho x)^(2N-1)) / (1 - rho x)).
// The weights are made on the device per piece (power tables by thread runs; the Lagrange side's 1 / (1 - rho w^j) by a
// batched inversion, Montgomery's trick per thread run). Each section streams through HBM in pieces
// (csrc/setup_common.hip.h: for_each_piece; the file as it is opened: csrc/ptau_file.hip.h; the sections' point counts: csrc/binfile.hpp): upload from the file, point checks (curve, range, G2 subgroup), MSMs with the piece's weights; the partial sums are added on the host.
// Section 7 (DESIGN.md "Phase-1 transcript"): its records are checked on the host (csrc/phase1.hpp: keys, ratios, the
// beacon, the last record against the file's points); the last nextChallenge needs the hash form of sections 2-6, which
// streams from the file through the device conversion of csrc/phase2_dev.hip.h into Blake2b.
#include "phase2_dev.hip.h"
#include "ptau_file.hip.h"
#include "zkpoa_internal.hpp"

#include <type_traits>
#include <vector>

using namespace zkpoa;

namespace {

constexpr uint32_t kRun = 16;   // consecutive weights per thread: one exponentiation (and one inversion) per run

// level l of the Lagrange sections (n = 2^l points), Montgomery form; the same rho_l for every section
struct PtauLevel {
  Fr rho;     // rho_l
  Fr w;       // w_n, the n-th root of unity of the level
  Fr w_inv;   // w_n^-1
  Fr c;       // top == 0: 1 - rho^n (the numerator of every weight of the level); top == 1: rho^(n-1)
  uint32_t top, pad[7];
};

// out[e] = P_l(w^j) in standard form for the points g0 + e, e < cnt, of a Lagrange section (global point index g: level
// l = log2(g + 1), j = g + 1 - 2^l). One run of kRun weights per thread: the denominators 1 - rho w^j are inverted together
// (the prefix products, times the numerators, go through `out`; the denominators stay in registers).
static __global__ __launch_bounds__(256) void lagrange_weights_kernel(const PtauLevel* __restrict__ lv, uint64_t g0,
                                                                      uint64_t cnt, void* __restrict__ out) {
  const uint64_t e0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * kRun;
  if (e0 >= cnt) return;
  const uint32_t m = (uint32_t)(cnt - e0 < kRun ? cnt - e0 : kRun);
  char* o = reinterpret_cast<char*>(out) + 32 * e0;
  const uint64_t first = g0 + e0 + 1;
  PtauLevel L = lv[63 - __builtin_clzll(first)];
  const uint64_t j0 = first - (1ull << (63 - __builtin_clzll(first)));
  Fr x = L.rho * fr_pow_u64(L.w, j0);                       // rho w^j
  Fr wj_inv = L.top ? fr_pow_u64(L.w_inv, j0) : Fr::one();  // w^-j (top level only)
  Fr den[kRun];
  Fr acc = Fr::one();
#pragma unroll
  for (uint32_t k = 0; k < kRun; k++) {
    den[k] = Fr::one();
    if (k < m) {
      if (k > 0) {
        const uint64_t gk = first + k;
        if ((gk & (gk - 1)) == 0) {   // a new level starts inside the run, at j = 0
          L = lv[63 - __builtin_clzll(gk)];
          x = L.rho;
          wj_inv = Fr::one();
        } else {
          x = x * L.w;
          if (L.top) wj_inv = wj_inv * L.w_inv;
        }
      }
      den[k] = Fr::one() - x;
      const Fr num = L.top ? Fr::one() - L.c * wj_inv : L.c;
      store_field(o + 32 * k, num * acc);
      acc = acc * den[k];
    }
  }
  Fr inv = acc.inv();
#pragma unroll
  for (int k = kRun - 1; k >= 0; k--) {
    if ((uint32_t)k < m) {
      store_field(o + 32 * k, (load_field<Fr>(o + 32 * k) * inv).from_mont());
      inv = inv * den[k];
    }
  }
}

// For the points g0 + e, e < cnt, of a power section of K points, standard form: ratio[e] = rho^g and (lag != null)
// lag[e] = s_g = sum over the levels l < n_levels with g < min(2^l, K) of rho_l^g.
static __global__ __launch_bounds__(256) void power_weights_kernel(const PtauLevel* __restrict__ lv, uint32_t n_levels,
                                                                   Fr rho, uint64_t g0, uint64_t cnt, uint64_t K,
                                                                   void* __restrict__ ratio, void* __restrict__ lag) {
  const uint64_t e0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * kRun;
  if (e0 >= cnt) return;
  const uint32_t m = (uint32_t)(cnt - e0 < kRun ? cnt - e0 : kRun);
  const uint64_t g = g0 + e0;
  char* orat = reinterpret_cast<char*>(ratio) + 32 * e0;
  Fr t = fr_pow_u64(rho, g);
#pragma unroll
  for (uint32_t k = 0; k < kRun; k++) {
    if (k < m) {
      store_field(orat + 32 * k, t.from_mont());
      t = t * rho;
    }
  }
  if (!lag) return;
  Fr s[kRun];
#pragma unroll
  for (uint32_t k = 0; k < kRun; k++) s[k] = Fr::zero();
  for (uint32_t l = 0; l < n_levels; l++) {
    const uint64_t lim = (1ull << l) < K ? (1ull << l) : K;
    if (g >= lim) continue;
    const Fr r = lv[l].rho;
    Fr p = fr_pow_u64(r, g);
#pragma unroll
    for (uint32_t k = 0; k < kRun; k++) {
      if (k < m && g + k < lim) {
        s[k] = s[k] + p;
        p = p * r;
      }
    }
  }
  char* olag = reinterpret_cast<char*>(lag) + 32 * e0;
#pragma unroll
  for (uint32_t k = 0; k < kRun; k++)
    if (k < m) store_field(olag + 32 * k, s[k].from_mont());
}

HFr fr_pow_host(const HFr& b, uint64_t e) {
  const uint64_t ex[4] = {e, 0, 0, 0};
  return b.pow(ex);
}
template <class HF>
XYZZ<HF> xyzz_of(const uint8_t* wire) {
  return XYZZ<HF>::from_affine(h_affine_from_bytes<HF>(wire));
}
template <class HF>
XYZZ<HF> xyzz_sub(XYZZ<HF> a, const XYZZ<HF>& b) {
  xyzz_add(a, xyzz_neg(b));
  return a;
}
template <class HF>
XYZZ<HF> xyzz_scale(const XYZZ<HF>& p, const HFr& k) {   // k: Montgomery form
  const HFr s = k.from_mont();
  return h_mul(p, s.l);
}

// One section at a time through HBM, `piece` points per upload: point checks, then the MSMs of the piece's weights.
struct Streamer {
  zkpoa_context* ctx;
  int fd;
  uint64_t piece;
  hipStream_t st;
  DevBuf pts, w1, w2;
  const PtauLevel* d_lv;
  PointChecker points;
  bool bad_points = false;   // a point off its curve or (subgroup) outside G2
  Streamer(zkpoa_context* c, int f, uint64_t pc, const PtauLevel* lv)
      : ctx(c), fd(f), piece(pc), st(c->dev.lanes[0].stream), pts(pc * 128), w1(pc * 32), w2(pc * 32), d_lv(lv), points(c) {}
  enum Mode { kCheck, kPower, kLagrange };
  // kPower: *ratio += sum rho^i X_i and, with n_levels, *lag += sum s_i X_i; kLagrange: *lag += sum P_l(w^j) X_{l,j}
  template <class HF>
  void run(const Sec& sc, uint64_t K, bool subgroup, Mode mode, const HFr* rho, uint32_t n_levels, const char* what,
           XYZZ<HF>* ratio, XYZZ<HF>* lag) {
    constexpr bool kG2 = std::is_same<HF, HFq2>::value;
    constexpr uint64_t unit = kG2 ? 128 : 64;
    for_each_piece(ctx, fd, sc.off, K, unit, piece, pts.p, [&](uint64_t i0, uint64_t cnt) {
      if (points.check(pts.p, cnt, kG2 ? 2 : 1, subgroup, what) & 6u) bad_points = true;
      if (mode == kCheck) return;
      const dim3 wgrid((uint32_t)((cnt + 256 * kRun - 1) / (256 * kRun)));
      if (mode == kPower)
        hipLaunchKernelGGL(power_weights_kernel, wgrid, dim3(256), 0, st, d_lv, n_levels, fr_dev(*rho), i0, cnt, K, w1.p,
                           n_levels ? w2.p : nullptr);
      else hipLaunchKernelGGL(lagrange_weights_kernel, wgrid, dim3(256), 0, st, d_lv, i0, cnt, w1.p);
      ZK_HIP(hipGetLastError());
      auto msm = [&](const void* sc_d, XYZZ<HF>* acc) {
        uint8_t out[2 * unit];
        if (kG2) msm_run_g2(ctx, 0, pts.p, sc_d, cnt, out, nullptr);
        else msm_run_g1(ctx, 0, pts.p, sc_d, cnt, out, nullptr);
        xyzz_add(*acc, xyzz_of<HF>(out));
      };
      if (mode == kPower) {
        msm(w1.p, ratio);
        if (n_levels) msm(w2.p, lag);
      } else {
        msm(w1.p, lag);
      }
    });
  }
};

using pairing::pair_eq;

HFr draw_nonzero() {   // 253 random bits from /dev/urandom (below r), Montgomery form; 0 is drawn again
  for (;;) {
    uint8_t b[32];
    urandom(b, 32);
    b[31] &= 0x1f;
    const HFr v = HFr::from_bytes(b);
    if (v.l[0] | v.l[1] | v.l[2] | v.l[3]) return v.to_mont();
  }
}

uint32_t ptau_verify(zkpoa_context* ctx, const char* path, uint64_t piece_points, uint32_t info[4]) {
  PhaseTimer phase("powersoftau verify", 34);
  // ---- the file's shape: anything that contradicts the header is a malformed file
  PtauInput in(path, false);   // the records: after the checks of sections 12-15
  auto& [fp, ps, shape, records] = in;
  const uint32_t power = shape.power;
  const uint64_t N = 1ull << power;
  if (in.lagrange() == PtauInput::kSome) throw SetupError("ptau: only some of sections 12-15 (Lagrange form) are present");
  const bool prepared = in.lagrange() == PtauInput::kAll;
  if (prepared) {
    ptau_check_preparable(power);
    for (const LagrangeSec& sc : ptau_lagrange_secs(power))
      if (ps[sc.dst].len != sc.bytes()) throw SetupError("ptau: section " + std::to_string(sc.dst) + " has the wrong length for power " + std::to_string(power));
  }
  info[0] = power;
  info[1] = shape.ceremony;
  info[2] = prepared ? 1 : 0;
  info[3] = shape.contributions;
  in.parse_records();
  phase("sections");

  // ---- random weights: one rho per power section (ratio checks), one rho_l per level (Lagrange checks)
  const uint32_t n_levels = prepared ? power + 2 : 0;
  HFr rho_T, rho_U, rho_A, rho_B;
  std::vector<PtauLevel> lv(n_levels ? n_levels : 1);
  {
    rho_T = draw_nonzero();
    rho_U = draw_nonzero();
    rho_A = draw_nonzero();
    rho_B = draw_nonzero();
    // w_{2^28} = 5^((r - 1) / 2^28); w_{2^l} = w_{2^28}^(2^(28 - l))
    uint64_t e[4];
    for (int i = 0; i < 4; i++) e[i] = (HFrParams::P[i] >> 28) | (i < 3 ? HFrParams::P[i + 1] << 36 : 0);
    const HFr w28 = HFr::from_u64(5).pow(e);
    for (uint32_t l = 0; l < n_levels; l++) {
      HFr w = w28;
      for (uint32_t s = l; s < 28; s++) w = w.sqr();
      HFr rho, rho_n;
      do {   // rho^n = 1 would make a denominator 1 - rho w^j zero
        rho = draw_nonzero();
        rho_n = rho;
        for (uint32_t s = 0; s < l; s++) rho_n = rho_n.sqr();
      } while (rho_n == HFr::one());
      PtauLevel& L = lv[l];
      memset(&L, 0, sizeof L);
      L.rho = fr_dev(rho);
      L.w = fr_dev(w);
      L.w_inv = fr_dev(w.inv());
      L.top = l == power + 1;
      L.c = fr_dev(L.top ? rho_n * rho.inv() : HFr::one() - rho_n);
    }
  }
  DevBuf d_lv(lv.size() * sizeof(PtauLevel));
  d_lv.up(lv.data(), lv.size() * sizeof(PtauLevel));
  phase("random weights");

  // ---- the sections, streamed
  if (!piece_points) piece_points = piece_from_free_hbm(128 + 64, 1ull << 16, 1ull << 26);   // the piece's points and weights
  piece_points = std::min<uint64_t>(piece_points, 4 * N);   // no piece larger than the largest section
  Streamer sm(ctx, fp.fd, piece_points, (const PtauLevel*)d_lv.p);
  typedef XYZZ<HFq> P1;
  typedef XYZZ<HFq2> P2;
  P1 mT = P1::inf(), mA = P1::inf(), mB = P1::inf(), sT = P1::inf(), sA = P1::inf(), sB = P1::inf();
  P1 lT = P1::inf(), lA = P1::inf(), lB = P1::inf();
  P2 mU = P2::inf(), sU = P2::inf(), lU = P2::inf();
  const auto pw = ptau_power_secs(power);   // sections 2-6: the typed sums above fix the order, the table the counts
  sm.run<HFq>(ps[2], pw[0].count, false, Streamer::kPower, &rho_T, n_levels, "ptau section 2", &mT, &sT);
  sm.run<HFq2>(ps[3], pw[1].count, true, Streamer::kPower, &rho_U, n_levels ? power + 1 : 0, "ptau section 3", &mU, &sU);
  sm.run<HFq>(ps[4], pw[2].count, false, Streamer::kPower, &rho_A, n_levels ? power + 1 : 0, "ptau section 4", &mA, &sA);
  sm.run<HFq>(ps[5], pw[3].count, false, Streamer::kPower, &rho_B, n_levels ? power + 1 : 0, "ptau section 5", &mB, &sB);
  sm.run<HFq2>(ps[6], pw[4].count, true, Streamer::kCheck, nullptr, 0, "ptau section 6", (P2*)nullptr, (P2*)nullptr);
  phase("powers (upload, checks, MSMs)");
  if (prepared) {
    const auto lg = ptau_lagrange_secs(power);   // sections 12-15
    sm.run<HFq>(ps[12], lg[0].count(), false, Streamer::kLagrange, nullptr, 0, "ptau section 12", (P1*)nullptr, &lT);
    sm.run<HFq2>(ps[13], lg[1].count(), true, Streamer::kLagrange, nullptr, 0, "ptau section 13", (P2*)nullptr, &lU);
    sm.run<HFq>(ps[14], lg[2].count(), false, Streamer::kLagrange, nullptr, 0, "ptau section 14", (P1*)nullptr, &lA);
    sm.run<HFq>(ps[15], lg[3].count(), false, Streamer::kLagrange, nullptr, 0, "ptau section 15", (P1*)nullptr, &lB);
    phase("Lagrange form (upload, checks, MSMs)");
  }

  // ---- single points (every coordinate passed the range check above) and the pairings
  uint32_t failed = sm.bad_points ? ZKPOA_PTAU_POINTS : 0;
  const uint8_t* pT = fp.p + ps[2].off;
  const uint8_t* pU = fp.p + ps[3].off;
  const uint8_t* pA = fp.p + ps[4].off;
  const uint8_t* pB = fp.p + ps[5].off;
  const uint8_t* pb2 = fp.p + ps[6].off;
  uint8_t g1b[64], g2b[128], zero[128] = {0};
  h_affine_to_bytes<HFq>(host_generator<HFq>(), g1b);
  h_affine_to_bytes<HFq2>(host_generator<HFq2>(), g2b);
  if (memcmp(pT, g1b, 64) || memcmp(pU, g2b, 128) || !memcmp(pT + 64, zero, 64) || !memcmp(pA, zero, 64) ||
      !memcmp(pB, zero, 64) || !memcmp(pb2, zero, 128))
    failed |= ZKPOA_PTAU_POINTS;
  const pairing::G1 G1 = host_generator<HFq>(), T1 = h_affine_from_bytes<HFq>(pT + 64), B0 = h_affine_from_bytes<HFq>(pB);
  const pairing::G2 G2 = host_generator<HFq2>(), U1 = h_affine_from_bytes<HFq2>(pU + 128),
                    beta2 = h_affine_from_bytes<HFq2>(pb2);
  // sum_{i<K-1} rho^i X_i = M - rho^(K-1) X_{K-1};  sum_{i<K-1} rho^i X_{i+1} = (M - X_0) / rho
  auto lhs = [](const auto& M, const HFr& rho, const auto& last, uint64_t K) {
    return h_to_affine(xyzz_sub(M, xyzz_scale(last, fr_pow_host(rho, K - 1))));
  };
  auto rhs = [](const auto& M, const HFr& rho, const auto& first) { return h_to_affine(xyzz_scale(xyzz_sub(M, first), rho.inv())); };
  {
    const P1 last = xyzz_of<HFq>(pT + 64 * (2 * N - 2)), first = xyzz_of<HFq>(pT);
    if (!pair_eq(lhs(mT, rho_T, last, 2 * N - 1), U1, rhs(mT, rho_T, first), G2) || !pair_eq(T1, G2, G1, U1))
      failed |= ZKPOA_PTAU_TAU_G1;
  }
  {
    const P2 last = xyzz_of<HFq2>(pU + 128 * (N - 1)), first = xyzz_of<HFq2>(pU);
    if (!pair_eq(T1, lhs(mU, rho_U, last, N), G1, rhs(mU, rho_U, first))) failed |= ZKPOA_PTAU_TAU_G2;
  }
  {
    const P1 last = xyzz_of<HFq>(pA + 64 * (N - 1)), first = xyzz_of<HFq>(pA);
    if (!pair_eq(lhs(mA, rho_A, last, N), U1, rhs(mA, rho_A, first), G2)) failed |= ZKPOA_PTAU_ALPHA;
  }
  {
    const P1 last = xyzz_of<HFq>(pB + 64 * (N - 1)), first = xyzz_of<HFq>(pB);
    if (!pair_eq(lhs(mB, rho_B, last, N), U1, rhs(mB, rho_B, first), G2) || !pair_eq(B0, G2, G1, beta2))
      failed |= ZKPOA_PTAU_BETA;
  }
  if (prepared) {
    if (!xyzz_sub(lT, sT).is_inf()) failed |= ZKPOA_PTAU_LAGRANGE_TAU_G1;
    if (!xyzz_sub(lU, sU).is_inf()) failed |= ZKPOA_PTAU_LAGRANGE_TAU_G2;
    if (!xyzz_sub(lA, sA).is_inf()) failed |= ZKPOA_PTAU_LAGRANGE_ALPHA;
    if (!xyzz_sub(lB, sB).is_inf()) failed |= ZKPOA_PTAU_LAGRANGE_BETA;
  }
  phase("pairings");
  // ---- section 7: the records, then the last nextChallenge over the file's own sections 2-6
  if (!records.empty()) {
    uint8_t response[64], next[64];
    bool ok = zkpoa::phase1::verify_records(records, power, pT + 64, pU + 128, pA, pB, pb2, response);
    phase("contribution records (host)");
    if (ok) {
      zkpoa::phase2::Blake2b h;
      h.update(response, 64);
      HashStream hs(ctx, h, 0);
      hash_form_ptau_sections(ctx, hs, fp.fd, ps, power, sm.pts.p, sm.piece);
      h.final(next);
      ok = !memcmp(next, records.back().next_challenge, 64);
      phase("nextChallenge (device hash form, Blake2b)");
    }
    if (!ok) failed |= ZKPOA_PTAU_CONTRIBUTIONS;
  }
  return failed;
}

}  // namespace

extern "C" int zkpoa_ptau_verify(zkpoa_context* ctx, const char* ptau_path, uint64_t piece_points, uint32_t* failed_checks,
                                 uint32_t info[4]) {
  ZK_API_BEGIN(ctx)
  if (!ptau_path || !failed_checks || !info) throw SetupError("powersoftau verify: null argument");
  uint32_t inf[4] = {0, 0, 0, 0};
  *failed_checks = ptau_verify(ctx, ptau_path, piece_points, inf);
  memcpy(info, inf, sizeof inf);
  ZK_API_END(ctx)
}
