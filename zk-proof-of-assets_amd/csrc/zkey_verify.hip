// `snarkjs zkey verify <circuit.r1cs> <pot.ptau> <circuit.zkey>` (g16_verify.sh -z) on the device: is this key what
// `zkey new` makes of this circuit and this ceremony, followed by contributions to delta only?
#include "abc.hip.h"
#include "setup_common.hip.h"

using namespace zkpoa;

namespace {

// Row j < n of the folds (Montgomery form): rs = [a | b | c] from the r1cs (wtns_check_kernel), ks = [a' | b'] from the
// key's section 4 (abc_rows_kernel). flags |= 1 where a' != a or b' != b; rs[0, 3n) is then rewritten in place as the
// standard-form scalars of the MSMs.
static __global__ __launch_bounds__(256) void fold_compare_kernel(void* __restrict__ rs, const void* __restrict__ ks,
                                                                  uint32_t n, uint32_t* __restrict__ flags) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  char* r = reinterpret_cast<char*>(rs);
  const char* k = reinterpret_cast<const char*>(ks);
  const Fr a = load_field<Fr>(r + 32 * (size_t)j), b = load_field<Fr>(r + 32 * ((size_t)n + j)),
           c = load_field<Fr>(r + 32 * (2 * (size_t)n + j));
  if (a != load_field<Fr>(k + 32 * (size_t)j) || b != load_field<Fr>(k + 32 * ((size_t)n + j))) atomicOr(flags, 1u);
  store_field(r + 32 * (size_t)j, a.from_mont());
  store_field(r + 32 * ((size_t)n + j), b.from_mont());
  store_field(r + 32 * (2 * (size_t)n + j), c.from_mont());
}

// ---- `snarkjs zkey verify <circuit.r1cs> <pot.ptau> <circuit.zkey>` (g16_verify.sh -z) --------------------------------------
// Restates what zkey_new and zkey_contribute compute, with random weights instead of the points one by one: rho over the
// wires, sigma over the domain (253 random bits each, from /dev/urandom), folds a = A rho, b = B rho, c = C rho per row
// (A extended by the public rows) from the r1cs on one side and, for a and b, from the key's section 4 on the other; then
//   A:  sum rho_i A_i  = sum a_j L1_j          B1 / B2: sum rho_i B_i = sum b_j L_j (G1 / G2)
//   ICCH: e(sum_{i<=l} rho_i IC_i - Q, G2) e(sum_{i>l} rho_i C_i + sum sigma_j H_j, delta2) = 1,
//         Q = sum a_j bL_j + b_j aL_j + c_j L1_j + sigma_j Hodd_j (one MSM over the four ptau ranges back to back)
// Returns the bitmask of failed checks (include/zkpoa_prover.h ZKPOA_ZKEY_*); a malformed file throws. One key section at a
// time is on the device. Section 10: a zero circuit hash ("no transcript") is not looked at further; otherwise the circuit
// hash and the contribution records are checked as well (setup.hip phase2_verify, DESIGN.md "Phase-2 transcript").
uint32_t zkey_verify(zkpoa_context* ctx, const char* r1cs_path, const char* ptau_path, const char* zkey_path) {
  PhaseTimer phase("zkey verify", 38);
  MappedFile fr(r1cs_path);
  const R1cs r = parse_r1cs(fr);
  const uint32_t cp = domain_log2(r);
  const uint64_t n = 1ull << cp, m = r.nWires, l = r.nPublic, nC = r.nConstraints;
  phase("r1cs parsed");

  // ---- the key's shape: everything that contradicts the circuit or itself is a malformed file
  MappedFile fk(zkey_path);
  auto ks = bin_sections(fk, "zkey", 1, "zkey");
  for (uint32_t t = 1; t <= 9; t++)
    if (!ks.count(t)) throw SetupError("zkey: section " + std::to_string(t) + " missing");
  // a transcript: section 10 starts with a circuit hash that is not zero (a key without one is checked as before)
  bool transcript = false;
  if (ks.count(10) && ks[10].len >= 64)
    for (int i = 0; i < 64; i++) transcript |= fk.p[ks[10].off + i] != 0;
  if (ks[1].len != 4) throw SetupError("zkey: section 1 has the wrong size");
  if (ks[2].len != kHdrLen) throw SetupError("zkey: groth16 header has the wrong size");
  const uint8_t* hp = fk.p + ks[2].off;
  const ZkeyHeader h = read_zkey_header(hp);
  if (h.n8q != 32 || h.n8r != 32) throw SetupError("zkey: groth16 header has the wrong size");
  uint32_t failed = 0;
  if (!h.q_ok || !h.r_ok) failed |= ZKPOA_ZKEY_HEADER;
  if (rd32(fk.p + ks[1].off) != 1) failed |= ZKPOA_ZKEY_HEADER;   // protocol 1 = groth16
  const uint64_t kNVars = h.nVars, kNPublic = h.nPublic, kDomain = h.domain;
  if (kNVars != m) throw SetupError("zkey: nVars = " + std::to_string(kNVars) + ", the r1cs has " + std::to_string(m) + " wires");
  if (kNPublic != l) throw SetupError("zkey: nPublic = " + std::to_string(kNPublic) + ", the r1cs has " + std::to_string(l));
  if (kDomain != n) throw SetupError("zkey: domain " + std::to_string(kDomain) + ", the r1cs needs " + std::to_string(n));
  const uint64_t want_len[10] = {0, 4, 0, (l + 1) * 64, 0, m * 64, m * 64, m * 128, (m - l - 1) * 64, n * 64};
  for (uint32_t t : {3u, 5u, 6u, 7u, 8u, 9u})
    if (ks[t].len != want_len[t]) throw SetupError("zkey: section " + std::to_string(t) + " has the wrong size");
  if (ks[4].len < 4) throw SetupError("zkey: section 4 has the wrong size");
  const uint64_t nCoefs = rd32(fk.p + ks[4].off);
  if (ks[4].len != 4 + nCoefs * 44) throw SetupError("zkey: section 4 has the wrong size for its count");
  host_check_coords(hp + kAlpha1, 18, "zkey header points");

  const PtauRanges pt = read_ptau_ranges(ptau_path, cp);
  phase("ptau ranges read");
  if (memcmp(hp + kAlpha1, pt.alpha1, 64) || memcmp(hp + kBeta1, pt.beta1, 64) || memcmp(hp + kBeta2, pt.beta2, 128))
    failed |= ZKPOA_ZKEY_HEADER;
  uint8_t g1b[64], g2b[128];
  h_affine_to_bytes<HFq>(host_generator<HFq>(), g1b);
  h_affine_to_bytes<HFq2>(host_generator<HFq2>(), g2b);
  if (memcmp(hp + kGamma2, g2b, 128)) failed |= ZKPOA_ZKEY_HEADER;

  Lane& lane = ctx->dev.lanes[0];
  hipStream_t st = lane.stream;
  PointChecker points(ctx);
  uint32_t* fl = points.fl();   // words 2 and 4-5 take the fold kernels' flags, word 0 fold_compare_kernel's
  auto up_file = [&](void* dst, const Sec& sc, uint64_t at = 0) {
    if (sc.len) ctx->uploader.upload(static_cast<char*>(dst) + at, nullptr, sc.len, ctx->dev.device, st, fk.fd, sc.off);
  };
  auto msm = [&](int group, const void* d_pts, const void* d_sc, uint64_t count, uint8_t* out) {
    if (!count) {
      memset(out, 0, group == 1 ? 64 : 128);
      return;
    }
    if (group == 1) msm_run_g1(ctx, 0, d_pts, d_sc, count, out, nullptr);
    else msm_run_g2(ctx, 0, d_pts, d_sc, count, out, nullptr);
  };

  // ---- header points: on their curves, the G2 ones in G2, delta1 != O
  {
    DevBuf d(3 * 64 + 3 * 128);
    uint8_t hb[3 * 64 + 3 * 128];
    memcpy(hb, hp + kAlpha1, 64);
    memcpy(hb + 64, hp + kBeta1, 64);
    memcpy(hb + 128, hp + kDelta1, 64);
    memcpy(hb + 192, hp + kBeta2, 128);
    memcpy(hb + 320, hp + kGamma2, 128);
    memcpy(hb + 448, hp + kDelta2, 128);
    d.up(hb, sizeof hb);
    if (points.check(d.p, 3, 1, false, "zkey header points") | points.check((char*)d.p + 192, 3, 2, true, "zkey header points"))
      failed |= ZKPOA_ZKEY_POINTS;
    // the ptau's own alpha, beta: input from outside, curve-checked
    memcpy(hb, pt.alpha1, 64);
    memcpy(hb + 64, pt.beta1, 64);
    memcpy(hb + 192, pt.beta2, 128);
    d.up(hb, sizeof hb);
    if (points.check(d.p, 2, 1, false, "ptau alpha / beta") | points.check((char*)d.p + 192, 1, 2, false, "ptau alpha / beta"))
      throw SetupError("ptau: alpha*G1, beta*G1 or beta*G2 is not on its curve");
  }
  const pairing::G1 delta1 = h_affine_from_bytes<HFq>(hp + kDelta1);
  const pairing::G2 delta2 = h_affine_from_bytes<HFq2>(hp + kDelta2);
  if (delta1.is_inf()) failed |= ZKPOA_ZKEY_POINTS;
  // e(delta1, G2) == e(G1, delta2)
  if (delta1.is_inf() || delta2.is_inf() || !pairing::pair_eq(delta1, host_generator<HFq2>(), host_generator<HFq>(), delta2))
    failed |= ZKPOA_ZKEY_DELTA;

  // ---- random weights: rho (m) then sigma (n), back to back so that [rho_{l+1..m} | sigma] is one scalar range
  DevBuf d_rho((m + n) * 32);
  {
    UVec<uint8_t> rnd((m + n) * 32);
    parallel_ranges(m + n, 1u << 18, [&](unsigned, uint64_t lo, uint64_t hi) {
      urandom(rnd.data() + lo * 32, (hi - lo) * 32);
      for (uint64_t i = lo; i < hi; i++) rnd[i * 32 + 31] &= 0x1f;   // 253 bits: below r
    });
    d_rho.up(rnd.data(), rnd.size());
  }
  phase("random weights");

  // ---- folds from the r1cs: wtns_check_kernel with w := rho writes a, b, c (Montgomery) into rows [0, nC) of
  // d_S = [a | b | c | sigma]; the public rows nC + i of a are rho_i
  DevBuf d_S(4 * n * 32);
  ZK_HIP(hipMemsetAsync(d_S.p, 0, 3 * n * 32, st));
  {
    const R1csRows rows = r1cs_rows(r);
    const uint64_t nnz = rows.sig.size();
    DevBuf d_rp(rows.row_ptr.size() * 4), d_sig(nnz * 4), d_coef(nnz * 32), d_rho_m(m * 32);
    d_rp.up(rows.row_ptr.data(), rows.row_ptr.size() * 4);
    d_sig.up(rows.sig.data(), nnz * 4);
    d_coef.up(rows.coef.data(), nnz * 32);
    ZK_HIP(hipMemcpyAsync(d_rho_m.p, d_rho.p, m * 32, hipMemcpyDeviceToDevice, st));
    if (nnz) hipLaunchKernelGGL(fr_to_mont_kernel, dim3((uint32_t)((nnz + 255) / 256)), dim3(256), 0, st, d_coef.p, nnz, fl + 2);
    hipLaunchKernelGGL(fr_to_mont_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, st, d_rho_m.p, m, fl + 2);
    if (nC)
      hipLaunchKernelGGL(wtns_check_kernel, dim3((uint32_t)((nC + 255) / 256)), dim3(256), 0, st, (const uint32_t*)d_rp.p,
                         (const uint32_t*)d_sig.p, (const void*)d_coef.p, (const void*)d_rho_m.p, (uint32_t)nC, fl + 4,
                         d_S.p, (uint32_t)n);
    ZK_HIP(hipMemcpyAsync((char*)d_S.p + nC * 32, d_rho_m.p, (l + 1) * 32, hipMemcpyDeviceToDevice, st));
    ZK_HIP(hipMemcpyAsync((char*)d_S.p + 3 * n * 32, (char*)d_rho.p + m * 32, n * 32, hipMemcpyDeviceToDevice, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    (void)points.read();
  }
  // ---- folds from the key: section 4 through abc.hip.h's CSR (count, scan, scatter) and rows kernels with w := rho
  {
    DevBuf d_recs(nCoefs * 44), d_K(3 * n * 32);
    const Sec recs{ks[4].off + 4, nCoefs * 44};
    up_file(d_recs.p, recs);
    AbcCsr csr;
    abc_build_csr(st, d_recs.p, nCoefs, (uint32_t)n, (uint32_t)m, 0u, 0u, csr);
    if (csr.err & 2u) throw SetupError("zkey: a coefficient is not a field element (>= r)");
    if (csr.err) failed |= ZKPOA_ZKEY_COEFFS;   // a record's matrix, row or signal out of range (the record is left out)
    const uint32_t lgrid = (uint32_t)((n + 255) / 256);
    char* K = reinterpret_cast<char*>(d_K.p);
    hipLaunchKernelGGL(abc_rows_kernel, dim3(lgrid), dim3(256), 0, st, csr.row_ptr.as<const uint32_t>(), csr.sig.as<const uint32_t>(),
                       (const void*)csr.vals.get(), (const void*)d_rho.p, (uint32_t)n, 0u, 1u, (void*)K, (void*)(K + n * 32),
                       (void*)(K + 2 * n * 32));
    if (csr.n_long)   // the constraints too long for one lane: one wave each
      hipLaunchKernelGGL(abc_long_rows_kernel, dim3((csr.n_long + 3) / 4), dim3(256), 0, st, csr.row_ptr.as<const uint32_t>(),
                         csr.sig.as<const uint32_t>(), (const void*)csr.vals.get(), (const void*)d_rho.p,
                         csr.long_list.as<const uint32_t>(), csr.n_long, 0u, 0u, (void*)K, (void*)(K + n * 32),
                         (void*)(K + 2 * n * 32));
    hipLaunchKernelGGL(fold_compare_kernel, dim3(lgrid), dim3(256), 0, st, d_S.p, (const void*)K, (uint32_t)n, fl);
    if (points.read()) failed |= ZKPOA_ZKEY_COEFFS;
  }
  phase("folds (r1cs and section 4)");

  // ---- the ptau side: [bL | aL | L1 | Hodd] under [a | b | c | sigma]; L1 under a and b; L2 under b
  uint8_t q_icch[64], pA[64], pB1[64], pB2[128];
  {
    DevBuf dP(4 * n * 64);
    dP.up(pt.bL.data(), n * 64, 0);
    dP.up(pt.aL.data(), n * 64, n * 64);
    dP.up(pt.L1.data(), n * 64, 2 * n * 64);
    {
      DevBuf dH(2 * n * 64);
      dH.up(pt.Hs.data(), 2 * n * 64);
      hipLaunchKernelGGL(strided_copy64_kernel, dim3((uint32_t)((4 * n + 255) / 256)), dim3(256), 0, st,
                         (const uint4*)dH.p, (uint4*)((char*)dP.p + 3 * n * 64), n, 1u, 2u);
      ZK_HIP(hipStreamSynchronize(st));
    }
    if (points.check(dP.p, 4 * n, 1, false, "ptau (Lagrange)")) throw SetupError("ptau: a Lagrange-form point is not on the curve");
    const char* L1d = (const char*)dP.p + 2 * n * 64;
    msm(1, dP.p, d_S.p, 4 * n, q_icch);
    msm(1, L1d, d_S.p, n, pA);
    msm(1, L1d, (const char*)d_S.p + n * 32, n, pB1);
  }
  {
    DevBuf dL2(n * 128);
    dL2.up(pt.L2.data(), n * 128);
    if (points.check(dL2.p, n, 2, false, "ptau tau*G2 (Lagrange)")) throw SetupError("ptau: a Lagrange-form point is not on the curve");
    msm(2, dL2.p, (const char*)d_S.p + n * 32, n, pB2);
  }
  phase("ptau side (upload, checks, MSMs)");

  // ---- the key side, one section at a time
  uint8_t kA[64], kB1[64], kB2[128], kIC[64], kCH[64];
  uint32_t pf = 0;
  {
    DevBuf d(m * 64);
    up_file(d.p, ks[5]);
    pf |= points.check(d.p, m, 1, false, "zkey section 5");
    msm(1, d.p, d_rho.p, m, kA);
    up_file(d.p, ks[6]);
    pf |= points.check(d.p, m, 1, false, "zkey section 6");
    msm(1, d.p, d_rho.p, m, kB1);
  }
  {
    DevBuf d(m * 128);
    up_file(d.p, ks[7]);
    pf |= points.check(d.p, m, 2, true, "zkey section 7");
    msm(2, d.p, d_rho.p, m, kB2);
  }
  {
    DevBuf d((l + 1) * 64);
    up_file(d.p, ks[3]);
    pf |= points.check(d.p, l + 1, 1, false, "zkey section 3");
    msm(1, d.p, d_rho.p, l + 1, kIC);
  }
  {
    DevBuf d((m - l - 1 + n) * 64);   // C and H back to back, under [rho_{l+1..m} | sigma]
    up_file(d.p, ks[8]);
    up_file(d.p, ks[9], ks[8].len);
    pf |= points.check(d.p, m - l - 1 + n, 1, false, "zkey section 8 / 9");
    msm(1, d.p, (const char*)d_rho.p + (l + 1) * 32, m - l - 1 + n, kCH);
  }
  if (pf) failed |= ZKPOA_ZKEY_POINTS;
  phase("key side (upload, checks, MSMs)");
  if (memcmp(kA, pA, 64)) failed |= ZKPOA_ZKEY_A;
  if (memcmp(kB1, pB1, 64)) failed |= ZKPOA_ZKEY_B1;
  if (memcmp(kB2, pB2, 128)) failed |= ZKPOA_ZKEY_B2;
  {   // e(IC - Q, G2) == e(-CH, delta2)
    XYZZ<HFq> x = XYZZ<HFq>::from_affine(h_affine_from_bytes<HFq>(kIC));
    pairing::G1 q = h_affine_from_bytes<HFq>(q_icch), ch = h_affine_from_bytes<HFq>(kCH);
    q.y = q.y.neg();
    xyzz_add(x, XYZZ<HFq>::from_affine(q));
    ch.y = ch.y.neg();
    if (!pairing::pair_eq(h_to_affine(x), host_generator<HFq2>(), ch, delta2)) failed |= ZKPOA_ZKEY_ICCH;
  }
  phase("pairings");
  if (transcript) failed |= phase2_verify(ctx, r1cs_path, ptau_path, zkey_path);
  return failed;
}

}  // namespace

extern "C" int zkpoa_zkey_verify(zkpoa_context* ctx, const char* r1cs_path, const char* ptau_path, const char* zkey_path,
                                 uint32_t* failed_checks) {
  ZK_API_BEGIN(ctx)
  if (!r1cs_path || !ptau_path || !zkey_path || !failed_checks) throw SetupError("zkey verify: null argument");
  *failed_checks = zkey_verify(ctx, r1cs_path, ptau_path, zkey_path);
  ZK_API_END(ctx)
}

