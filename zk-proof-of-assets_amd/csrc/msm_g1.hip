// G1 instantiation of the Pippenger MSM (zkey sections 5, 6, 8, 9: A, B1, C, H queries).
#include "msm_run.hip.h"

namespace zkpoa {
void msm_run_g1(zkpoa_context* ctx, int lane_id, const void* d_bases, const void* d_scalars, uint64_t n, uint8_t* out,
                float* ms2, const MsmTable* table, const double* density) {
  msm_run<Fq, HFq>(ctx, lane_id, d_bases, d_scalars, n, out, ms2, table, density);
}
MsmTablePtr msm_table_build_g1(zkpoa_context* ctx, const void* d_bases, uint64_t n, int c) {
  MsmTablePtr t(new MsmTable());
  *t = msm_table_build<Fq>(ctx->dev.lanes[0].stream, d_bases, n, msm_table_c(n, c, false));
  return t;
}
size_t msm_table_bytes_g1(uint64_t n, int c) { return msm_table_bytes<Fq>(n, msm_table_c(n, c, false)); }
void msm_table_release(MsmTable* t) {
  if (!t) return;
  msm_table_free(*t);
  delete t;
}
const void* msm_table_data(const MsmTable* t) { return t ? t->d : nullptr; }
void msm_density(hipStream_t st, const void* d_scalars, uint64_t n, double out[32], void* d_scratch) {
  for (int c = 0; c < 32; c++) out[c] = (double)msm_windows(c < 4 ? 4u : (uint32_t)c);   // uniform default
  if (n == 0) return;
  unsigned long long h[kDensityHi - kDensityLo + 1];
  ZK_HIP(hipMemsetAsync(d_scratch, 0, 32 * 8, st));
  hipLaunchKernelGGL(msm_density_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, d_scalars, n,
                     (unsigned long long*)d_scratch);
  ZK_HIP(hipMemcpyAsync(h, d_scratch, sizeof(h), hipMemcpyDeviceToHost, st));
  ZK_HIP(hipStreamSynchronize(st));
  for (int c = kDensityLo; c <= kDensityHi; c++) out[c] = (double)h[c - kDensityLo] / (double)n;
}
size_t msm_workspace(const MsmRequest& req, unsigned parts) {   // (layouts only: no G2 kernel is instantiated here)
  if (req.n == 0) return 0;
  const MsmPlan p = msm_make_plan(req);
  return (parts & kMsmSort ? msm_sort_workspace_bytes(p) : 0) + (parts & kMsmAccumG1 ? msm_accum_workspace_bytes<Fq>(p) : 0) +
         (parts & kMsmAccumG2 ? msm_accum_workspace_bytes<Fq2>(p) : 0);
}
void msm_table_info(const MsmTable* t, uint64_t out[4]) {
  out[0] = t->n;
  out[1] = t->c;
  out[2] = t->W;
  out[3] = t->bytes;
}
std::unique_ptr<MsmSorted> msm_sort_run(zkpoa_context* ctx, int lane_id, const void* d_scalars, const MsmRequest& req) {
  if (lane_id) ctx->dev.wait_lanes();
  // the sorting lane also accumulates a G1 array afterwards: reserve room for that in the same arena
  return std::make_unique<MsmSorted>(msm_sort_phase(ctx->dev.lanes[lane_id], d_scalars, req, &msm_accum_workspace_bytes<Fq>, true));
}
void msm_accum_g1(zkpoa_context* ctx, int lane_id, const MsmSorted* sr, bool own_arena, const void* d_bases,
                  uint8_t* out, float* ms2) {
  msm_accum_run<Fq, HFq>(ctx, lane_id, *sr, own_arena, d_bases, out, ms2);
}
}  // namespace zkpoa

// Test hook, no context, no GPU, no environment variable: the plan of one request and the workspace its parts take.
// Thirteen words: c, W, Wb, ne, TB, K0, K, logS, logRows; sparse; bytes of the sort, of the G1 and of the G2 accumulation
// (0 for n == 0). density: null or 32 doubles indexed by the window width. Returns 13 (the first `cap` words are written),
// -1 for arguments out of range.
extern "C" int zkpoa_test_msm_plan(uint64_t n, int c, int merged, int for_g2, const double* density32_or_null, int k0,
                                   uint64_t* out, unsigned cap) {
  using namespace zkpoa;
  if (n > (1ull << 28) || c < 0 || c > 31 || (merged | for_g2) >> 1 || k0 < 0 || (!out && cap)) return -1;
  const MsmRequest req{n, c, merged != 0, for_g2 != 0, density32_or_null, k0};
  const MsmPlan p = msm_make_plan(req);
  const uint64_t w[13] = {p.c, p.W, p.Wb, p.ne, p.TB, p.K0, p.K, p.logS, p.logRows, p.sparse ? 1u : 0u,
                          msm_workspace(req, kMsmSort), msm_workspace(req, kMsmAccumG1), msm_workspace(req, kMsmAccumG2)};
  for (unsigned i = 0; i < 13 && i < cap; i++) out[i] = w[i];
  return 13;
}
