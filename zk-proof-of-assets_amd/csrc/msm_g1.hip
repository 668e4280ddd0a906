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
void msm_table_release(MsmTable* t) { delete t; }
const void* msm_table_data(const MsmTable* t) { return t ? t->d.get() : nullptr; }
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
size_t msm_workspace(const MsmRequest& req, unsigned parts, bool guard) {   // (layouts only: no G2 kernel is instantiated here)
  if (req.n == 0) return 0;
  const MsmPlan p = msm_make_plan(req);
  return (parts & kMsmSort ? msm_sort_workspace_bytes(p, guard) : 0) + (parts & kMsmAccumG1 ? msm_accum_workspace_bytes<Fq>(p, guard) : 0) +
         (parts & kMsmAccumG2 ? msm_accum_workspace_bytes<Fq2>(p, guard) : 0);
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

// the thirteen words the test hooks below report of a plan (and of the request it was made from); the sizes are those
// of the unguarded arena, whatever ZKPOA_WS_GUARD says
static void plan_words(const zkpoa::MsmPlan& p, uint64_t w[13]) {
  using namespace zkpoa;
  const uint64_t v[13] = {p.c, p.W, p.Wb, p.ne, p.TB, p.K0, p.K, p.logS, p.logRows, p.sparse ? 1u : 0u,
                          msm_workspace(p.req, kMsmSort, false), msm_workspace(p.req, kMsmAccumG1, false), msm_workspace(p.req, kMsmAccumG2, false)};
  for (int i = 0; i < 13; i++) w[i] = v[i];
}

// Test hook, no context, no GPU, no environment variable: the plan of one request and the workspace its parts take.
// Thirteen words: c, W, Wb, ne, TB, K0, K, logS, logRows; sparse; bytes of the sort, of the G1 and of the G2 accumulation
// (0 for n == 0). density: null or 32 doubles indexed by the window width. Returns 13 (the first `cap` words are written),
// -1 for arguments out of range.
extern "C" int zkpoa_test_msm_plan(uint64_t n, int c, int merged, int for_g2, const double* density32_or_null, int k0,
                                   uint64_t* out, unsigned cap) {
  using namespace zkpoa;
  if (n > (1ull << 28) || c < 0 || c > 31 || (merged | for_g2) >> 1 || k0 < 0 || (!out && cap)) return -1;
  const MsmPlan p = msm_make_plan(MsmRequest{n, c, merged != 0, for_g2 != 0, density32_or_null, k0});
  uint64_t w[13];
  plan_words(p, w);
  for (unsigned i = 0; i < 13 && i < cap; i++) out[i] = w[i];
  return 13;
}

// Test hook: phase A of one request on host scalars, through msm_sort_run (the prover's own entry: no second copy of the
// launch sequence), and what it hands phase B copied back. The arrays are checked against their capacities before any
// of them is written. len_hist is read AFTER the piece ordering: msm_piece_order_kernel only reads the histogram (its
// cursors are an array of their own, MsmSortLayout::len_cursor), so these are the words the scan left.
extern "C" int zkpoa_test_msm_sort(zkpoa_context* ctx, int lane, const void* scalars, uint64_t n, int c, int merged, int for_g2,
                                   const double* density32_or_null, int k0, uint64_t plan[13], uint32_t totals[3],
                                   uint32_t* const out[7], const uint64_t cap[7]) {
  using namespace zkpoa;
  if (!ctx || lane < 0 || lane >= DeviceCtx::kLanes || n > (1ull << 28) || c < 0 || c > 31 || (merged | for_g2) >> 1 || k0 < 0 ||
      (n && !scalars) || !plan || !totals || !out || !cap)
    return PROVER_ERROR;
  try {
    ZK_HIP(hipSetDevice(ctx->dev.device));
    if (lane) ctx->dev.wait_lanes();
    ctx->dev.ensure_lane(lane);
    const MsmRequest req{n, c, merged != 0, for_g2 != 0, density32_or_null, k0};
    DevBuf ds(n * 32);
    ds.up(scalars, n * 32);
    const std::unique_ptr<MsmSorted> sr = msm_sort_run(ctx, lane, ds.p, req);   // (synchronised on return)
    const MsmPlan& p = sr->p;
    const MsmSortLayout& m = sr->m;
    plan_words(p, plan);   // of the plan that ran
    totals[0] = sr->total_entries;
    totals[1] = sr->max_count;
    totals[2] = sr->total1;
    const struct {
      const uint32_t* d;
      uint64_t count;
    } parts[7] = {{m.counts, p.TB},           {m.off0, (uint64_t)p.TB + 1}, {m.po_a, (uint64_t)p.TB + 1}, {m.sorted, sr->total_entries},
                  {m.pbkt, sr->total1},       {m.order, sr->total1},        {m.len_hist, (uint64_t)p.K0 + 1}};
    for (int i = 0; i < 7; i++)
      if (cap[i] < parts[i].count || (parts[i].count && !out[i])) return PROVER_ERROR_SHORT_BUFFER;
    for (int i = 0; i < 7; i++)
      if (parts[i].count) ZK_HIP(hipMemcpy(out[i], parts[i].d, parts[i].count * 4, hipMemcpyDeviceToHost));
  } catch (const std::exception& e) {
    return PROVER_ERROR;   // last_error is shared between lanes: not touched
  }
  return PROVER_OK;
}

// Test hook: msm_density (the prover's measurement of a witness) on host scalars, on lane 0's stream.
extern "C" int zkpoa_test_msm_density(zkpoa_context* ctx, const void* scalars, uint64_t n, double out[32]) {
  using namespace zkpoa;
  ZK_API_BEGIN(ctx)
  if (n > (1ull << 28) || (n && !scalars) || !out) throw std::runtime_error("zkpoa_test_msm_density: arguments out of range");
  DevBuf ds(n * 32), scratch(32 * 8);
  ds.up(scalars, n * 32);
  msm_density(ctx->dev.lanes[0].stream, ds.p, n, out, scratch.p);
  ZK_API_END(ctx)
}
