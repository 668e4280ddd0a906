// NTT translation unit: kernels from ntt.hip.h + the C-ABI entry points zkpoa_ntt / zkpoa_ntt_device / zkpoa_ntt_form.
#include "ntt.hip.h"
#include "zkpoa_internal.hpp"

namespace zkpoa {

static NttEngine* engine(zkpoa_context* ctx) {
  if (!ctx->ntt) ctx->ntt = new NttEngine();
  return ctx->ntt;
}

void ntt_prepare(zkpoa_context* ctx, hipStream_t st, uint32_t k) { (void)engine(ctx)->size(st, k); }
void ntt_to_odd_coset(zkpoa_context* ctx, hipStream_t st, void* d_data, uint32_t k, uint32_t batch, size_t stride) {
  engine(ctx)->to_odd_coset(st, d_data, k, batch, stride);
}
void ntt_natural(zkpoa_context* ctx, hipStream_t st, void* d_data, uint32_t k, bool inverse) {
  NttEngine* e = engine(ctx);
  e->run(st, e->size(st, k), kNttNatural, inverse, d_data);
}
void ntt_dif(zkpoa_context* ctx, hipStream_t st, void* d_data, uint32_t k, bool inverse, uint32_t batch, size_t stride) {
  NttEngine* e = engine(ctx);
  e->run(st, e->size(st, k), kNttDif, inverse, d_data, batch, stride);
}
void ntt_dit(zkpoa_context* ctx, hipStream_t st, void* d_data, uint32_t k, bool inverse, uint32_t batch, size_t stride) {
  NttEngine* e = engine(ctx);
  e->run(st, e->size(st, k), kNttDit, inverse, d_data, batch, stride);
}
void ntt_split_mid(zkpoa_context* ctx, hipStream_t st, const void* in, void* out, uint32_t k, uint32_t G, uint32_t h,
                   uint32_t rank_stride) {
  engine(ctx)->split_mid(st, in, out, k, G, h, rank_stride);
}
void ntt_release(zkpoa_context* ctx) {   // the engine's members free their device memory
  delete ctx->ntt;
  ctx->ntt = nullptr;
}

}  // namespace zkpoa
using namespace zkpoa;

extern "C" int zkpoa_ntt_device(zkpoa_context* ctx, void* d_data, unsigned log_n, int inverse) {
  ZK_API_BEGIN(ctx)
  if (log_n > 28) throw HipError("ntt: log_n > 28 (two-adicity of Fr)");
  hipStream_t st = ctx->dev.lanes[0].stream;
  ntt_prepare(ctx, st, log_n);
  timed(ctx, st, kMsNtt, [&] { ntt_natural(ctx, st, d_data, log_n, inverse != 0); });
  ZK_API_END(ctx)
}

extern "C" int zkpoa_ntt(zkpoa_context* ctx, void* data, unsigned log_n, int inverse) {
  ZK_API_BEGIN(ctx)
  if (log_n > 28) throw HipError("ntt: log_n > 28 (two-adicity of Fr)");
  LaneInOut d(data, 32, 1ull << log_n);
  int rc = zkpoa_ntt_device(ctx, d.at<void>(0), log_n, inverse);
  if (rc != PROVER_OK) return rc;
  d.down();
  ZK_API_END(ctx)
}

// The forms the prover and the split chain run (zkpoa_ntt reaches the natural-order form only), on a host buffer.
extern "C" int zkpoa_ntt_form(zkpoa_context* ctx, void* data, unsigned log_n, int form, int inverse, unsigned batch,
                              uint64_t stride) {
  ZK_API_BEGIN(ctx)
  if (log_n > 28) throw HipError("ntt_form: log_n > 28 (two-adicity of Fr)");
  if (form < 0 || form > 2) throw HipError("ntt_form: form is 0 (dif), 1 (dit) or 2 (to_odd_coset)");
  if (batch == 0 || batch > 65535) throw HipError("ntt_form: batch is 1..65535 (grid.y)");
  const uint64_t n = 1ull << log_n;
  if (stride < n) throw HipError("ntt_form: stride < 2^log_n");
  LaneInOut d(data, 32, (batch - 1) * stride + n);
  void* dp = d.at<void>(0);
  hipStream_t st = ctx->dev.lanes[0].stream;
  ntt_prepare(ctx, st, log_n);
  if (form == 0) ntt_dif(ctx, st, dp, log_n, inverse != 0, batch, (size_t)stride * 32);
  else if (form == 1) ntt_dit(ctx, st, dp, log_n, inverse != 0, batch, (size_t)stride * 32);
  else ntt_to_odd_coset(ctx, st, dp, log_n, batch, (size_t)stride * 32);
  finish(st);
  d.down();
  ZK_API_END(ctx)
}

// Test hook, no context and no GPU: the pass plan of a size-2^log_n transform, seven words per pass (s_lo, B, logT,
// grid.x, threads, dynamic LDS bytes, direct table 0/1). tile_log 0 = the tile the size takes by default, 10 / 11 = that
// tile. Returns the pass count (the first `cap` words' worth are written), -1 for arguments out of range.
extern "C" int zkpoa_test_ntt_plan(unsigned log_n, unsigned tile_log, uint32_t* out, unsigned cap) {
  if (log_n > 28 || (tile_log != 0 && tile_log != 10 && tile_log != 11)) return -1;
  const auto plan = ntt_plan(log_n, tile_log ? tile_log : ntt_tile_log_by_size(log_n));
  for (size_t i = 0; i < plan.size() && 7 * (i + 1) <= cap; i++) {
    const NttPass& ps = plan[i];
    const uint32_t w[7] = {ps.s_lo, ps.B, ps.logT, ps.grid, ps.threads, ps.lds_bytes, ps.direct ? 1u : 0u};
    memcpy(out + 7 * i, w, sizeof w);
  }
  return (int)plan.size();
}
