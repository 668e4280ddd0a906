// G1 instantiation of the inverse NTT over curve points (ptau sections 12, 14, 15).
#include "ec_ntt.hip.h"

namespace zkpoa {
EcNttWork* ec_intt_work_g1(zkpoa_context* ctx, uint32_t log_max) { return ec_intt_work<Fq>(ctx, log_max); }
void ec_intt_g1(zkpoa_context* ctx, EcNttWork& wk, const void* d_in, uint32_t log_n, void* d_out) {
  ec_intt_run<Fq>(ctx->dev.lanes[0].stream, wk, d_in, log_n, d_out);
}
}  // namespace zkpoa
