// G2 instantiation of the per-point scalar multiplication (ptau sections 3 and 6).
#include "ptau_contribute.hip.h"

namespace zkpoa {
size_t scalar_mul_each_scratch_g2(uint64_t n, uint64_t slab) { return scalar_mul_each_scratch_bytes<Fq2>(n, slab ? slab : kMulEachSlab); }
void scalar_mul_each_g2(zkpoa_context* ctx, const void* d_points, const void* d_scalars, uint64_t n, void* d_out, uint32_t* d_flags,
                        void* d_scratch, uint64_t slab) {
  scalar_mul_each<Fq2>(ctx->dev.lanes[0].stream, d_points, d_scalars, n, d_out, d_flags, d_scratch, slab);
}
}  // namespace zkpoa
