// G1 instantiation of the per-point scalar multiplication (ptau sections 2, 4, 5).
#include "ptau_contribute.hip.h"

namespace zkpoa {
size_t scalar_mul_each_scratch_g1(uint64_t n, uint64_t slab) { return scalar_mul_each_scratch_bytes<Fq>(n, slab ? slab : kMulEachSlab); }
void scalar_mul_each_g1(zkpoa_context* ctx, const void* d_points, const void* d_scalars, uint64_t n, void* d_out, uint32_t* d_flags,
                        void* d_scratch, uint64_t slab) {
  scalar_mul_each<Fq>(ctx->dev.lanes[0].stream, d_points, d_scalars, n, d_out, d_flags, d_scratch, slab);
}
}  // namespace zkpoa
