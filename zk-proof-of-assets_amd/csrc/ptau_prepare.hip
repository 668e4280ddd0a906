// `snarkjs powersoftau prepare phase2 <in.ptau> <out.ptau>` on the device: the Lagrange-form sections 12-15 (what `zkey
// new` reads, what `zkey verify` and `powersoftau verify` check against) made from the powers of a ceremony file.
//
// snarkjs ptau layout, power p, N = 2^p (as csrc/ptau_verify.hip): level l of an output section starts at point 2^l - 1
// and is the inverse NTT (csrc/ec_ntt.hip.h) of the first 2^l points of its source section:
//   12 <- 2 (tau^i G1), levels 0..p+1; the top level takes the section's 2N - 1 points and one point at infinity
//   13 <- 3 (tau^i G2), 14 <- 4 (alpha tau^i G1), 15 <- 5 (beta tau^i G1), levels 0..p
// The file is validated as `powersoftau verify` validates it (header, section lengths, every point on its curve and in
// range, sections 3 and 6 in G2); what that command checks with pairings (one tau, alpha, beta) is not repeated here.
// A source section is uploaded once, its levels run one after the other into one device copy of the output section,
// which comes back in one piece. A level whose buffers do not fit in free HBM is an error before anything is written:
// streaming a level through HBM in pieces is not done. Sections 1-7 are copied byte for byte, sections 12-15 of the
// input, if any, are ignored; the output (csrc/setup_common.hip.h: SectionFile, 11 sections in the order 1-7, 12-15)
// appears under its name only when it is complete.
#include "ptau_file.hip.h"
#include "zkpoa_internal.hpp"

#include <memory>

using namespace zkpoa;

namespace {

void ptau_prepare(zkpoa_context* ctx, const char* in_path, const char* out_path, uint32_t info[4]) {
  PhaseTimer phase("powersoftau prepare phase2", 34);
  if (same_file(in_path, out_path)) throw SetupError("powersoftau prepare phase2: the output path names the input file");
  PtauInput in(in_path, false, true);   // section 7 is copied unread; the power is checked before the lengths
  auto& [fp, ps, shape, records] = in;
  const uint32_t p = shape.power;
  info[0] = p;
  info[1] = shape.ceremony;
  info[2] = in.lagrange() == PtauInput::kAll ? 1 : 0;
  info[3] = shape.contributions;
  const auto jobs = ptau_lagrange_secs(p);
  auto src_bytes = [](const LagrangeSec& j) { return j.unit() << j.top; };   // section 2: with its infinity
  {
    size_t free_b = 0, total_b = 0, need = 0;
    ZK_HIP(hipMemGetInfo(&free_b, &total_b));
    for (const auto& j : jobs) need = std::max<size_t>(need, src_bytes(j) + j.bytes() + ec_intt_work_bytes(j.group, j.top));
    need += 64u << 20;   // flags, the allocator's granularity
    if (need > free_b)
      throw SetupError("powersoftau prepare phase2: power " + std::to_string(p) + " needs " + std::to_string(need >> 20) +
                       " MiB of device memory for its largest level, " + std::to_string(free_b >> 20) +
                       " MiB are free (a level is not streamed through the device in pieces)");
  }
  phase("sections");

  hipStream_t st = ctx->dev.lanes[0].stream;
  PointChecker points(ctx);
  auto checked = [&](const void* d, uint64_t count, int group, bool subgroup, uint32_t sec) {
    points.require(d, count, group, subgroup, ("ptau section " + std::to_string(sec)).c_str());
  };
  {
    DevBuf beta2(128);
    beta2.up(fp.p + ps[6].off, 128);
    checked(beta2.p, 1, 2, true, 6);
  }
  UVec<uint8_t> out[4];
  for (int t = 0; t < 4; t++) {
    const LagrangeSec& j = jobs[t];
    const uint64_t have = ps[j.src].len;   // (2N - 1) * 64 for section 2: one point short of the top level
    DevBuf src(src_bytes(j)), dst(j.bytes());
    ctx->uploader.upload(src.p, nullptr, have, ctx->dev.device, st, fp.fd, ps[j.src].off);
    if (have < src_bytes(j)) ZK_HIP(hipMemsetAsync(static_cast<char*>(src.p) + have, 0, src_bytes(j) - have, st));
    checked(src.p, have / j.unit(), j.group, j.group == 2, j.src);
    std::unique_ptr<EcNttWork> wk(j.group == 2 ? ec_intt_work_g2(ctx, j.top) : ec_intt_work_g1(ctx, j.top));
    for (uint32_t l = 0; l <= j.top; l++) {
      void* to = static_cast<char*>(dst.p) + j.unit() * ((1ull << l) - 1);
      if (j.group == 2) ec_intt_g2(ctx, *wk, src.p, l, to);
      else ec_intt_g1(ctx, *wk, src.p, l, to);
    }
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    if (phase.verbose) phase(("section " + std::to_string(j.dst) + " (upload, point checks, iNTT)").c_str());
    out[t].alloc(j.bytes());
    ZK_HIP(hipMemcpy(out[t].data(), dst.p, j.bytes(), hipMemcpyDeviceToHost));
    if (phase.verbose) phase(("section " + std::to_string(j.dst) + " (download)").c_str());
  }

  uint32_t ids[11];   // sections 1-7 as they are, then 12-15
  uint64_t lens[11];
  for (uint32_t t = 0; t < 11; t++) {
    ids[t] = t < 7 ? t + 1 : jobs[t - 7].dst;
    lens[t] = t < 7 ? ps[ids[t]].len : out[t - 7].size();
  }
  SectionFile fo(out_path, "ptau", ids, lens, 11);
  for (uint32_t t = 1; t <= 7; t++) fo.put(t, fp.p + ps[t].off, ps[t].len);
  for (int t = 0; t < 4; t++) fo.put(jobs[t].dst, out[t].data(), out[t].size());
  fo.commit();
  phase("write");
}

}  // namespace

extern "C" int zkpoa_ec_intt_device(zkpoa_context* ctx, int group, const void* d_in, uint32_t log_n, void* d_out) {
  ZK_API_BEGIN(ctx)
  if (!d_in || !d_out) throw HipError("ec_intt: null pointer");
  if (group != 1 && group != 2) throw HipError("ec_intt: group must be 1 (G1) or 2 (G2)");
  if (log_n > 28) throw HipError("ec_intt: more than 2^28 points (BN254's Fr has no root of unity of that order)");
  std::unique_ptr<EcNttWork> wk(group == 2 ? ec_intt_work_g2(ctx, log_n) : ec_intt_work_g1(ctx, log_n));
  if (group == 2) ec_intt_g2(ctx, *wk, d_in, log_n, d_out);
  else ec_intt_g1(ctx, *wk, d_in, log_n, d_out);
  finish(ctx->dev.lanes[0].stream);
  ZK_API_END(ctx)
}

extern "C" int zkpoa_ptau_prepare_phase2(zkpoa_context* ctx, const char* in_path, const char* out_path, uint32_t info[4]) {
  ZK_API_BEGIN(ctx)
  if (!in_path || !out_path || !info) throw SetupError("powersoftau prepare phase2: null argument");
  uint32_t inf[4] = {0, 0, 0, 0};
  ptau_prepare(ctx, in_path, out_path, inf);
  memcpy(info, inf, sizeof inf);
  ZK_API_END(ctx)
}
