// Device side of the phase-2 transcript (DESIGN.md "Phase-2 transcript"): the points a circuit hash covers are in HBM
// where `zkey new` makes them and `zkey verify` checks them, so their hash form is made there and streamed to the one
// serial Blake2b on the host; the H part of the hash (tau^(i+n) G1 - tau^i G1) is a point subtraction over ptau section 2.
#pragma once
#include "phase2.hpp"
#include "setup_common.hip.h"

#include <functional>

namespace {

// Wire form -> hash form. One lane per 32-byte coordinate (two 16 B loads, two 16 B stores): out of Montgomery form,
// canonical, bytes reversed. K = 2 (G1: x, y) or 4 (G2: x.c0, x.c1, y.c0, y.c1 -> x.c1, x.c0, y.c1, y.c0) lanes make a
// point; a point whose coordinates are all zero is infinity: 0x40 then zeros. count = coordinates = K * points.
template <int K>
static __global__ __launch_bounds__(256) void hash_form_kernel(const uint4* __restrict__ in, uint4* __restrict__ out,
                                                               uint64_t count) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const bool live = i < count;   // (no early return: the lanes of a point exchange their zero test below)
  Fq v = Fq::zero();
  if (live) v = load_fp<FqParams>(in + 2 * i);
  uint32_t nz = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) nz |= v.l[k];
  nz |= __shfl_xor(nz, 1);
  if (K == 4) nz |= __shfl_xor(nz, 2);
  if (!live) return;
  const Fq s = v.from_mont().canon();
  const uint64_t o = K == 4 ? (i ^ 1ull) : i;
  uint4 hi = make_uint4(__builtin_bswap32(s.l[7]), __builtin_bswap32(s.l[6]), __builtin_bswap32(s.l[5]), __builtin_bswap32(s.l[4]));
  const uint4 lo = make_uint4(__builtin_bswap32(s.l[3]), __builtin_bswap32(s.l[2]), __builtin_bswap32(s.l[1]), __builtin_bswap32(s.l[0]));
  if (!nz && (o & (K - 1)) == 0) hi.x = 0x40u;   // the point's first byte
  out[2 * o] = hi;
  out[2 * o + 1] = lo;
}

// Wire form -> compressed form (DESIGN.md "Phase-1 transcript": what a contribution's response hash covers). One lane
// per point: x alone, big-endian standard form (G2: c1 then c0), bit 7 of the first byte set when y is the negative
// root (standard form above (q - 1) / 2; for Fq2 the sign of c1, of c0 when c1 = 0 -- the sign rule of `fromRng`), a point
// whose coordinates are all zero is infinity: 0x40 then zeros. q < 2^254 leaves both bits free.
ZK_DEV bool fq_std_negative(const Fq& s) {   // s: standard form, canonical
  constexpr uint32_t kHalfQ[8] = {0x6c3e7ea3u, 0x9e10460bu, 0xb438e546u, 0xcbc0b548u,
                                  0x40c0ac2eu, 0xdc2822dbu, 0x7098d014u, 0x18322739u};
  uint32_t bw = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) (void)subb(kHalfQ[k], s.l[k], bw);
  return bw != 0;
}
ZK_DEV bool fq_std_zero(const Fq& s) {
  uint32_t nz = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) nz |= s.l[k];
  return nz == 0;
}
ZK_DEV void store_be(uint4* out, const Fq& s, uint32_t flag) {
  out[0] = make_uint4(__builtin_bswap32(s.l[7]) | flag, __builtin_bswap32(s.l[6]), __builtin_bswap32(s.l[5]), __builtin_bswap32(s.l[4]));
  out[1] = make_uint4(__builtin_bswap32(s.l[3]), __builtin_bswap32(s.l[2]), __builtin_bswap32(s.l[1]), __builtin_bswap32(s.l[0]));
}
template <class F>
static __global__ __launch_bounds__(256) void compressed_form_kernel(const void* __restrict__ in, uint4* __restrict__ out,
                                                                     uint64_t count) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= count) return;
  const Affine<F> p = load_affine<F>(in, i);
  if constexpr (std::is_same<F, Fq>::value) {
    const Fq x = p.x.from_mont().canon(), y = p.y.from_mont().canon();
    const bool inf = fq_std_zero(x) && fq_std_zero(y);
    store_be(out + 2 * i, x, inf ? 0x40u : (fq_std_negative(y) ? 0x80u : 0u));
  } else {
    const Fq x0 = p.x.c0.from_mont().canon(), x1 = p.x.c1.from_mont().canon();
    const Fq y0 = p.y.c0.from_mont().canon(), y1 = p.y.c1.from_mont().canon();
    const bool inf = fq_std_zero(x0) && fq_std_zero(x1) && fq_std_zero(y0) && fq_std_zero(y1);
    const bool neg = fq_std_zero(y1) ? fq_std_negative(y0) : fq_std_negative(y1);
    store_be(out + 4 * i, x1, inf ? 0x40u : (neg ? 0x80u : 0u));
    store_be(out + 4 * i + 2, x0, 0u);
  }
}

// out[i] = T[i + n] - T[i], i < count (count = n - 1), affine wire form in and out. Thread t takes the points
// t, t + threads, ... (kBatch of them, coalesced across the wave) and divides their slopes with ONE inversion
// (Montgomery's trick over the lane's batch). Exceptional cases: either operand at infinity, T[i+n] = T[i] (result
// infinity), T[i+n] = -T[i] (a doubling; infinity when y = 0).
constexpr int kHDiffBatch = 8;
static __global__ __launch_bounds__(256) void h_diff_kernel(const void* __restrict__ T, uint64_t n, uint64_t count,
                                                            void* __restrict__ out) {
  const uint64_t threads = (uint64_t)gridDim.x * 256u, t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  Fq x1[kHDiffBatch], y1[kHDiffBatch], x2[kHDiffBatch], num[kHDiffBatch], den[kHDiffBatch], pre[kHDiffBatch];
  uint32_t kind[kHDiffBatch];   // 0 slope, 1 result infinity, 2 result = operand (x1, y1), 3 not a point of this thread
  Fq acc = Fq::one();
#pragma unroll
  for (int k = 0; k < kHDiffBatch; k++) {
    const uint64_t i = t + (uint64_t)k * threads;
    kind[k] = 3;
    den[k] = Fq::one();
    if (i < count) {
      const Affine<Fq> a = load_affine<Fq>(T, i + n);
      Affine<Fq> b = load_affine<Fq>(T, i);
      b.y = b.y.neg();
      x1[k] = a.x;
      y1[k] = a.y;
      x2[k] = b.x;
      if (b.is_inf()) kind[k] = 2;
      else if (a.is_inf()) {
        kind[k] = 2;
        x1[k] = b.x;
        y1[k] = b.y;
      } else if (a.x == b.x) {
        if (a.y == b.y && !a.y.is_zero()) {
          kind[k] = 0;
          const Fq xx = a.x.sqr();
          num[k] = xx.dbl() + xx;
          den[k] = a.y.dbl();
        } else kind[k] = 1;
      } else {
        kind[k] = 0;
        num[k] = b.y - a.y;
        den[k] = b.x - a.x;
      }
    }
    pre[k] = acc;
    acc = acc * den[k];
  }
  Fq inv = acc.inv();
#pragma unroll
  for (int k = kHDiffBatch - 1; k >= 0; k--) {
    const Fq dinv = inv * pre[k];
    inv = inv * den[k];
    if (kind[k] == 3) continue;
    char* o = reinterpret_cast<char*>(out) + 64 * (t + (uint64_t)k * threads);
    Fq x3 = Fq::zero(), y3 = Fq::zero();
    if (kind[k] == 2) {
      x3 = x1[k];
      y3 = y1[k];
    } else if (kind[k] == 0) {
      const Fq lam = num[k] * dinv;
      x3 = lam.sqr() - x1[k] - x2[k];
      y3 = lam * (x1[k] - x3) - y1[k];
    }
    store_field(o, x3);
    store_field(o + 32, y3);
  }
}

// The serial Blake2b over device-resident points: the device converts piece i + 1 into one pinned buffer while the host
// hashes piece i out of the other. Hash order is the points' order, whatever the piece size.
struct HashStream {
  zkpoa_context* ctx;
  zkpoa::phase2::Blake2b& hasher;
  uint64_t piece_bytes;
  PinnedMem pinned[2];
  DevMem d_stage[2];
  DevEvent ev[2];
  double convert_ms = 0, hash_ms = 0;   // host clock: waiting for the device's pieces; hashing
  uint64_t bytes = 0;
  std::vector<uint8_t>* capture = nullptr;   // tests: the hash-form bytes as well
  std::function<void(const uint8_t*, uint64_t)> sink;   // a command that also writes what it hashes: each piece, in order
  HashStream(zkpoa_context* c, zkpoa::phase2::Blake2b& h, uint64_t piece_points) : ctx(c), hasher(h) {
    if (!piece_points) piece_points = 1ull << 18;
    piece_bytes = piece_points * 128;   // a piece holds piece_points G2 points, or twice as many G1 points
    for (int b = 0; b < 2; b++) {
      pinned[b].alloc(piece_bytes);
      d_stage[b].alloc(piece_bytes);
      ev[b].create(hipEventDisableTiming);
    }
  }
  HashStream(const HashStream&) = delete;
  HashStream& operator=(const HashStream&) = delete;
  // `count` points of group 1 / 2 at d (wire form), preceded by their big-endian count when with_count; compressed: the
  // compressed form (half the bytes) instead of the hash form
  void points(const void* d, uint64_t count, int group, bool with_count, bool compressed = false) {
    if (with_count) hasher.update_u32_be((uint32_t)count);
    const uint64_t in_unit = group == 1 ? 64 : 128, unit = compressed ? in_unit / 2 : in_unit, per_piece = piece_bytes / in_unit;
    hipStream_t st = ctx->dev.lanes[0].stream;
    auto issue = [&](uint64_t first, int b) {
      const uint64_t cnt = std::min(per_piece, count - first), coords = cnt * (in_unit / 32);
      const uint4* src = reinterpret_cast<const uint4*>(static_cast<const char*>(d) + first * in_unit);
      const dim3 grid((uint32_t)((coords + 255) / 256)), pgrid((uint32_t)((cnt + 255) / 256));
      if (compressed && group == 1) hipLaunchKernelGGL((compressed_form_kernel<Fq>), pgrid, dim3(256), 0, st, (const void*)src, d_stage[b].as<uint4>(), cnt);
      else if (compressed) hipLaunchKernelGGL((compressed_form_kernel<Fq2>), pgrid, dim3(256), 0, st, (const void*)src, d_stage[b].as<uint4>(), cnt);
      else if (group == 1) hipLaunchKernelGGL((hash_form_kernel<2>), grid, dim3(256), 0, st, src, d_stage[b].as<uint4>(), coords);
      else hipLaunchKernelGGL((hash_form_kernel<4>), grid, dim3(256), 0, st, src, d_stage[b].as<uint4>(), coords);
      ZK_HIP(hipMemcpyAsync(pinned[b].get(), d_stage[b].get(), cnt * unit, hipMemcpyDeviceToHost, st));
      ZK_HIP(hipEventRecord(ev[b], st));
    };
    if (count) issue(0, 0);
    int b = 0;
    for (uint64_t first = 0; first < count; first += per_piece, b ^= 1) {
      const uint64_t cnt = std::min(per_piece, count - first);
      if (first + per_piece < count) issue(first + per_piece, b ^ 1);   // its buffer was hashed in the last round
      const auto t0 = std::chrono::steady_clock::now();
      ZK_HIP(hipEventSynchronize(ev[b]));
      const auto t1 = std::chrono::steady_clock::now();
      const uint8_t* piece = pinned[b].as<const uint8_t>();
      hasher.update(piece, cnt * unit);
      if (capture) capture->insert(capture->end(), piece, piece + cnt * unit);
      if (sink) sink(piece, cnt * unit);
      convert_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
      hash_ms += zkpoa::ms_since(t1);
      bytes += cnt * unit;
    }
    ZK_HIP(hipGetLastError());
  }
};

// d_out[i] = T[i + n] - T[i] for i < n - 1 (T: the ptau's tau^i G1, at least 2n - 1 points on the device)
inline void h_diff(zkpoa_context* ctx, const void* d_T, uint64_t n, void* d_out) {
  if (n < 2) return;
  hipStream_t st = ctx->dev.lanes[0].stream;
  const uint64_t count = n - 1, threads = (count + kHDiffBatch - 1) / kHDiffBatch;
  hipLaunchKernelGGL(h_diff_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, st, d_T, n, count, d_out);
  ZK_HIP(hipStreamSynchronize(st));
  ZK_HIP(hipGetLastError());
}

}  // namespace
