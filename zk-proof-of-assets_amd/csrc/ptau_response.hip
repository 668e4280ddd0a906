// The inverse directions of the two byte forms of a ceremony's points (DESIGN.md "Phase-1 transcript", "Challenge and
// response files"): hash form -> wire form (what `powersoftau challenge contribute` reads) and compressed form -> wire
// form (what `powersoftau import response` reads), with the square root in Fq and Fq2 that decompression needs. The
// forward directions are hash_form_kernel and compressed_form_kernel of csrc/phase2_dev.hip.h; the commands that use
// these are in csrc/ptau_contribute.hip.
//
// The root. q = 3 mod 4: a^((q + 1) / 4) is a root of a when there is one, and a^((q + 1) / 4) = a * a^((q - 3) / 4). Both
// fields are served by the one exponent E = (q - 3) / 4 (fq_pow_e). The exponent is the same for every element, so the walk
// is a fixed one: a sliding window of 4 bits over E, made once on the host (sqrt_chain: runs of squarings, each followed
// by one product with an odd power a, a^3, ..., a^15) and handed to the kernel as an argument. Every lane of a wave
// squares and multiplies in step; the only branch is on the chain's entry, which is uniform.
//   Fq:  s = a^E, root = s a, a square iff root^2 = a.
//   Fq2: a = a0 + a1 u. d = sqrt(a0^2 + a1^2) (the norm, first exponentiation), t = (a0 + d) / 2 (t = a0 when a1 = 0),
//        s = t^E (second exponentiation), c = s t, so c^2 = chi t with chi = t^((q - 1) / 2) = s^2 t = +-1. The inverse of c
//        is s chi. chi = 1: root = (c, a1 / (2c)); chi = -1: root = (a1 / (2c), c) (-1 is a non-residue, u^2 = -1). A lane
//        takes two exponentiations whatever its element; a is a square iff root^2 = a.
#include "phase2_dev.hip.h"
#include "setup_common.hip.h"
#include "zkpoa_internal.hpp"

using namespace zkpoa;

namespace {

constexpr uint32_t kFormThreads = 256;   // the workgroup of every kernel here

// ---- a^E, E = (q - 3) / 4 ------------------------------------------------------------------------------------------------
// step k: (step[k] & 0xff) squarings, then a product with a^(2 m - 1) when m = step[k] >> 8 is not zero
struct SqrtChain {
  uint32_t n;
  uint32_t step[80];
};
SqrtChain sqrt_chain() {
  uint64_t e[4] = {HFqParams::P[0], HFqParams::P[1], HFqParams::P[2], HFqParams::P[3]};
  e[0] -= 3;   // q = 3 mod 4: no borrow
  for (int i = 0; i < 4; i++) e[i] = (e[i] >> 2) | (i < 3 ? e[i + 1] << 62 : 0);
  auto bit = [&](int i) { return i >= 0 && ((e[i >> 6] >> (i & 63)) & 1u); };
  SqrtChain ch{};
  int i = 255, pending = 0;
  while (i >= 0 && !bit(i)) i--;
  while (i >= 0) {
    if (!bit(i)) {
      pending++;
      i--;
      continue;
    }
    int j = i - 3 < 0 ? 0 : i - 3;   // the longest window of at most 4 bits that ends in a set bit
    while (!bit(j)) j++;
    uint32_t v = 0;
    for (int b = i; b >= j; b--) v = (v << 1) | (bit(b) ? 1u : 0u);
    ch.step[ch.n++] = (uint32_t)(pending + (i - j + 1)) | ((v + 1) / 2) << 8;
    pending = 0;
    i = j - 1;
  }
  if (pending) ch.step[ch.n++] = (uint32_t)pending;
  return ch;
}
const SqrtChain& the_sqrt_chain() {   // made once per process
  static const SqrtChain ch = sqrt_chain();
  return ch;
}
ZK_DEV Fq fq_pow_e(const Fq& a, const SqrtChain& ch) {
  Fq tab[8];   // a, a^3, ..., a^15
  tab[0] = a;
  const Fq a2 = a.sqr();
#pragma unroll
  for (int k = 1; k < 8; k++) tab[k] = tab[k - 1] * a2;
  Fq acc = Fq::one();
  for (uint32_t k = 0; k < ch.n; k++) {
    const uint32_t step = ch.step[k];
    for (uint32_t s = step & 0xffu; s; s--) acc = acc.sqr();
    switch (step >> 8) {   // uniform: the chain is the kernel's argument
      case 1: acc = acc * tab[0]; break;
      case 2: acc = acc * tab[1]; break;
      case 3: acc = acc * tab[2]; break;
      case 4: acc = acc * tab[3]; break;
      case 5: acc = acc * tab[4]; break;
      case 6: acc = acc * tab[5]; break;
      case 7: acc = acc * tab[6]; break;
      case 8: acc = acc * tab[7]; break;
      default: break;
    }
  }
  return acc;
}
// a / 2 on the Montgomery representation (halving it halves the element)
ZK_DEV Fq fq_half(const Fq& a) {
  const Fq c = a.canon();
  const uint32_t mask = 0u - (c.l[0] & 1u);
  uint32_t carry = 0, s[8];
#pragma unroll
  for (int k = 0; k < 8; k++) s[k] = addc(c.l[k], FqParams::P[k] & mask, carry);   // < 2q < 2^255
  Fq r;
#pragma unroll
  for (int k = 0; k < 8; k++) r.l[k] = (s[k] >> 1) | (k < 7 ? s[k + 1] << 31 : 0u);
  return r;
}
ZK_DEV bool fq_negative(const Fq& a) { return fq_std_negative(a.from_mont().canon()); }   // a: Montgomery form
ZK_DEV bool field_negative(const Fq& a) { return fq_negative(a); }
ZK_DEV bool field_negative(const Fq2& a) { return a.c1.is_zero() ? fq_negative(a.c0) : fq_negative(a.c1); }

// a root of a, and whether it is one (a is a square)
ZK_DEV bool field_sqrt(const Fq& a, const SqrtChain& ch, Fq& root) {
  root = fq_pow_e(a, ch) * a;
  return root.sqr() == a;
}
ZK_DEV bool field_sqrt(const Fq2& a, const SqrtChain& ch, Fq2& root) {
  Fq n0, n1;
  Fq::sqr_pair(a.c0, a.c1, n0, n1);
  const Fq norm = n0 + n1;
  const Fq d = fq_pow_e(norm, ch) * norm;
  const Fq t = a.c1.is_zero() ? a.c0 : fq_half(a.c0 + d);
  const Fq s = fq_pow_e(t, ch);
  const Fq c = s * t, chi = s.sqr() * t;   // c^2 = chi t, chi = +-1 (0 when t = 0)
  const Fq other = fq_half(a.c1 * (s * chi));
  const bool plus = chi == Fq::one();
  root = plus ? Fq2{c, other} : Fq2{other, c};
  return root.sqr() == a;
}

// ---- the first offender of a conversion: atomicMin over (point index << 3 | kind) ------------------------------------------
enum FormFault : uint32_t { kNotBelowQ = 1, kBit7 = 2, kBothFlags = 3, kInfNotZero = 4, kNotOnCurve = 5 };
constexpr unsigned long long kNoFault = ~0ull;
ZK_DEV void form_fault(unsigned long long* first, uint64_t point, uint32_t kind) { atomicMin(first, (point << 3) | kind); }

ZK_DEV bool fq_below_q(const Fq& s) {
  uint32_t bw = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) (void)subb(s.l[k], FqParams::P[k], bw);
  return bw != 0;
}
// 32 bytes big-endian -> limbs (standard form); the first byte is the top byte of l[7]
ZK_DEV Fq load_be(const uint4* in) {
  const uint4 hi = in[0], lo = in[1];
  Fq s;
  s.l[7] = __builtin_bswap32(hi.x); s.l[6] = __builtin_bswap32(hi.y); s.l[5] = __builtin_bswap32(hi.z); s.l[4] = __builtin_bswap32(hi.w);
  s.l[3] = __builtin_bswap32(lo.x); s.l[2] = __builtin_bswap32(lo.y); s.l[1] = __builtin_bswap32(lo.z); s.l[0] = __builtin_bswap32(lo.w);
  return s;
}

// Hash form -> wire form, the inverse of hash_form_kernel: one lane per 32-byte coordinate, K = 2 (G1) or 4 (G2: x.c1,
// x.c0, y.c1, y.c0 -> x.c0, x.c1, y.c0, y.c1) lanes make a point. 0x40 then zeros is infinity: the all-zero point.
// Faults: bit 7 of a point's first byte, 0x40 followed by anything but zeros, a coordinate not below q.
template <int K>
static __global__ __launch_bounds__(kFormThreads) void from_hash_form_kernel(const uint4* __restrict__ in, uint4* __restrict__ out,
                                                                             uint64_t count, unsigned long long* __restrict__ first) {
  const uint64_t i = (uint64_t)blockIdx.x * kFormThreads + threadIdx.x;
  const bool live = i < count;   // (no early return: the lanes of a point exchange below)
  Fq s = Fq::zero();
  if (live) s = load_be(in + 2 * i);
  const bool head = (i & (K - 1)) == 0;
  const bool bit7 = head && (s.l[7] >> 31);
  const bool inf_byte = head && (s.l[7] >> 24) == 0x40u;
  if (inf_byte) s.l[7] &= 0x00ffffffu;
  uint32_t nz = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) nz |= s.l[k];
  uint32_t inf = inf_byte ? 1u : 0u;
  nz |= __shfl_xor(nz, 1);
  inf |= __shfl_xor(inf, 1);
  if (K == 4) {
    nz |= __shfl_xor(nz, 2);
    inf |= __shfl_xor(inf, 2);
  }
  if (!live) return;
  const uint64_t point = i / K;
  if (bit7) form_fault(first, point, kBit7);
  else if (inf && nz) form_fault(first, point, kInfNotZero);
  else if (!fq_below_q(s)) form_fault(first, point, kNotBelowQ);
  const uint64_t o = K == 4 ? (i ^ 1ull) : i;
  store_fp<FqParams>(out + 2 * o, s.to_mont());
}

// Compressed form -> wire form, the inverse of compressed_form_kernel: one lane per point. x (G2: c1 then c0) with the
// two flag bits of the first byte taken off, y the root of x^3 + b that is negative exactly when bit 7 is set.
// Faults: both flag bits, 0x40 followed by anything but zeros, x not below q, x^3 + b not a square.
template <class F>
static __global__ __launch_bounds__(kFormThreads) void decompressed_form_kernel(const uint4* __restrict__ in, void* __restrict__ out,
                                                                                uint64_t count, CurveB b, SqrtChain ch,
                                                                                unsigned long long* __restrict__ first) {
  const uint64_t i = (uint64_t)blockIdx.x * kFormThreads + threadIdx.x;
  if (i >= count) return;
  constexpr int kCoords = FieldBytes<F>::N / 32;
  Fq xs[kCoords];   // G2: c1, c0
  uint32_t nz = 0;
  bool below = true;
#pragma unroll
  for (int c = 0; c < kCoords; c++) xs[c] = load_be(in + 2 * (kCoords * i + c));
  const uint32_t flags = xs[0].l[7] >> 30;
  xs[0].l[7] &= 0x3fffffffu;
#pragma unroll
  for (int c = 0; c < kCoords; c++) {
#pragma unroll
    for (int k = 0; k < 8; k++) nz |= xs[c].l[k];
    below = below && fq_below_q(xs[c]);
  }
  char* o = reinterpret_cast<char*>(out) + 2 * FieldBytes<F>::N * i;
  F x, y = F::zero();
  if constexpr (kCoords == 1) x = xs[0].to_mont();
  else x = Fq2{xs[1].to_mont(), xs[0].to_mont()};
  uint32_t fault = 0;
  if (flags == 3u) fault = kBothFlags;
  else if ((flags & 1u) && nz) fault = kInfNotZero;
  else if (!below) fault = kNotBelowQ;
  if (fault || (flags & 1u)) {   // nothing to take a root of: the all-zero point
    if (fault) form_fault(first, i, fault);
    store_field(o, F::zero());
    store_field(o + FieldBytes<F>::N, F::zero());
    return;
  }
  const F rhs = x.sqr() * x + load_field<F>(b.q);
  if (!field_sqrt(rhs, ch, y)) form_fault(first, i, kNotOnCurve);
  if (field_negative(y) != ((flags & 2u) != 0)) y = y.neg();
  store_field(o, x);
  store_field(o + FieldBytes<F>::N, y);
}

// roots[i] = the non-negative root of a[i] (zero when there is none), ok[i] = 1 when a[i] is a square; wire form
template <class F>
static __global__ __launch_bounds__(kFormThreads) void sqrt_kernel(const void* __restrict__ a, uint64_t n, SqrtChain ch,
                                                                   void* __restrict__ roots, uint8_t* __restrict__ ok) {
  const uint64_t i = (uint64_t)blockIdx.x * kFormThreads + threadIdx.x;
  if (i >= n) return;
  const F v = load_field<F>(reinterpret_cast<const char*>(a) + FieldBytes<F>::N * i);
  F root;
  const bool sq = field_sqrt(v, ch, root);
  if (!sq) root = F::zero();
  else if (field_negative(root)) root = root.neg();
  store_field(reinterpret_cast<char*>(roots) + FieldBytes<F>::N * i, root);
  ok[i] = sq ? 1 : 0;
}

const char* fault_text(uint32_t kind) {
  switch (kind) {
    case kNotBelowQ: return "a coordinate is not below q";
    case kBit7: return "bit 7 of its first byte is set";
    case kBothFlags: return "both flag bits of its first byte are set";
    case kInfNotZero: return "0x40 (infinity) is followed by bytes that are not zero";
    default: return "x is not on the curve (x^3 + b is not a square)";
  }
}

}  // namespace

namespace zkpoa {

FormConverter::FormConverter(zkpoa_context* c) : ctx(c), first(8) {
  ZK_HIP(hipMemsetAsync(first.p, 0xff, 8, ctx->dev.lanes[0].stream));
}
void FormConverter::convert(bool compressed, int group, const void* d_bytes, uint64_t n, void* d_out) {
  if (!n) return;
  const uint64_t lanes = compressed ? n : n * (group == 2 ? 4 : 2);
  if ((lanes + kFormThreads - 1) / kFormThreads >> 31) throw SetupError("form conversion: too many points in one call");
  const dim3 grid((uint32_t)((lanes + kFormThreads - 1) / kFormThreads)), block(kFormThreads);
  hipStream_t st = ctx->dev.lanes[0].stream;
  unsigned long long* f = static_cast<unsigned long long*>(first.p);
  const uint4* in = static_cast<const uint4*>(d_bytes);
  const SqrtChain& ch = the_sqrt_chain();
  CurveB b{};
  if (group == 2) pairing::twist_b().to_bytes(&b.q[0]);
  else HFq::from_u64(3).to_bytes(&b.q[0]);
  if (!compressed && group == 1) hipLaunchKernelGGL((from_hash_form_kernel<2>), grid, block, 0, st, in, (uint4*)d_out, lanes, f);
  else if (!compressed) hipLaunchKernelGGL((from_hash_form_kernel<4>), grid, block, 0, st, in, (uint4*)d_out, lanes, f);
  else if (group == 1) hipLaunchKernelGGL((decompressed_form_kernel<Fq>), grid, block, 0, st, in, d_out, n, b, ch, f);
  else hipLaunchKernelGGL((decompressed_form_kernel<Fq2>), grid, block, 0, st, in, d_out, n, b, ch, f);
  ZK_HIP(hipGetLastError());
}
void FormConverter::require(uint64_t i0, const char* what) {
  unsigned long long v = kNoFault;
  ZK_HIP(hipMemcpyAsync(&v, first.p, 8, hipMemcpyDeviceToHost, ctx->dev.lanes[0].stream));
  ZK_HIP(hipStreamSynchronize(ctx->dev.lanes[0].stream));
  if (v == kNoFault) return;
  ZK_HIP(hipMemsetAsync(first.p, 0xff, 8, ctx->dev.lanes[0].stream));
  throw SetupError(std::string(what) + ": point " + std::to_string(i0 + (v >> 3)) + ": " + fault_text((uint32_t)(v & 7u)));
}

}  // namespace zkpoa

// host points in, host points out, in pieces of piece_points
static void form_to_wire(zkpoa_context* ctx, bool compressed, int group, const void* bytes, uint64_t n, uint64_t piece_points,
                         void* out_points) {
  const char* const what = compressed ? "decompressed form" : "from hash form";
  if ((group != 1 && group != 2) || (n && (!bytes || !out_points))) throw SetupError(std::string(what) + ": bad argument");
  const uint64_t unit = group == 1 ? 64 : 128, in_unit = compressed ? unit / 2 : unit;
  if (!piece_points) piece_points = 1ull << 18;
  const uint64_t piece = std::min(piece_points, n ? n : 1);
  DevBuf d_in(piece * in_unit), d_out(piece * unit);
  FormConverter conv(ctx);
  for (uint64_t i0 = 0; i0 < n; i0 += piece) {
    const uint64_t cnt = std::min(piece, n - i0);
    d_in.up(static_cast<const char*>(bytes) + i0 * in_unit, cnt * in_unit);
    conv.convert(compressed, group, d_in.p, cnt, d_out.p);
    conv.require(i0, what);
    ZK_HIP(hipMemcpy(static_cast<char*>(out_points) + i0 * unit, d_out.p, cnt * unit, hipMemcpyDeviceToHost));
  }
}

extern "C" int zkpoa_decompressed_form(zkpoa_context* ctx, int group, const void* bytes, uint64_t n, uint64_t piece_points,
                                       void* out_points) {
  ZK_API_BEGIN(ctx)
  form_to_wire(ctx, true, group, bytes, n, piece_points, out_points);
  ZK_API_END(ctx)
}

extern "C" int zkpoa_from_hash_form(zkpoa_context* ctx, int group, const void* bytes, uint64_t n, uint64_t piece_points,
                                    void* out_points) {
  ZK_API_BEGIN(ctx)
  form_to_wire(ctx, false, group, bytes, n, piece_points, out_points);
  ZK_API_END(ctx)
}

extern "C" int zkpoa_sqrt_device(zkpoa_context* ctx, int field, const void* a, uint64_t n, void* roots, uint8_t* is_square) {
  ZK_API_BEGIN(ctx)
  if (field != 0 && field != 2) throw SetupError("sqrt: field must be 0 (Fq) or 2 (Fq2)");
  if (n && (!a || !roots || !is_square)) throw SetupError("sqrt: null pointer");
  if (n == 0) return PROVER_OK;
  const uint64_t size = field == 2 ? 64 : 32;
  if ((n + kFormThreads - 1) / kFormThreads >> 31) throw SetupError("sqrt: too many elements in one call");
  host_check_coords(static_cast<const uint8_t*>(a), n * size / 32, "sqrt");
  DevBuf d_a(n * size), d_r(n * size), d_ok(n);
  d_a.up(a, n * size);
  hipStream_t st = ctx->dev.lanes[0].stream;
  const dim3 grid((uint32_t)((n + kFormThreads - 1) / kFormThreads));
  const SqrtChain& ch = the_sqrt_chain();
  if (field == 0) hipLaunchKernelGGL((sqrt_kernel<Fq>), grid, dim3(kFormThreads), 0, st, (const void*)d_a.p, n, ch, d_r.p, (uint8_t*)d_ok.p);
  else hipLaunchKernelGGL((sqrt_kernel<Fq2>), grid, dim3(kFormThreads), 0, st, (const void*)d_a.p, n, ch, d_r.p, (uint8_t*)d_ok.p);
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipStreamSynchronize(st));
  ZK_HIP(hipMemcpy(roots, d_r.p, n * size, hipMemcpyDeviceToHost));
  ZK_HIP(hipMemcpy(is_square, d_ok.p, n, hipMemcpyDeviceToHost));
  ZK_API_END(ctx)
}
