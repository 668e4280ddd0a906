// HD-wallet key sources (include/zkpoa_hd_wallet.h): the child-key step of BIP-32 on the GPU, one child index per lane,
// batched SHA-512 / HMAC-SHA512, and on the host what stands before a range of children: the master key of a seed, the
// seed of a BIP-39 mnemonic, the reading of an extended key and of a path. The arithmetic is csrc/secp256k1.hip.h and
// csrc/sha512.hip.h; this file is the kernels and the C ABI. Not hardened against side channels: see the header.
//
// A range of children is two kernels. bip32_hmac_kernel: I = HMAC-SHA512(chain, data || be32(i)) from the mid-states of
// the chain code, two compressions per lane, 64-bit words and few of them. bip32_tweak_kernel: IL -> the child, one
// fixed-base multiplication, and under a public parent one mixed addition of the parent; it is also all of
// zkpoa_bip32_tweak. Between them IL crosses device memory once (32 bytes per lane); in return the curve kernel does
// not carry the hash's registers, and the status paths of the tweak are tested on the kernel that runs in a derivation.
#include "lane_batch.hip.h"
#include "secp256k1.hip.h"
#include "sha512.hip.h"

#include <string.h>

using namespace zkpoa;
using namespace zkpoa::secp;

namespace {

constexpr uint32_t kTweakThreads = 64;         // one wave per workgroup, as the public-key kernel
constexpr uint64_t kTweakLanesMax = 1u << 20;  // children per launch
constexpr uint32_t kHardened = 0x80000000u;

// What every lane of a call reads about the parent: made on the host, once per call.
struct Parent {
  sha512::HmacKey mac;     // the chain code as the HMAC key: the state after the ipad and after the opad block
  uint64_t data[2][5];     // the 33 bytes before the index as big-endian words, byte 32 at the top of word 4:
                           // [0] serP(K_par), [1] 0x00 || ser256(k_par) (a private parent only)
  uint32_t k[8];           // k_par (a private parent), least significant limb first
  AffineK K;               // K_par
  uint32_t is_private;
};

__global__ __launch_bounds__(256) void sha512_kernel(const uint8_t* __restrict__ messages, uint32_t len, uint64_t n,
                                                     uint32_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  uint64_t h[8];
  sha512::digest(messages + t * len, len, h);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    out[16 * t + 2 * i] = bswap32((uint32_t)(h[i] >> 32));
    out[16 * t + 2 * i + 1] = bswap32((uint32_t)h[i]);
  }
}

__global__ __launch_bounds__(256) void hmac_sha512_kernel(const sha512::HmacKey* __restrict__ key, const uint8_t* __restrict__ messages,
                                                          uint32_t len, uint64_t n, uint32_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  const uint8_t* msg = messages + t * len;
  uint64_t h[8];
  sha512::hmac_of(*key, [msg](uint32_t j) -> uint32_t { return msg[j]; }, len, h);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    out[16 * t + 2 * i] = bswap32((uint32_t)(h[i] >> 32));
    out[16 * t + 2 * i + 1] = bswap32((uint32_t)h[i]);
  }
}

// Lane t: I for child index first + t (which is below 2^32). The 37-byte message is one block: data, the index at bytes
// 33 .. 36, 0x80 at byte 37. The data form goes by the lane's own index: a wave may hold both.
__global__ __launch_bounds__(256) void bip32_hmac_kernel(const Parent* __restrict__ par, uint64_t first, uint64_t n,
                                                         uint32_t* __restrict__ out_il, uint32_t* __restrict__ out_chain) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  const uint32_t index = (uint32_t)(first + t);
  const uint64_t* data = par->data[index >> 31];
  uint64_t m[16], I[8];
#pragma unroll
  for (int i = 0; i < 16; i++) m[i] = i < 5 ? data[i] : 0;
  m[4] |= ((uint64_t)index << 24) | (0x80ull << 16);
  m[15] = 8 * (128 + 37);
  sha512::hmac_block(par->mac, m, I);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    out_il[8 * t + 2 * i] = bswap32((uint32_t)(I[i] >> 32));
    out_il[8 * t + 2 * i + 1] = bswap32((uint32_t)I[i]);
    out_chain[8 * t + 2 * i] = bswap32((uint32_t)(I[4 + i] >> 32));
    out_chain[8 * t + 2 * i + 1] = bswap32((uint32_t)I[4 + i]);
  }
}

// Lane t: the child for tweak IL_t. A private parent: k = IL + k_par, Q = k G. A public parent: Q = IL G + K_par, by one
// mixed addition after the multiplication (complete: IL G = K_par doubles, IL G = -K_par is infinity). An invalid lane
// (IL zero or not below n, k zero, Q infinity) walks the same path with the scalar 1 and gets zeros, in its chain code
// too when the call has one.
__global__ __launch_bounds__(kTweakThreads) void bip32_tweak_kernel(const Parent* __restrict__ par, const void* __restrict__ tweaks,
                                                                    const AffineK* __restrict__ ftab, uint64_t n,
                                                                    void* __restrict__ out_key32, uint8_t* __restrict__ out_prefix,
                                                                    uint32_t* __restrict__ chain, void* __restrict__ out_pubkey,
                                                                    uint32_t* __restrict__ out_address, uint8_t* __restrict__ out_status) {
  const uint64_t t = (uint64_t)blockIdx.x * kTweakThreads + threadIdx.x;
  if (t >= n) return;
  Sc s;
  load_be32(tweaks, t, s.l);
  uint32_t status = (s.is_zero() || s.ge_n()) ? 1u : 0u;
  if (status) s = Sc::one();
  const bool priv = par->is_private != 0;
  if (priv) {
    Sc kp;
#pragma unroll
    for (int i = 0; i < 8; i++) kp.l[i] = par->k[i];
    s = sc_add(s, kp);
    if (s.is_zero()) {
      status = 1u;
      s = Sc::one();
    }
  }
  XyzzK P = fixed_mul(s, ftab);
  if (!priv) {
    const AffineK K = par->K;
    xyzz_add_affine(P, K, false);
    if (P.is_inf()) {
      status = 1u;
      P = XyzzK::from_affine(generator());
    }
  }
  AffineK q = to_affine(P);
  uint32_t addr[5];
  eth_address_words(q, addr);
  uint32_t key[8];
#pragma unroll
  for (int i = 0; i < 8; i++) key[i] = priv ? s.l[i] : q.x.l[i];
  uint32_t prefix = priv ? 0u : (q.y.is_odd() ? 3u : 2u);
  if (status) {
    q = {secp::Fp::zero(), secp::Fp::zero()};
    prefix = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) key[i] = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) addr[i] = 0;
    if (chain) {
#pragma unroll
      for (int i = 0; i < 8; i++) chain[8 * t + i] = 0;
    }
  }
  store_be32(out_key32, t, key);
  out_prefix[t] = (uint8_t)prefix;
  store_key_outputs(t, q, addr, status, out_pubkey, out_address, out_status);
}

// ---- the host side ---------------------------------------------------------------------------------------------------
void limbs_from_be(const uint8_t* b, uint32_t (&l)[8]) {
  for (int i = 0; i < 8; i++) l[7 - i] = ((uint32_t)b[4 * i] << 24) | ((uint32_t)b[4 * i + 1] << 16) | ((uint32_t)b[4 * i + 2] << 8) | b[4 * i + 3];
}
void be_from_limbs(const uint32_t (&l)[8], uint8_t* b) {
  for (int i = 0; i < 8; i++)
    for (int k = 0; k < 4; k++) b[4 * i + k] = (uint8_t)(l[7 - i] >> (24 - 8 * k));
}
void be_from_words(const uint64_t* w, int words, uint8_t* b) {
  for (int i = 0; i < words; i++)
    for (int k = 0; k < 8; k++) b[8 * i + k] = (uint8_t)(w[i] >> (56 - 8 * k));
}

// a private key in [1, n)?
bool private_key_of(const uint8_t* be, Sc& k) {
  limbs_from_be(be, k.l);
  return !k.is_zero() && !k.ge_n();
}
// the point of 02 / 03 || x, when x is below p and on the curve
bool decompress(const uint8_t* key33, AffineK& out) {
  if (key33[0] != 2 && key33[0] != 3) return false;
  secp::Fp x;
  limbs_from_be(key33 + 1, x.l);
  if (x.ge_p()) return false;
  const secp::Fp rhs = x.sqr() * x + secp::Fp::small(7);
  secp::Fp y = rhs.sqrt_candidate();
  if (!(y.sqr() == rhs)) return false;
  if (y.is_odd() != (key33[0] == 3)) y = y.neg();
  out = {x, y};
  return true;
}

void data_words(const uint8_t (&b)[33], uint64_t (&w)[5]) {
  for (int i = 0; i < 4; i++) {
    w[i] = 0;
    for (int k = 0; k < 8; k++) w[i] = (w[i] << 8) | b[8 * i + k];
  }
  w[4] = (uint64_t)b[32] << 56;
}

// The parent of a call from its key data (and chain code: nullptr for the tweak alone). Throws for key data that is none.
void make_parent(const char* name, const uint8_t* key33, const uint8_t* chain32, Parent& par) {
  memset(&par, 0, sizeof(par));
  uint8_t ser[33];
  if (key33[0] == 0) {
    Sc k;
    if (!private_key_of(key33 + 1, k)) throw HipError(std::string(name) + ": the parent's private key is zero or not below the group order");
    par.is_private = 1;
    for (int i = 0; i < 8; i++) par.k[i] = k.l[i];
    par.K = to_affine(fixed_mul(k, fixed_table_host()));
    memcpy(ser, key33, 33);
    data_words(ser, par.data[1]);
  } else if (!decompress(key33, par.K)) {
    throw HipError(std::string(name) + ": the parent key is neither 0x00 || a private key nor 02 / 03 || the x of a curve point");
  }
  ser[0] = par.K.y.is_odd() ? 3 : 2;
  be_from_limbs(par.K.x.l, ser + 1);
  data_words(ser, par.data[0]);
  if (chain32) sha512::hmac_key(chain32, 32, par.mac);
}

// n x 33 B key data from the kernel's two arrays
void join_key_data(const std::vector<uint8_t>& prefix, const std::vector<uint8_t>& key32, uint64_t n, uint8_t* out_key33) {
  for (uint64_t i = 0; i < n; i++) {
    out_key33[33 * i] = prefix[i];
    memcpy(out_key33 + 33 * i + 1, &key32[32 * i], 32);
  }
}

// The tweak kernel over n lanes and its outputs; tweaks: on the device. chain: the device array of the chain codes, or
// nullptr. Called inside timed().
struct TweakOut {
  LaneOut<SecretBuf> key32;
  LaneOut<> prefix, pub, addr, status;
  std::vector<uint8_t> h_key32, h_prefix;
  uint8_t* out_key33;
  TweakOut(uint64_t n, hipStream_t st, void* out_key33_, void* out_pubkey_xy, void* out_address20, uint8_t* out_status)
      : key32(nullptr, 32, n, st), prefix(nullptr, 1, n), pub(out_pubkey_xy, 64, n), addr(out_address20, 20, n), status(out_status, 1, n),
        h_key32(32 * n), h_prefix(n), out_key33(static_cast<uint8_t*>(out_key33_)) {
    key32.host = h_key32.data();
    prefix.host = h_prefix.data();
  }
  void launch(hipStream_t st, const Parent* d_par, const void* d_tweaks, uint32_t* d_chain, const AffineK* d_tab, uint64_t n) {
    for_slabs(n, kTweakLanesMax, [&](uint64_t i0, uint64_t m) {
      hipLaunchKernelGGL(bip32_tweak_kernel, dim3(blocks_of(m, kTweakThreads)), dim3(kTweakThreads), 0, st, d_par,
                         static_cast<const void*>(static_cast<const char*>(d_tweaks) + 32 * i0), d_tab, m, key32.at<void>(i0),
                         prefix.at<uint8_t>(i0), d_chain ? d_chain + 8 * i0 : nullptr, pub.at<void>(i0), addr.at<uint32_t>(i0),
                         status.at<uint8_t>(i0));
    });
  }
  void down() {
    key32.down();
    prefix.down();
    join_key_data(h_prefix, h_key32, h_prefix.size(), out_key33);
    for (const auto* o : {&pub, &addr, &status}) o->down();
  }
};

bool public_key_data(const uint8_t* key33) { return key33[0] != 0; }

// zkpoa_bip32_children, and each level of zkpoa_bip32_derive_path
void children(zkpoa_context* ctx, const uint8_t* parent_key33, const uint8_t* chain32, uint64_t first, uint64_t n, void* out_key33,
              void* out_chain32, void* out_pubkey_xy, void* out_address20, uint8_t* out_status) {
  ctx->ms[kMsLaneBatch] = 0;
  if (first > (1ull << 32) || n > (1ull << 32) - first) throw HipError("bip32_children: first_index + n is at most 2^32");
  if (!batch_wanted("bip32_children", "children", n,
                    parent_key33 && chain32 && out_key33 && out_chain32 && out_pubkey_xy && out_address20 && out_status))
    return;
  if (public_key_data(parent_key33) && first + n > kHardened) throw HipError("bip32_children: a public parent has no hardened children (an index of 2^31 or more)");
  Parent par;
  make_parent("bip32_children", parent_key33, chain32, par);
  hipStream_t st = ctx->dev.lanes[0].stream;
  LaneIn dtab(fixed_table_host(), sizeof(AffineK), kFixedEntries);
  LaneIn<SecretBuf> dpar(&par, sizeof(par), 1, st);
  LaneArray<SecretBuf> il(32, n, st);
  LaneOut ochain(out_chain32, 32, n);
  TweakOut out(n, st, out_key33, out_pubkey_xy, out_address20, out_status);
  timed(ctx, st, kMsLaneBatch, [&] {
    for_slabs(n, kTweakLanesMax, [&](uint64_t i0, uint64_t m) {
      hipLaunchKernelGGL(bip32_hmac_kernel, dim3(blocks_of(m, 256)), dim3(256), 0, st, dpar.at<const Parent>(0), first + i0, m,
                         il.at<uint32_t>(i0), ochain.at<uint32_t>(i0));
    });
    out.launch(st, dpar.at<const Parent>(0), il.at<const void>(0), ochain.at<uint32_t>(0), dtab.at<const AffineK>(0), n);
  });
  memset(&par, 0, sizeof(par));
  ochain.down();
  out.down();
}

const char kBase58[] = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz";

// base58 -> exactly `want` bytes
bool base58_decode(const char* text, uint8_t* out, size_t want) {
  const size_t len = strlen(text);
  if (len == 0 || len > 2 * want) return false;
  std::vector<uint8_t> num(want, 0);   // big-endian
  size_t zeros = 0;
  while (text[zeros] == '1') zeros++;
  for (size_t i = 0; i < len; i++) {
    const char* at = text[i] ? strchr(kBase58, text[i]) : nullptr;
    if (!at) return false;
    uint32_t carry = (uint32_t)(at - kBase58);
    for (size_t k = want; k-- > 0;) {
      carry += 58u * num[k];
      num[k] = (uint8_t)carry;
      carry >>= 8;
    }
    if (carry) return false;   // more than `want` bytes
  }
  size_t lead = 0;
  while (lead < want && num[lead] == 0) lead++;
  if (lead != zeros) return false;   // every leading zero byte is a '1' and the other way round: the length is `want`
  memcpy(out, num.data(), want);
  return true;
}

void sha256d(const uint8_t* msg, uint32_t len, uint8_t (&out)[32]) {
  uint32_t h[8];
  uint8_t first[32];
  sha256::digest(msg, len, h);
  for (int i = 0; i < 8; i++)
    for (int k = 0; k < 4; k++) first[4 * i + k] = (uint8_t)(h[i] >> (24 - 8 * k));
  sha256::digest(first, 32, h);
  for (int i = 0; i < 8; i++)
    for (int k = 0; k < 4; k++) out[4 * i + k] = (uint8_t)(h[i] >> (24 - 8 * k));
}

// the indices of a path; false for anything that is none
bool parse_path(const char* path, std::vector<uint32_t>& out) {
  out.clear();
  if (!path || path[0] != 'm') return false;
  const char* p = path + 1;
  while (*p) {
    if (*p++ != '/') return false;
    uint64_t v = 0;
    int digits = 0;
    for (; *p >= '0' && *p <= '9'; p++, digits++) {
      v = v * 10 + (uint64_t)(*p - '0');
      if (v >= kHardened) return false;
    }
    if (!digits) return false;
    if (*p == '\'' || *p == 'h') {
      v |= kHardened;
      p++;
    }
    if (out.size() == 255) return false;
    out.push_back((uint32_t)v);
  }
  return true;
}

#define ZK_HOST_API_BEGIN try {
#define ZK_HOST_API_END              \
  }                                  \
  catch (const std::exception&) {    \
    return PROVER_ERROR;             \
  }                                  \
  return PROVER_OK;

}  // namespace

extern "C" int zkpoa_sha512_batch(zkpoa_context* ctx, const void* messages, uint64_t message_len, uint64_t n, void* out64) {
  ZK_API_BEGIN(ctx)
  if (message_len > 4096) throw HipError("sha512: messages of at most 4096 bytes");
  if (!batch_wanted("sha512", "messages", n, (messages || !message_len) && out64)) return PROVER_OK;
  LaneIn dm(messages, message_len, n);
  LaneOut dout(out64, 64, n);
  hipStream_t st = ctx->dev.lanes[0].stream;
  hipLaunchKernelGGL(sha512_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, dm.at<const uint8_t>(0), (uint32_t)message_len, n,
                     dout.at<uint32_t>(0));
  finish(st);
  dout.down();
  ZK_API_END(ctx)
}

extern "C" int zkpoa_hmac_sha512_batch(zkpoa_context* ctx, const void* key, uint64_t key_len, const void* messages, uint64_t message_len,
                                       uint64_t n, void* out64) {
  ZK_API_BEGIN(ctx)
  if (message_len > 4096) throw HipError("hmac_sha512: messages of at most 4096 bytes");
  if (key_len > 4096) throw HipError("hmac_sha512: a key of at most 4096 bytes");
  if (!batch_wanted("hmac_sha512", "messages", n, (key || !key_len) && (messages || !message_len) && out64)) return PROVER_OK;
  hipStream_t st = ctx->dev.lanes[0].stream;
  sha512::HmacKey mac;
  sha512::hmac_key(static_cast<const uint8_t*>(key), (uint32_t)key_len, mac);
  LaneIn<SecretBuf> dkey(&mac, sizeof(mac), 1, st);
  memset(&mac, 0, sizeof(mac));
  LaneIn dm(messages, message_len, n);
  LaneOut dout(out64, 64, n);
  hipLaunchKernelGGL(hmac_sha512_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, dkey.at<const sha512::HmacKey>(0),
                     dm.at<const uint8_t>(0), (uint32_t)message_len, n, dout.at<uint32_t>(0));
  finish(st);
  dout.down();
  ZK_API_END(ctx)
}

extern "C" int zkpoa_bip32_children(zkpoa_context* ctx, const uint8_t* parent_key33, const uint8_t* chain32, uint64_t first_index, uint64_t n,
                                    void* out_key33, void* out_chain32, void* out_pubkey_xy, void* out_address20, uint8_t* out_status) {
  ZK_API_BEGIN(ctx)
  children(ctx, parent_key33, chain32, first_index, n, out_key33, out_chain32, out_pubkey_xy, out_address20, out_status);
  ZK_API_END(ctx)
}

extern "C" int zkpoa_bip32_tweak(zkpoa_context* ctx, const uint8_t* parent_key33, uint64_t n, const void* tweaks32, void* out_key33,
                                 void* out_pubkey_xy, void* out_address20, uint8_t* out_status) {
  ZK_API_BEGIN(ctx)
  ctx->ms[kMsLaneBatch] = 0;
  if (!batch_wanted("bip32_tweak", "tweaks", n, parent_key33 && tweaks32 && out_key33 && out_pubkey_xy && out_address20 && out_status))
    return PROVER_OK;
  Parent par;
  make_parent("bip32_tweak", parent_key33, nullptr, par);
  hipStream_t st = ctx->dev.lanes[0].stream;
  LaneIn dtab(fixed_table_host(), sizeof(AffineK), kFixedEntries);
  LaneIn<SecretBuf> dpar(&par, sizeof(par), 1, st), dil(tweaks32, 32, n, st);
  memset(&par, 0, sizeof(par));
  TweakOut out(n, st, out_key33, out_pubkey_xy, out_address20, out_status);
  timed(ctx, st, kMsLaneBatch, [&] { out.launch(st, dpar.at<const Parent>(0), dil.at<const void>(0), nullptr, dtab.at<const AffineK>(0), n); });
  out.down();
  ZK_API_END(ctx)
}

extern "C" int zkpoa_bip32_master(const void* seed, uint64_t seed_len, uint8_t* out_key33, uint8_t* out_chain32) {
  if (!seed || !out_key33 || !out_chain32 || seed_len < 16 || seed_len > 64) return PROVER_ERROR;
  ZK_HOST_API_BEGIN
  sha512::HmacKey mac;
  sha512::hmac_key(reinterpret_cast<const uint8_t*>("Bitcoin seed"), 12, mac);
  const uint8_t* s = static_cast<const uint8_t*>(seed);
  uint64_t I[8];
  sha512::hmac_of(mac, [s](uint32_t j) -> uint32_t { return s[j]; }, (uint32_t)seed_len, I);
  uint8_t bytes[64];
  be_from_words(I, 8, bytes);
  Sc k;
  if (!private_key_of(bytes, k)) return PROVER_ERROR;
  out_key33[0] = 0;
  memcpy(out_key33 + 1, bytes, 32);
  memcpy(out_chain32, bytes + 32, 32);
  ZK_HOST_API_END
}

extern "C" int zkpoa_bip39_seed(const char* mnemonic, const char* passphrase, uint8_t* out_seed64) {
  if (!mnemonic || !out_seed64) return PROVER_ERROR;
  ZK_HOST_API_BEGIN
  // (the salt ends with the number of PBKDF2's block, 1: the only one, because dkLen = hLen)
  const std::string password = mnemonic, salt = std::string("mnemonic") + (passphrase ? passphrase : "") + std::string("\0\0\0\1", 4);
  if (password.size() > 4096 || salt.size() > 4096 + 12) return PROVER_ERROR;
  for (const std::string* s : {&password, &salt})
    for (const char c : *s)
      if ((unsigned char)c >= 0x80) return PROVER_ERROR;   // would need NFKD
  sha512::HmacKey mac;
  sha512::hmac_key(reinterpret_cast<const uint8_t*>(password.data()), (uint32_t)password.size(), mac);
  uint64_t u[8], acc[8], m[16];
  const uint8_t* sp = reinterpret_cast<const uint8_t*>(salt.data());
  sha512::hmac_of(mac, [sp](uint32_t j) -> uint32_t { return sp[j]; }, (uint32_t)salt.size(), u);
  for (int i = 0; i < 8; i++) acc[i] = u[i];
  for (int round = 1; round < 2048; round++) {
    sha512::pad_64(u, m);
    sha512::hmac_block(mac, m, u);
    for (int i = 0; i < 8; i++) acc[i] ^= u[i];
  }
  be_from_words(acc, 8, out_seed64);
  ZK_HOST_API_END
}

extern "C" int zkpoa_bip32_parse_key(const char* text, uint8_t* out_key33, uint8_t* out_chain32, uint32_t out_depth_index[2]) {
  if (!text || !out_key33 || !out_chain32 || !out_depth_index) return PROVER_ERROR;
  ZK_HOST_API_BEGIN
  uint8_t raw[82], check[32];
  if (!base58_decode(text, raw, sizeof(raw))) return PROVER_ERROR;
  sha256d(raw, 78, check);
  if (memcmp(check, raw + 78, 4) != 0) return PROVER_ERROR;
  const uint32_t version = ((uint32_t)raw[0] << 24) | ((uint32_t)raw[1] << 16) | ((uint32_t)raw[2] << 8) | raw[3];
  const uint8_t* key = raw + 45;
  if (version == 0x0488ADE4u) {
    Sc k;
    if (key[0] != 0 || !private_key_of(key + 1, k)) return PROVER_ERROR;
  } else if (version == 0x0488B21Eu) {
    AffineK K;
    if (!decompress(key, K)) return PROVER_ERROR;
  } else {
    return PROVER_ERROR;
  }
  memcpy(out_key33, key, 33);
  memcpy(out_chain32, raw + 13, 32);
  out_depth_index[0] = raw[4];
  out_depth_index[1] = ((uint32_t)raw[9] << 24) | ((uint32_t)raw[10] << 16) | ((uint32_t)raw[11] << 8) | raw[12];
  ZK_HOST_API_END
}

extern "C" int zkpoa_bip32_parse_path(const char* path, uint32_t* out_index, uint32_t* out_levels) {
  if (!path || !out_index || !out_levels) return PROVER_ERROR;
  ZK_HOST_API_BEGIN
  std::vector<uint32_t> levels;
  if (!parse_path(path, levels)) return PROVER_ERROR;
  for (size_t i = 0; i < levels.size(); i++) out_index[i] = levels[i];
  *out_levels = (uint32_t)levels.size();
  ZK_HOST_API_END
}

extern "C" int zkpoa_bip32_derive_path(zkpoa_context* ctx, const uint8_t* key33, const uint8_t* chain32, const char* path,
                                       uint8_t* out_key33, uint8_t* out_chain32) {
  ZK_API_BEGIN(ctx)
  if (!key33 || !chain32 || !path || !out_key33 || !out_chain32) throw HipError("bip32_derive_path: null argument");
  std::vector<uint32_t> levels;
  if (!parse_path(path, levels)) throw HipError(std::string("bip32_derive_path: not a path (m, m/0, m/44'/60'/0'/0; at most 255 levels): ") + path);
  uint8_t key[33], chain[32], pub[64], addr[20], status;
  memcpy(key, key33, 33);
  memcpy(chain, chain32, 32);
  for (const uint32_t index : levels) {
    if ((index & kHardened) && public_key_data(key)) throw HipError("bip32_derive_path: a hardened level under a public key");
    uint8_t next_key[33], next_chain[32];
    children(ctx, key, chain, index, 1, next_key, next_chain, pub, addr, &status);
    if (status) throw HipError("bip32_derive_path: child " + std::to_string(index & ~kHardened) + ((index & kHardened) ? "'" : "") + " is invalid");
    memcpy(key, next_key, 33);
    memcpy(chain, next_chain, 32);
  }
  if (levels.empty()) {   // "m": still has to be key data
    Parent par;
    make_parent("bip32_derive_path", key, nullptr, par);
    memset(&par, 0, sizeof(par));
  }
  memcpy(out_key33, key, 33);
  memcpy(out_chain32, chain, 32);
  ZK_API_END(ctx)
}
