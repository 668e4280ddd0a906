// Host check of the secp256k1 layer function by function: the ZK_HD text of csrc/secp256k1.hip.h (Fp, Sc, recode_signed4,
// to_affine, fixed_mul, double_mul, recover_one) compiled for the CPU, with the sanitizers on, and driven by lines on
// stdin. tests/test_secp_prim_host.py builds it, feeds it the operand sets and ladder cases of tests/secp_limb_ref.py and
// compares every answer with big integers. No GPU, no HIP call.
// Build: hipcc -x hip --offload-host-only -O0 -g -std=c++17 -Xarch_host -fsanitize=address,undefined
//              -Xarch_host -fno-sanitize-recover=all -I zk-proof-of-assets_amd/csrc tools/secp_prim_check.cpp -o secp_prim_check
// Lines in (integers as 64 hex digits, big-endian; taken and printed raw, no range fix-up) -> line out
//   <op> <operands>                  the ops of zkpoa_secp_prim (include/zkpoa_secp_prim.h) by number, the same operands and
//                                    results: 8-word values as 64 hex digits, extra words as 8 hex digits each
//   recover <r> <s> <z> <v> <address, 40 hex digits> -> <status> <r'> <x> <y> <address>
//                                    recover_one, the lane's table over host memory at stride 1
#include "secp256k1.hip.h"

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace zkpoa;
using namespace zkpoa::secp;

static std::vector<uint8_t> bytes_of(const std::string& hex) {
  std::vector<uint8_t> out;
  for (size_t i = 0; i + 1 < hex.size(); i += 2) out.push_back((uint8_t)std::stoul(hex.substr(i, 2), nullptr, 16));
  return out;
}
static void limbs_of(const std::string& hex, uint32_t (&l)[8]) {
  const std::vector<uint8_t> b = bytes_of(hex);
  if (b.size() != 32) throw std::runtime_error("an integer is 64 hex digits: " + hex);
  load_be32(b.data(), 0, l);   // (a vector's storage is aligned for words)
}
static std::string hex_of(const uint8_t* b, size_t n) {
  static const char digits[] = "0123456789abcdef";
  std::string o;
  for (size_t i = 0; i < n; i++) {
    o.push_back(digits[b[i] >> 4]);
    o.push_back(digits[b[i] & 15]);
  }
  return o;
}
static std::string hex_of(const uint32_t (&l)[8]) {
  alignas(4) uint8_t b[32];
  store_be32(b, 0, l);
  return hex_of(b, 32);
}
static std::string word_of(uint32_t w) {
  const uint8_t b[4] = {(uint8_t)(w >> 24), (uint8_t)(w >> 16), (uint8_t)(w >> 8), (uint8_t)w};
  return hex_of(b, 4);
}
static std::string xyzz_of(const XyzzK& p) { return hex_of(p.x.l) + " " + hex_of(p.y.l) + " " + hex_of(p.zz.l) + " " + hex_of(p.zzz.l); }

int main() {
  std::vector<AffineK> ftab(kFixedEntries);
  fixed_base_table(ftab.data());
  AffineK gtab[8];
  generator_table(gtab);
  std::vector<uint32_t> table(8 * 32);   // one lane's 1R .. 8R
  const LaneTable lt{table.data(), 1};
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    in >> op;
    if (op.empty()) continue;
    if (op == "recover") {
      std::string a, b, c, addr;
      uint32_t v = 0;
      in >> a >> b >> c >> v >> addr;
      uint32_t r[8], s[8], z[8];
      limbs_of(a, r);
      limbs_of(b, s);
      limbs_of(c, z);
      const std::vector<uint8_t> ab = bytes_of(addr);
      if (ab.size() != 20) throw std::runtime_error("an address is 40 hex digits: " + addr);
      uint32_t given[5];
      for (int i = 0; i < 5; i++) given[i] = ab[4 * i] | (ab[4 * i + 1] << 8) | (ab[4 * i + 2] << 16) | ((uint32_t)ab[4 * i + 3] << 24);
      const Recovered g = recover_one(r, s, z, v, given, gtab, lt);
      std::cout << g.status << " " << hex_of(g.r_prime.l) << " " << hex_of(g.q.x.l) << " " << hex_of(g.q.y.l) << " "
                << hex_of(reinterpret_cast<const uint8_t*>(g.addr), 20) << "\n";
      continue;
    }
    secp::Fp f[4];
    secp::Sc k[4];
    int given = 0;
    for (std::string a; given < 4 && in >> a; given++) {
      limbs_of(a, f[given].l);
      limbs_of(a, k[given].l);
    }
    const int code = std::stoi(op);
    const int wanted = (code == 0 || code == 2 || code == 3 || code == 9 || code == 10) ? 2 : (code == 18 || code == 20) ? 4 : 1;
    if (code < 0 || code > 20 || given != wanted) {
      std::cerr << "unknown line: " << line << "\n";
      return 2;
    }
    switch (code) {
      case 0: std::cout << hex_of((f[0] * f[1]).l); break;
      case 1: std::cout << hex_of(f[0].sqr().l); break;
      case 2: std::cout << hex_of((f[0] + f[1]).l); break;
      case 3: std::cout << hex_of((f[0] - f[1]).l); break;
      case 4: std::cout << hex_of(f[0].neg().l); break;
      case 5: std::cout << hex_of(f[0].dbl().l); break;
      case 6: std::cout << hex_of(f[0].inv().l); break;
      case 7: std::cout << hex_of(f[0].sqrt_candidate().l); break;
      case 8: std::cout << word_of(f[0].ge_p() ? 1u : 0u); break;
      case 9: std::cout << hex_of((k[0] * k[1]).l); break;
      case 10: std::cout << hex_of(sc_add(k[0], k[1]).l); break;
      case 11: std::cout << hex_of(k[0].neg().l); break;
      case 12: std::cout << hex_of(k[0].inv().l); break;
      case 13: std::cout << hex_of(k[0].reduce_once().l); break;
      case 14: std::cout << hex_of(key_from_hash(k[0].l).l); break;
      case 15: std::cout << word_of(k[0].ge_n() ? 1u : 0u); break;
      case 16: std::cout << word_of(k[0].is_high() ? 1u : 0u); break;
      case 17: {
        uint32_t mag[8];
        uint64_t sgn;
        recode_signed4(k[0].l, mag, sgn);
        std::cout << hex_of(mag) << " " << word_of((uint32_t)sgn) << " " << word_of((uint32_t)(sgn >> 32));
        break;
      }
      case 18: {
        const AffineK a = to_affine(XyzzK{f[0], f[1], f[2], f[3]});
        std::cout << hex_of(a.x.l) << " " << hex_of(a.y.l);
        break;
      }
      case 19: std::cout << xyzz_of(fixed_mul(k[0], ftab.data())); break;
      default: {
        const XyzzK q = double_mul(AffineK{f[0], f[1]}, k[2], k[3], gtab, lt);
        std::cout << xyzz_of(q) << " " << word_of(q.is_inf() ? 1u : 0u);
        break;
      }
    }
    std::cout << "\n";
  }
  return 0;
}
