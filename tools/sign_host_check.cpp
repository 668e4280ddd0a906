// Host check of the signing path: the ZK_HD text of csrc/sha256.hip.h and csrc/secp256k1.hip.h (SHA-256, HMAC, the RFC
// 6979 generator, the fixed-base table and multiplication, public keys, signatures, derived keys) compiled for the CPU,
// with the sanitizers on, and driven by lines on stdin. tests/test_sign_host.py builds it, feeds it the edge cases of
// tests/test_gpu_ecdsa_sign.py and compares every answer with tests/sign_ref.py. No GPU, no HIP call.
// Build: hipcc -x hip --offload-host-only -O0 -g -std=c++17 -Xarch_host -fsanitize=address,undefined
//              -Xarch_host -fno-sanitize-recover=all -I zk-proof-of-assets_amd/csrc tools/sign_host_check.cpp -o sign_host_check
// Lines in (integers as 64 hex digits, big-endian)    -> line out
//   sign <key> <hash>          -> <status> <r> <s> <v> <x> <y> <address, 40 hex digits>
//   pub <key>                  -> <status> <x> <y> <address>
//   nonce <key> <hash> <skip>  -> <k>
//   sha <message in hex, or -> -> <digest>
//   key <seed in hex, or -> <index> -> <key>
#include "secp256k1.hip.h"

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace zkpoa;
using namespace zkpoa::secp;

static std::vector<uint8_t> bytes_of(const std::string& hex) {
  std::vector<uint8_t> out;
  if (hex == "-") return out;
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
static std::string address_of(const uint32_t (&a)[5]) { return hex_of(reinterpret_cast<const uint8_t*>(a), 20); }

int main() {
  std::vector<AffineK> ftab(kFixedEntries);
  fixed_base_table(ftab.data());
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op, a, b;
    in >> op;
    if (op.empty()) continue;
    if (op == "sign") {
      in >> a >> b;
      uint32_t d[8], z[8];
      limbs_of(a, d);
      limbs_of(b, z);
      const Signed g = sign_one(d, z, ftab.data());
      std::cout << g.status << " " << hex_of(g.r.l) << " " << hex_of(g.s.l) << " " << g.v << " " << hex_of(g.q.x.l) << " " << hex_of(g.q.y.l) << " "
                << address_of(g.addr) << "\n";
    } else if (op == "pub") {
      in >> a;
      uint32_t d[8];
      limbs_of(a, d);
      const PublicKey g = public_key(d, ftab.data());
      std::cout << g.status << " " << hex_of(g.q.x.l) << " " << hex_of(g.q.y.l) << " " << address_of(g.addr) << "\n";
    } else if (op == "nonce") {
      int skip = 0;
      in >> a >> b >> skip;
      uint32_t d[8], z[8], k[8];
      limbs_of(a, d);
      limbs_of(b, z);
      rfc6979_candidate(d, z, skip, k);
      std::cout << hex_of(k) << "\n";
    } else if (op == "sha") {
      in >> a;
      const std::vector<uint8_t> m = bytes_of(a);
      uint32_t h[8], l[8];
      sha256::digest(m.data(), (uint32_t)m.size(), h);
      be_words(h, l);
      std::cout << hex_of(l) << "\n";
    } else if (op == "key") {
      unsigned long long index = 0;
      in >> a >> index;
      const std::vector<uint8_t> seed = bytes_of(a);
      std::cout << hex_of(derive_key(seed.data(), (uint32_t)seed.size(), index).l) << "\n";
    } else {
      std::cerr << "unknown line: " << line << "\n";
      return 2;
    }
  }
  return 0;
}
