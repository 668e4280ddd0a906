// Three modes of `ecdsa-sigs-parser`, the last node steps of the reference's workflow, host only:
//   layer-two-input    scripts/input_prep_for_layer_two.ts (full_workflow.sh:521-529): one batch's keys, their x-coordinate
//                      hash, the Merkle paths of its accounts and the layer-one proof -> the layer-two circuit's input
//   layer-three-input  scripts/input_prep_for_layer_three.ts (:575-579): the layer-two proofs side by side, their balance
//                      sums, the Merkle root and the Pedersen generators and blinding-factor bits
//   pedersen-check     scripts/pedersen_commitment_checker.ts (:588-591): balance sum * G + blinding factor * H against
//                      the point in layer three's public signals
// and what they share with layer-one-input: the batch range, the {"__bigint__": ...} reader, the limb writer. The files
// are read through the pull parser; of the parsed-signatures file and of merkle_proofs.json, gigabytes at 2^20
// signatures, only the entries of the batch are converted. The outputs are the text JSON.stringify(..., 2) writes, byte
// for byte, and appear only when complete. No function here touches the GPU.
#pragma once
#include "host_files.hpp"
#include "host_text.hpp"
#include "pedersen_host.hpp"
#include "poseidon_host.hpp"

#include <algorithm>

namespace zkpoa {
namespace layer_inputs {

struct InputError : std::runtime_error {
  explicit InputError(const std::string& m) : std::runtime_error(m) {}
};

inline U256 parse_number(const Span& s, const char* what) {   // decimal or 0x hex, below 2^256
  U256 x;
  if (!x.parse_number(s.b, s.e)) throw InputError(std::string(what) + " is not a number below 2^256: " + s.str());
  return x;
}

inline std::string entry(uint64_t i) { return "entry " + std::to_string(i) + ": "; }

inline U256 read_bigint(Json& js, const char* what) {
  U256 out;
  bool seen = false;
  js.object([&](const Span& k) {
    if (k.is("__bigint__")) {
      out = parse_number(js.string(), what);
      seen = true;
    } else {
      js.skip();
    }
  });
  if (!seen) throw InputError(std::string(what) + " is not a {\"__bigint__\": ...} object");
  return out;
}

inline void put_limbs(std::string& o, const char* indent, const U256& x, bool last) {
  o += indent;
  o += "[\n";
  for (int k = 0; k < 4; k++) {
    o += indent;
    o += "  \"" + std::to_string((unsigned long long)x.v[k]) + (k < 3 ? "\",\n" : "\"\n");
  }
  o += indent;
  o += last ? "]\n" : "],\n";
}

// --account-start-index / --account-end-index as the reference's scripts use them: array.slice(start, end)
struct BatchRange {
  long long start = 0, end = -1;
  // can slice(start, end) reach element i, whatever the array's length? (decided while the array is still being read)
  bool reaches(uint64_t i) const { return !((start >= 0 && (long long)i < start) || (end >= 0 && (long long)i >= end)); }
  long long first_kept() const { return start > 0 ? start : 0; }   // the first element reaches() lets through
  // once the number of attestations is known: -1 is "all of them", and the reference's one range check
  void close(long long len) {
    if (end == -1) {
      printf("Batch contains all input data i.e. there is only 1 batch\n");
      end = len;
    }
    if (start >= end) throw InputError("startIndex " + std::to_string(start) + " must be less than endIndex " + std::to_string(end));
  }
  // Array.prototype.slice: a negative index counts from the end, both are clamped to [0, length]
  void slice(long long len, long long& lo, long long& hi) const {
    lo = std::min(len, start < 0 ? std::max(0ll, len + start) : start);
    hi = std::max(lo, std::min(len, end < 0 ? std::max(0ll, len + end) : end));
  }
};

// The accountAttestations of a parsed-signatures file: entry(js, i) reads element i; the elements the range cannot reach
// are skipped unread (BatchRange(): none is). -> the array's length
template <class Fn>
long long for_each_attestation(const std::string& path, const BatchRange& range, Fn entry) {
  MappedFile text(path.c_str());
  Json js{text.begin(), text.end()};
  long long total = 0;
  bool seen = false;
  js.object([&](const Span& key) {
    if (!key.is("accountAttestations")) return js.skip();
    seen = true;
    js.array([&](uint64_t i) {
      total = (long long)i + 1;
      if (!range.reaches(i)) return js.skip();
      entry(js, i);
    });
  });
  js.end();
  if (!seen) throw InputError("no accountAttestations in " + path);
  return total;
}

// ---- JSON.stringify(value, null, 2) of a value as it stands in a file: the layout changes, scalars are copied -------
inline void restyle(Json& js, std::string& o, const std::string& indent) {
  if (js.at('[')) {
    const uint64_t n = js.array([&](uint64_t i) {
      o += i ? ",\n" : "[\n";
      o += indent + "  ";
      restyle(js, o, indent + "  ");
    });
    o += n ? "\n" + indent + "]" : "[]";
  } else if (js.at('{')) {
    bool any = false;
    js.object([&](const Span& key) {
      o += any ? ",\n" : "{\n";
      o += indent + "  \"" + key.str() + "\": ";
      restyle(js, o, indent + "  ");
      any = true;
    });
    o += any ? "\n" + indent + "}" : "{}";
  } else {
    js.ws();
    const char* b = js.p;
    js.skip();
    o.append(b, js.p);
  }
}

// ---- layer-two-input -----------------------------------------------------------------------------------------------
struct Account {
  U256 x, y, address, balance;
};

// accountAttestations[i].signature.pubkey.{x, y} and .accountData.{address, balance} of the entries the range reaches;
// -> the array's length
inline long long read_accounts(const std::string& path, const BatchRange& range, std::vector<Account>& kept) {
  return for_each_attestation(path, range, [&](Json& js, uint64_t i) {
    Account a;
    unsigned have = 0;
    js.object([&](const Span& k1) {
      if (k1.is("signature")) {
        js.object([&](const Span& k2) {
          if (!k2.is("pubkey")) return js.skip();
          js.object([&](const Span& k3) {
            if (k3.is("x")) a.x = read_bigint(js, "pubkey.x"), have |= 1u;
            else if (k3.is("y")) a.y = read_bigint(js, "pubkey.y"), have |= 2u;
            else js.skip();
          });
        });
      } else if (k1.is("accountData")) {
        js.object([&](const Span& k2) {
          if (k2.is("address")) a.address = read_bigint(js, "accountData.address"), have |= 4u;
          else if (k2.is("balance")) a.balance = read_bigint(js, "accountData.balance"), have |= 8u;
          else js.skip();
        });
      } else {
        js.skip();
      }
    });
    if (have != 15u) throw InputError(entry(i) + "needs signature.pubkey.{x, y} and accountData.{address, balance}");
    kept.push_back(a);
  });
}

struct ProofsSlice {
  std::vector<U256> leaf_address;
  std::string path_elements, path_indices;   // as they stand in the output, from "[" to "]"
};

// The slices of merkle_proofs.json's three arrays; elements the range cannot reach are skipped unconverted.
inline void read_merkle_proofs(const std::string& path, const BatchRange& range, ProofsSlice& out) {
  MappedFile text(path.c_str());
  Json js{text.begin(), text.end()};
  unsigned seen = 0;
  // one array: keep(i, k) converts element i as the k-th it keeps; then slice() by the array's own length
  auto sliced = [&](auto keep, auto drop_front, auto drop_back) {
    uint64_t kept = 0;
    const long long len = (long long)js.array([&](uint64_t i) {
      if (!range.reaches(i)) return js.skip();
      keep(i, kept++);
    });
    long long lo, hi;
    range.slice(len, lo, hi);
    // reaches() lets through [first_kept, ...): slice() may want fewer at either end (a negative index)
    const long long front = lo - range.first_kept(), count = hi - lo;
    if (front > 0) drop_front((uint64_t)front);
    drop_back((uint64_t)std::max(0ll, count));
  };
  js.object([&](const Span& key) {
    if (key.is("leaves")) {
      seen |= 1u;
      sliced(
          [&](uint64_t i, uint64_t) {
            bool have = false;
            js.object([&](const Span& k) {
              if (!k.is("address")) return js.skip();
              out.leaf_address.push_back(read_bigint(js, "leaves[].address"));
              have = true;
            });
            if (!have) throw InputError("merkle proofs: leaf " + std::to_string(i) + " has no address");
          },
          [&](uint64_t front) { out.leaf_address.erase(out.leaf_address.begin(), out.leaf_address.begin() + (long)front); },
          [&](uint64_t count) { out.leaf_address.resize(std::min<uint64_t>(count, out.leaf_address.size())); });
    } else if (key.is("path_elements") || key.is("path_indices")) {
      const bool elements = key.b[5] == 'e';
      seen |= elements ? 2u : 4u;
      std::vector<std::string> rows;
      sliced(
          [&](uint64_t, uint64_t) {
            std::string row;
            const uint64_t n = js.array([&](uint64_t l) {
              row += l ? ",\n      " : "[\n      ";
              if (elements) {
                row += "\"" + read_bigint(js, "path_elements[][]").dec() + "\"";
              } else {
                js.ws();
                const char* b = js.p;
                js.skip();
                row.append(b, js.p);
              }
            });
            row += n ? "\n    ]" : "[]";
            rows.push_back(row);
          },
          [&](uint64_t front) { rows.erase(rows.begin(), rows.begin() + (long)front); },
          [&](uint64_t count) { rows.resize(std::min<uint64_t>(count, rows.size())); });
      std::string& o = elements ? out.path_elements : out.path_indices;
      o = rows.empty() ? "[]" : "[";
      for (size_t i = 0; i < rows.size(); i++) o += (i ? ",\n    " : "\n    ") + rows[i];
      if (!rows.empty()) o += "\n  ]";
    } else {
      js.skip();
    }
  });
  js.end();
  if (seen != 7u) throw InputError("merkle proofs: " + path + " needs leaves, path_elements and path_indices");
}

inline U256 read_bigint_file(const std::string& path, const char* what) {
  MappedFile text(path.c_str());
  Json js{text.begin(), text.end()};
  const U256 v = read_bigint(js, what);
  js.end();
  return v;
}

// the x coordinates as 4 x 64-bit limbs each, least significant first, through the sponge
inline U256 x_coords_hash(const std::vector<Account>& acc, uint64_t lo, uint64_t count) {
  std::vector<HFr> in(4 * count);
  for (uint64_t i = 0; i < count; i++)
    for (int k = 0; k < 4; k++) in[4 * i + k] = HFr::from_u64(acc[lo + i].x.v[k]);
  const HFr h = poseidon_sponge(in.data(), in.size()).from_mont();
  U256 out;
  memcpy(out.v, h.l, 32);
  return out;
}

// checkAddressOrdering (input_prep_for_layer_two.ts:127-153)
inline void check_address_ordering(const std::vector<Account>& acc, uint64_t lo, uint64_t count, const std::vector<U256>& leaves) {
  printf("Checking that the order of addresses in input data & Merkle proofs is the same..\n");
  if (count != leaves.size())
    throw InputError("Length of input data array " + std::to_string(count) + " should equal length of merkle proofs array " +
                     std::to_string(leaves.size()));
  for (uint64_t i = 0; i < count; i++) {
    const U256 &a = acc[lo + i].address, &m = leaves[i];
    if (memcmp(a.v, m.v, 32) != 0)
      throw InputError("[i = " + std::to_string(i) + "] Address in input data array " + a.dec() + " should equal address in merkle proofs array " +
                       m.dec());
    if (i > 0) {
      const U256& prev = leaves[i - 1];
      if (m.below(prev.v))
        throw InputError("Addresses must be in ascending order, but address at i=" + std::to_string(i) + " (" + m.dec() +
                         ") is less than the previous address (" + prev.dec() + ")");
      if (memcmp(m.v, prev.v, 32) == 0)
        throw InputError("Cannot have duplicate addresses, but address at i=" + std::to_string(i) + " (" + m.dec() +
                         ") is the same as the previous address (" + prev.dec() + ")");
    }
  }
}

struct LayerTwoPaths {
  std::string input, merkle_root, merkle_proofs, hash_out, layer_one_proof, out;
};

inline int layer_two_mode(const LayerTwoPaths& p, BatchRange range) {
  PhaseTimer lap("layer-two-input", 8);
  std::vector<Account> acc;   // entries first_kept, first_kept + 1, ...
  const long long len = read_accounts(p.input, range, acc);
  lap("read");
  printf("Preparing input for layer 2 using the following data:\n- System input: %s\n- Start index for batch: %lld\n"
         "- End index for batch: %lld\n- Merkle proofs path: %s\n- Merkle root path: %s\nPath to write processed data to: %s\n"
         "Path to write public keys hash to: %s\n\n",
         p.input.c_str(), range.start, range.end, p.merkle_proofs.c_str(), p.merkle_root.c_str(), p.out.c_str(), p.hash_out.c_str());
  const long long first_kept = range.first_kept();
  range.close(len);
  long long lo, hi;
  range.slice(len, lo, hi);
  const uint64_t m = (uint64_t)(hi - lo), at = (uint64_t)(lo - first_kept);
  if (m == 0) throw InputError("the batch [" + std::to_string(range.start) + ", " + std::to_string(range.end) + ") holds no account of the " +
                               std::to_string(len) + " in " + p.input);
  const std::string hash = x_coords_hash(acc, at, m).dec();
  lap("hash");
  printf("Hash of public keys x-coords: %s\n", hash.c_str());
  const U256 root = read_bigint_file(p.merkle_root, "the Merkle root");
  ProofsSlice proofs;
  read_merkle_proofs(p.merkle_proofs, range, proofs);
  lap("proofs");
  std::string o = "{\n";
  {
    MappedFile text(p.layer_one_proof.c_str());
    Json js{text.begin(), text.end()};
    js.object([&](const Span& key) {
      if (key.is("pubInput")) return js.skip();
      o += "  \"" + key.str() + "\": ";
      restyle(js, o, "  ");
      o += ",\n";
    });
    js.end();
  }
  check_address_ordering(acc, at, m, proofs.leaf_address);
  o += "  \"pubkey_x_coord_hash\": \"" + hash + "\",\n  \"pubkey\": [\n";
  for (uint64_t i = 0; i < m; i++) {
    o += "    [\n";
    put_limbs(o, "      ", acc[at + i].x, false);
    put_limbs(o, "      ", acc[at + i].y, true);
    o += i + 1 < m ? "    ],\n" : "    ]\n";
  }
  o += "  ],\n";
  for (int f = 0; f < 2; f++) {
    o += f ? "  \"leaf_balances\": [\n" : "  \"leaf_addresses\": [\n";
    for (uint64_t i = 0; i < m; i++) o += "    \"" + (f ? acc[at + i].balance : acc[at + i].address).dec() + (i + 1 < m ? "\",\n" : "\"\n");
    o += "  ],\n";
  }
  o += "  \"merkle_root\": \"" + root.dec() + "\",\n  \"path_elements\": " + proofs.path_elements + ",\n  \"path_indices\": " +
       proofs.path_indices + "\n}";
  // both outputs only now that nothing can fail but the writing itself (the reference writes the hash before its
  // checks); every batch job of the workflow writes the same hash path, so that file too goes in whole or not at all
  write_text_atomic(p.out, o);
  write_text_atomic(p.hash_out, hash);
  lap("write");
  return 0;
}

// ---- layer-three-input ---------------------------------------------------------------------------------------------
constexpr uint64_t kTwo255Limb3 = 1ull << 63;

inline U256 parse_blinding_factor(const std::string& text) {   // BigInt(string): decimal or 0x hex
  U256 x;
  if (!x.parse_number(text.data(), text.data() + text.size()))
    throw InputError("--blindingFactor is not a decimal or 0x-hex number below 2^256: " + text);
  return x;
}

inline int layer_three_mode(const std::string& root_path, const std::string& proof_paths, const std::string& out_path,
                            const std::string& blinding_text) {
  static const char* const kKeys[7] = {"gamma2", "delta2", "negalfa1xbeta2", "IC", "negpa", "pb", "pc"};
  const U256 blinding = parse_blinding_factor(blinding_text);
  // formatScalarPower keeps 255 bits: from 2^255 on it drops bit 255 (or returns 264 bits), and the circuit would commit
  // with another factor than the one the Pedersen check is given
  if (blinding.v[3] & kTwo255Limb3)
    throw InputError("the blinding factor " + blinding.dec() + " is not below 2^255: the layer-three circuit takes 255 bits of it");
  const U256 root = read_bigint_file(root_path, "the Merkle root");
  std::vector<std::string> paths;
  for (size_t b = 0;;) {
    const size_t c = proof_paths.find(',', b);
    paths.push_back(proof_paths.substr(b, c == std::string::npos ? c : c - b));
    if (c == std::string::npos) break;
    b = c + 1;
  }
  std::vector<std::string> parts[7];   // parts[k][i]: proof i's value of key k, laid out two levels in
  std::vector<std::string> balances;
  for (const std::string& path : paths) {
    struct stat sb;
    if (lstat(path.c_str(), &sb) != 0) throw InputError("cannot open " + path);
    if (!S_ISREG(sb.st_mode)) throw InputError("Expected " + path + " to be a path to a file");
    const size_t dot = path.rfind('.');
    if (path.substr(dot == std::string::npos ? 0 : dot + 1) != "json") throw InputError("Expected " + path + " to be a path to a json file");
    MappedFile text(path.c_str());
    Json js{text.begin(), text.end()};
    unsigned have = 0;
    std::string balance;
    js.object([&](const Span& key) {
      for (int k = 0; k < 7; k++)
        if (key.is(kKeys[k])) {
          std::string o;
          restyle(js, o, "    ");
          parts[k].push_back(o);
          have |= 1u << k;
          return;
        }
      if (!key.is("pubInput")) return js.skip();
      js.array([&](uint64_t i) {
        if (i) return js.skip();
        if (js.at('"')) throw InputError(path + ": pubInput[0] is a string, not a number");
        balance = js.number().str();
        have |= 128u;
      });
    });
    js.end();
    if (have != 255u) throw InputError(path + " needs gamma2, delta2, negalfa1xbeta2, IC, negpa, pb, pc and pubInput");
    // JSON.parse holds a number as a double: from 2^53 on the balance sum written out would be a rounded one
    U256 v;
    bool digits = !balance.empty() && (balance.size() == 1 || balance[0] != '0');
    for (char ch : balance) digits = digits && ch >= '0' && ch <= '9';
    if (!digits || !v.parse_dec(balance.data(), balance.data() + balance.size()) || v.v[1] || v.v[2] || v.v[3] || v.v[0] >= (1ull << 53))
      throw InputError(path + ": pubInput[0] = " + balance + " is not an integer below 2^53: the reference's JSON number would round it");
    balances.push_back(balance);
  }
  std::string joined;
  for (size_t i = 0; i < balances.size(); i++) joined += (i ? "," : "") + balances[i];
  printf("Preparing input for layer 3 using the following data:\n- Merkle root: %s\n- Blinding factor: %s\n"
         "- Balances (layer 2 output): %s\nPath to write processed data to: %s\n\n",
         root.dec().c_str(), blinding.dec().c_str(), joined.c_str(), out_path.c_str());
  std::string o = "{\n";
  for (int k = 0; k < 7; k++) {
    o += std::string("  \"") + kKeys[k] + "\": [\n";
    for (size_t i = 0; i < parts[k].size(); i++) o += "    " + parts[k][i] + (i + 1 < parts[k].size() ? ",\n" : "\n");
    o += "  ],\n";
  }
  o += "  \"balances\": [\n";
  for (size_t i = 0; i < balances.size(); i++) o += "    " + balances[i] + (i + 1 < balances.size() ? ",\n" : "\n");
  o += "  ],\n  \"merkle_root\": \"" + root.dec() + "\",\n";
  for (int g = 0; g < 2; g++) {
    const EdPoint& pt = g ? pedersen_generator_h() : pedersen_generator_g();
    const U256* coord[4] = {&pt.x, &pt.y, &pt.z, &pt.t};
    o += g ? "  \"ped_com_generator_h\": [\n" : "  \"ped_com_generator_g\": [\n";
    for (int c = 0; c < 4; c++) {
      U256 ch[3];
      chunks85(*coord[c], ch);
      o += "    [\n";
      for (int k = 0; k < 3; k++) o += "      \"" + ch[k].dec() + (k < 2 ? "\",\n" : "\"\n");
      o += c < 3 ? "    ],\n" : "    ]\n";
    }
    o += "  ],\n";
  }
  o += "  \"ped_com_blinding_factor\": [\n";
  for (int b = 0; b < 255; b++) o += std::string("    \"") + (((blinding.v[b >> 6] >> (b & 63)) & 1) ? "1" : "0") + (b < 254 ? "\",\n" : "\"\n");
  o += "  ]\n}";
  write_text_atomic(out_path, o);
  return 0;
}

// ---- pedersen-check ------------------------------------------------------------------------------------------------
inline int pedersen_check_mode(const std::string& input_path, const std::string& public_path, const std::string& blinding_text) {
  const U256 blinding = parse_blinding_factor(blinding_text);
  U256 sum;
  for_each_attestation(input_path, BatchRange(), [&](Json& js, uint64_t i) {
    bool have = false;
    js.object([&](const Span& k1) {
      if (!k1.is("accountData")) return js.skip();
      js.object([&](const Span& k2) {
        if (!k2.is("balance")) return js.skip();
        const U256 b = read_bigint(js, "accountData.balance");
        unsigned __int128 c = 0;
        for (int k = 0; k < 4; k++) {
          c += (unsigned __int128)sum.v[k] + b.v[k];
          sum.v[k] = (uint64_t)c;
          c >>= 64;
        }
        if (c) throw InputError("the balance sum is not below 2^256");
        have = true;
      });
    });
    if (!have) throw InputError(entry(i) + "needs accountData.balance");
  });
  U256 signals[12];
  {
    MappedFile text(public_path.c_str());
    Json js{text.begin(), text.end()};
    const uint64_t n = js.array([&](uint64_t i) {
      if (i >= 12) return js.skip();
      signals[i] = parse_number(js.scalar(), "a public signal");
    });
    js.end();
    if (n < 12) throw InputError(public_path + " holds " + std::to_string(n) + " public signals; the commitment is the first 12");
  }
  printf("Balance sum calculated from input data: %s\nBlinding factor given: %s\n", sum.dec().c_str(), blinding.dec().c_str());
  if (!ed_equal(pedersen_commit(sum, blinding), pedersen_dechunk(signals)))
    throw InputError("the Pedersen commitment of this balance sum and blinding factor is not the one in " + public_path);
  return 0;
}

}  // namespace layer_inputs
}  // namespace zkpoa
