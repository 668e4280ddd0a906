// `ecdsa-sigs-parser` -- stands in for five TypeScript steps of the reference's workflow, and (sign, anon-set: further
// down) for the two test scripts that make the workflow's first two files:
//   ecdsa-sigs-parser --signatures <in.json> --output-path <out.json>             scripts/ecdsa_sigs_parser.ts
//       (full_workflow.sh:354-357): ECDSA signatures -> ECDSA* attestations. Recovery, r', Keccak and the address
//       comparison run on the GPU (zkpoa_ecdsa_star, zkpoa_eth_address); the output is the text that
//       JSON.stringify(outputData, jsonReplacer, 2) writes, byte for byte, and appears only when complete.
//   ecdsa-sigs-parser layer-one-input -i <parsed.json> -o <out.json> [-s start] [-e end]
//       scripts/input_prep_for_layer_one.ts (full_workflow.sh:497-501): host only, the signatures of one batch as
//       4 x 64-bit limbs.
//   ecdsa-sigs-parser layer-two-input | layer-three-input | pedersen-check ...
//       the workflow's last three node steps (full_workflow.sh:521-529, :575-579, :588-591), host only: this file only
//       reads their options and hands over to layer_inputs.hpp, which also holds what layer-one-input shares with them.
//   ecdsa-sigs-parser hd-list <HD source> -o <addresses.csv>
//       no counterpart in the reference: the addresses of a BIP-32 wallet's children (include/zkpoa_hd_wallet.h), the
//       watch-only listing; the same HD source is a key source of sign and anon-set.
// Both files are read through a pull parser over the mapped text: a million signatures are 350 MB of JSON in and over
// a gigabyte out, and neither is ever held as a tree. The output is formatted by the host threads 2^16 entries at a
// time. Exit status 0, or 1 with one line on stderr and no output file.
#include "../../include/zkpoa_prover.h"
#include "host_files.hpp"
#include "host_text.hpp"
#include "layer_inputs.hpp"

#include <algorithm>
#include <map>

using namespace zkpoa;
using namespace zkpoa::layer_inputs;

namespace {

// "0x" + 1..64 hex digits -> 32 bytes, big-endian, padded on the left
bool parse_hex_u256(const Span& s, uint8_t* out) {
  U256 x;
  if (s.size() < 3 || s.size() > 66 || s.b[0] != '0' || s.b[1] != 'x' || !x.parse_hex(s.b + 2, s.e)) return false;
  x.to_be(out);
  return true;
}

// all of the text is a decimal integer (strtoll's: out of range gives the nearest end of the range)
bool parse_integer(const std::string& t, long long& out) {
  char* rest = nullptr;
  out = strtoll(t.c_str(), &rest, 10);
  return rest != t.c_str() && !*rest;
}

// ---- the command line: the reference's option names, long (--name value, --name=value) and short -------------------
// What is wrong with a command line: its spelling (an unknown option, a value that is missing or no number, options that
// do not go together), or a required option that is absent. How a mode answers either is in the table of modes.
struct CliError : std::runtime_error {
  bool absent;
  explicit CliError(const std::string& m, bool absent_ = false) : std::runtime_error(m), absent(absent_) {}
};
struct Option {
  const char *name, *alt;   // "--poa-input-data", "-i"
};
struct Cli {
  const char* mode;
  std::map<std::string, std::string> got;   // by the long name
  bool has(const char* name) const { return got.count(name) != 0; }
  const std::string& value(const char* name) const {   // "" when not given
    static const std::string none;
    const auto it = got.find(name);
    return it == got.end() ? none : it->second;
  }
  const std::string& required(const char* name) const {
    if (value(name).empty()) throw CliError(std::string(mode) + " needs " + name + " <value>", true);
    return value(name);
  }
  long long integer(const char* name, long long otherwise) const {
    long long v = otherwise;
    if (has(name) && !parse_integer(value(name), v)) throw CliError(std::string(name) + " is not an integer");
    return v;
  }
  // a number of things, least .. 2^32, written as at most ten digits and nothing else
  uint64_t count(const char* name, long long least, const char* complaint) const {
    const std::string& s = value(name);
    long long v;
    if (s.size() > 10 || s.find_first_not_of("0123456789") != std::string::npos || !parse_integer(s, v) || v < least || v > (1ll << 32))
      throw CliError(std::string(name) + " is not a number of " + complaint);
    return (uint64_t)v;
  }
  BatchRange batch_range() const {
    BatchRange range;
    range.start = integer("--account-start-index", 0);
    range.end = integer("--account-end-index", -1);
    return range;
  }
};
// help: -h / --help end the reading and are reported as "--help"
Cli parse_options(int argc, char** argv, int first, const char* mode, const std::vector<Option>& known, bool help) {
  Cli cli{mode, {}};
  for (int i = first; i < argc; i++) {
    std::string a = argv[i], val;
    bool has = false;
    const size_t eq = a.find('=');
    if (a.rfind("--", 0) == 0 && eq != std::string::npos) {
      val = a.substr(eq + 1);
      a = a.substr(0, eq);
      has = true;
    }
    if (help && (a == "-h" || a == "--help")) {
      cli.got["--help"];
      return cli;
    }
    const Option* opt = nullptr;
    for (const Option& k : known)
      if (a == k.name || (k.alt && a == k.alt)) opt = &k;
    if (!opt) throw CliError("unknown argument " + a);
    if (!has) {
      if (i + 1 >= argc) throw CliError("option " + a + " needs a value");
      val = argv[++i];
    }
    cli.got[opt->name] = val;
  }
  return cli;
}

// (the entry writer -- put_text, put_entries, write_entries -- is host_files.hpp's: `merkle-tree` writes through it too)

// ---- parsing mode --------------------------------------------------------------------------------------------------
struct Signatures {
  std::vector<uint8_t> r, s, z, v, addr;   // 32, 32, 32, 1, 20 bytes per entry
  std::vector<char> addr_text;             // 42 characters per entry, as given
  std::vector<std::string> balance;        // decimal, no leading zeros
  uint64_t n = 0;
};

void read_signatures(const std::string& path, Signatures& g) {
  MappedFile text(path.c_str());
  Json js{text.begin(), text.end()};
  js.array([&](uint64_t i) {
    bool have_sig = false, have_addr = false, have_bal = false;
    g.r.resize(32 * (i + 1));
    g.s.resize(32 * (i + 1));
    g.z.resize(32 * (i + 1));
    g.v.resize(i + 1);
    g.addr.resize(20 * (i + 1));
    g.addr_text.resize(42 * (i + 1));
    js.object([&](const Span& key) {
      if (key.is("signature")) {
        unsigned seen = 0;
        js.object([&](const Span& k2) {
          if (k2.is("r") || k2.is("s")) {
            const Span h = js.string();
            // a 32-byte quantity: ethers takes "0x" + 64 digits; shorter spellings are padded here
            if (!parse_hex_u256(h, (k2.b[0] == 'r' ? g.r.data() : g.s.data()) + 32 * i))
              throw InputError(entry(i) + "signature." + k2.str() + " is not 0x-prefixed hex of at most 32 bytes");
            seen |= k2.b[0] == 'r' ? 1u : 2u;
          } else if (k2.is("msghash")) {
            if (!parse_hex_bytes(js.string(), g.z.data() + 32 * i, 32)) throw InputError(entry(i) + "signature.msghash is not 0x + 64 hex digits");
            seen |= 4u;
          } else if (k2.is("v")) {
            const std::string t = js.number().str();
            long long val;
            if (!parse_integer(t, val)) throw InputError(entry(i) + "signature.v is not an integer: " + t);
            g.v[i] = (uint8_t)(val < 0 || val > 255 ? 255 : val);   // anything but 27 / 28 is status 1
            seen |= 8u;
          } else {
            js.skip();
          }
        });
        if (seen != 15u) throw InputError(entry(i) + "signature needs r, s, v and msghash");
        have_sig = true;
      } else if (key.is("address")) {
        const Span a = js.string();
        if (!parse_hex_bytes(a, g.addr.data() + 20 * i, 20)) throw InputError(entry(i) + "address is not 0x + 40 hex digits: " + a.str());
        memcpy(g.addr_text.data() + 42 * i, a.b, 42);
        have_addr = true;
      } else if (key.is("balance")) {
        Span b = js.string();
        if (b.size() && b.e[-1] == 'n') b.e--;   // a BigInt literal's suffix, as the reference accepts it
        if (!b.size()) throw InputError(entry(i) + "balance is empty");
        for (const char* q = b.b; q < b.e; q++)
          if (*q < '0' || *q > '9') throw InputError(entry(i) + "balance is not a decimal number: " + b.str());
        while (b.size() > 1 && *b.b == '0') b.b++;
        g.balance.push_back(b.str());
        have_bal = true;
      } else {
        js.skip();
      }
    });
    if (!have_sig || !have_addr || !have_bal) throw InputError(entry(i) + "needs signature, address and balance");
    g.n = i + 1;
  });
  js.end();
}

const char* status_text(unsigned st) {
  switch (st) {
    case 2: return "r or s is zero or not below the group order";
    case 3: return "non-canonical s (s >= 2^255)";
    case 4: return "r is not the x coordinate of a curve point";
    case 5: return "the recovered public key is the point at infinity";
    default: return "unknown status";
  }
}

void put_big(std::string& o, const char* indent, const char* key, const U256& x, bool last) {
  o += indent;
  o += "\"";
  o += key;
  o += "\": {\n";
  o += indent;
  o += "  \"__bigint__\": \"";
  x.append_dec(o);
  o += "\"\n";
  o += indent;
  o += last ? "}\n" : "},\n";
}

int parse_mode(const Cli& cli) {
  const std::string &in_path = cli.value("--signatures"), &out_path = cli.value("--output-path");
  if (in_path.empty() || out_path.empty()) throw CliError("--signatures <FILE> and --output-path <FILE> are required", true);
  ContextStart start(device_from_env());   // the device starts up while this thread reads the file
  Signatures g;
  PhaseTimer lap("ecdsa-sigs-parser", 8);
  read_signatures(in_path, g);
  lap("read");
  const uint64_t n = g.n;
  printf("Parsing %llu ECDSA signatures..\n", (unsigned long long)n);
  zkpoa_context* ctx = start.get();   // what is left of the start-up counts as device time
  std::vector<uint8_t> rprime(32 * n + 1), pub(64 * n + 1), derived(20 * n + 1), status(n + 1);
  std::vector<char> text(42 * n + 1);
  if (zkpoa_ecdsa_star(ctx, n, g.r.data(), g.s.data(), g.z.data(), g.v.data(), g.addr.data(), rprime.data(), pub.data(),
                       derived.data(), status.data()) != PROVER_OK)
    throw InputError(std::string("zkpoa_ecdsa_star: ") + zkpoa_last_error(ctx));
  if (zkpoa_eth_address(ctx, pub.data(), n, derived.data(), text.data()) != PROVER_OK)
    throw InputError(std::string("zkpoa_eth_address: ") + zkpoa_last_error(ctx));
  lap("device");
  // the reference compares strings: the address given must be the EIP-55 spelling of the one derived
  for (uint64_t i = 0; i < n; i++) {
    const unsigned st = status[i];
    if (st == 1) throw InputError(entry(i) + "Invalid ECDSA 'v' value " + std::to_string((int)g.v[i]) + " (must be 27 or 28)");
    if (st != 0 && st != 6) throw InputError(entry(i) + status_text(st));
    if (st == 6 || memcmp(&text[42 * i], &g.addr_text[42 * i], 42) != 0)
      throw InputError(entry(i) + "the address given is " + std::string(&g.addr_text[42 * i], 42) + " but the signature's key has address " +
                       std::string(&text[42 * i], 42));
  }
  printf("Successfully parsed ECDSA signatures and converted them to ECDSA* signatures\n");
  write_entries(out_path, n ? "{\n  \"accountAttestations\": [\n" : "{\n  \"accountAttestations\": []\n}", n ? "  ]\n}" : "", n, 1400,
                [&](std::string& o, uint64_t i) {
                  o += "    {\n      \"signature\": {\n";
                  put_big(o, "        ", "r", U256::from_be(&g.r[32 * i]), false);
                  put_big(o, "        ", "s", U256::from_be(&g.s[32 * i]), false);
                  put_big(o, "        ", "r_prime", U256::from_be(&rprime[32 * i]), false);
                  o += "        \"pubkey\": {\n";
                  put_big(o, "          ", "x", U256::from_be(&pub[64 * i]), false);
                  put_big(o, "          ", "y", U256::from_be(&pub[64 * i + 32]), true);
                  o += "        },\n        \"msghash\": {\n          \"__uint8array__\": [\n";
                  for (int k = 0; k < 32; k++) {
                    o += "            ";
                    o += std::to_string((unsigned)g.z[32 * i + k]);
                    o += k < 31 ? ",\n" : "\n";
                  }
                  o += "          ]\n        }\n      },\n      \"accountData\": {\n";
                  uint8_t a32[32] = {0};
                  memcpy(a32 + 12, &derived[20 * i], 20);
                  put_big(o, "        ", "address", U256::from_be(a32), false);
                  o += "        \"balance\": {\n          \"__bigint__\": \"" + g.balance[i] + "\"\n        }\n      }\n    }";
                  o += i + 1 < n ? ",\n" : "\n";
                });
  lap("write");
  return 0;
}

// ---- layer-one-input mode ------------------------------------------------------------------------------------------
struct StarSig {
  U256 r, s, rprime, x, y, msghash;
};

int layer_one_mode(const Cli& cli) {
  BatchRange range = cli.batch_range();
  const std::string &in_path = cli.value("--poa-input-data"), &out_path = cli.value("--write-layer-one-data-to");
  if (in_path.empty() || out_path.empty())
    throw CliError("layer-one-input needs --poa-input-data <FILE> and --write-layer-one-data-to <FILE>", true);
  printf("Preparing input for layer 1 using the following data:\n- System input: %s\n- Start index for batch: %lld\n"
         "- End index for batch: %lld\nPath to write processed data to: %s\n\n",
         in_path.c_str(), range.start, range.end, out_path.c_str());
  std::vector<StarSig> sigs;   // entries first_kept, first_kept + 1, ...: only those the range can reach are converted
  const long long first_kept = range.first_kept();
  const long long total = for_each_attestation(in_path, range, [&](Json& js, uint64_t i) {
    StarSig g;
    unsigned have = 0;
    js.object([&](const Span& k1) {
      if (!k1.is("signature")) return js.skip();
      js.object([&](const Span& k2) {
        if (k2.is("r")) g.r = read_bigint(js, "r"), have |= 1u;
        else if (k2.is("s")) g.s = read_bigint(js, "s"), have |= 2u;
        else if (k2.is("r_prime")) g.rprime = read_bigint(js, "r_prime"), have |= 4u;
        else if (k2.is("pubkey")) {
          js.object([&](const Span& k3) {
            if (k3.is("x")) g.x = read_bigint(js, "pubkey.x"), have |= 8u;
            else if (k3.is("y")) g.y = read_bigint(js, "pubkey.y"), have |= 16u;
            else js.skip();
          });
        } else if (k2.is("msghash")) {
          js.object([&](const Span& k3) {
            if (!k3.is("__uint8array__")) return js.skip();
            uint8_t bytes[32] = {0};
            const uint64_t len = js.array([&](uint64_t k) {
              long long val;
              if (!parse_integer(js.number().str(), val) || val < 0 || val > 255 || k >= 32) throw InputError(entry(i) + "msghash is not 32 bytes");
              bytes[k] = (uint8_t)val;
            });
            if (len != 32) throw InputError(entry(i) + "msghash is not 32 bytes");
            g.msghash = U256::from_be(bytes);
            have |= 32u;
          });
        } else {
          js.skip();
        }
      });
    });
    if (have != 63u) throw InputError(entry(i) + "signature needs r, s, r_prime, pubkey.x, pubkey.y and msghash");
    sigs.push_back(g);
  });
  range.close(total);
  long long lo, hi;
  range.slice(total, lo, hi);
  const uint64_t m = (uint64_t)(hi - lo);
  AtomicFile fo(out_path.c_str());
  uint64_t off = 0;
  const char* names[5] = {"r", "s", "rprime", "pubkey", "msghash"};
  for (int f = 0; f < 5; f++) {
    put_text(fo, off, std::string(f ? "" : "{\n") + "  \"" + names[f] + (m ? "\": [\n" : "\": []"));
    put_entries(fo, off, m, 1024, 0, [&](std::string& o, uint64_t i) {
      const StarSig& g = sigs[(uint64_t)(lo - first_kept) + i];
      const bool last = i + 1 == m;
      if (f == 3) {
        o += "    [\n";
        put_limbs(o, "      ", g.x, false);
        put_limbs(o, "      ", g.y, true);
        o += last ? "    ]\n" : "    ],\n";
      } else {
        put_limbs(o, "    ", f == 0 ? g.r : f == 1 ? g.s : f == 2 ? g.rprime : g.msghash, last);
      }
    });
    put_text(fo, off, std::string(m ? "  ]" : "") + (f < 4 ? ",\n" : "\n}"));
  }
  fo.commit();
  return 0;
}


// ---- sign and anon-set modes -----------------------------------------------------------------------------------------
// The two files the workflow starts from, which the reference makes with tests/generate_ecdsa_signatures.ts (noble's
// sign, at most 128 keys of a list in the script) and tests/generate_anon_set.ts (at most about 10,600 addresses). Keys
// come from a file, are derived from a seed on the GPU, or are the children of a BIP-32 key (further down); signing, public keys, addresses and the filler accounts'
// hashes run there (include/zkpoa_ecdsa_sign.h), sorting and formatting on the host threads. Not hardened against side
// channels, and the keys pass through host memory and a text file: made for rehearsals and test data.
constexpr uint64_t kGroupOrder[4] = {0xbfd25e8cd0364141ull, 0xbaaedce6af48a03bull, 0xfffffffffffffffeull, 0xffffffffffffffffull};

struct Keys {
  std::vector<uint8_t> key;       // 32 bytes per key, big-endian; none under a public HD source
  std::vector<U256> balance;
  std::vector<uint64_t> line;     // of the key file, 1-based; empty for derived keys
  std::vector<uint8_t> addr, pub; // an HD source only: 20 and 64 bytes per account, which its derivation gives already
  std::vector<uint64_t> index;    // an HD source only: the child index of each account
  uint64_t n = 0;
};

U256 default_balance(const U256& key) {   // the reference's generateDeterministicBalance: key mod 1000
  unsigned __int128 rem = 0;
  for (int k = 3; k >= 0; k--) rem = ((rem << 64) | key.v[k]) % 1000u;
  U256 b;
  b.v[0] = (uint64_t)rem;
  return b;
}

// <decimal or 0x-hex key>[,<decimal balance>] per line; blank lines and lines that begin with # are skipped. The first
// bad line ends the command: "key <line number>: ...".
void read_keys(const std::string& path, Keys& g) {
  MappedFile text(path.c_str());
  const char *p = text.begin(), *end = text.end();
  for (uint64_t line = 1; p < end; line++) {
    const char* eol = static_cast<const char*>(memchr(p, '\n', (size_t)(end - p)));
    const char *b = p, *e = eol ? eol : end;
    p = eol ? eol + 1 : end;
    auto blank = [](char c) { return c == ' ' || c == '\t' || c == '\r'; };
    while (b < e && blank(*b)) b++;
    while (e > b && blank(e[-1])) e--;
    if (b == e || *b == '#') continue;
    const std::string where = "key " + std::to_string(line) + ": ";
    const char* comma = static_cast<const char*>(memchr(b, ',', (size_t)(e - b)));
    const char* ke = comma ? comma : e;
    while (ke > b && blank(ke[-1])) ke--;
    U256 key, bal;
    if (!key.parse_number(b, ke)) throw InputError(where + "not a decimal or 0x-hex number below 2^256: " + std::string(b, ke));
    if (!(key.v[0] | key.v[1] | key.v[2] | key.v[3])) throw InputError(where + "the key is zero");
    if (!key.below(kGroupOrder)) throw InputError(where + "the key is not below the group order");
    if (comma) {
      const char* bb = comma + 1;
      while (bb < e && blank(*bb)) bb++;
      if (!bal.parse_dec(bb, e)) throw InputError(where + "the balance is not a decimal number below 2^256: " + std::string(bb, e));
    } else {
      bal = default_balance(key);
    }
    g.key.resize(32 * (g.n + 1));
    key.to_be(&g.key[32 * g.n]);
    g.balance.push_back(bal);
    g.line.push_back(line);
    g.n++;
  }
}

void derive_keys(zkpoa_context* ctx, const std::string& seed, uint64_t count, Keys& g) {
  g.key.resize(32 * count + 1);
  if (zkpoa_secp256k1_derive_keys(ctx, seed.data(), seed.size(), 0, count, g.key.data()) != PROVER_OK)
    throw InputError(std::string("zkpoa_secp256k1_derive_keys: ") + zkpoa_last_error(ctx));
  g.balance.resize(count);
  parallel_ranges(count, 4096, [&](unsigned, uint64_t lo, uint64_t hi) {
    for (uint64_t i = lo; i < hi; i++) g.balance[i] = default_balance(U256::from_be(&g.key[32 * i]));
  });
  g.n = count;
}

void put_hex(std::string& o, const uint8_t* b, size_t bytes) {
  static const char digits[] = "0123456789abcdef";
  for (size_t i = 0; i < bytes; i++) {
    o.push_back(digits[b[i] >> 4]);
    o.push_back(digits[b[i] & 15]);
  }
}

// indices 0 .. n-1 by the 20 address bytes, ascending; equal addresses keep their order (Array.prototype.sort is stable)
// The first eight bytes travel with the index, so that nearly every comparison stays inside the array being sorted; the
// host threads sort a piece each, then merge the pieces pairwise.
std::vector<uint32_t> order_by_address(const uint8_t* addr20, uint64_t n) {
  struct Item {
    uint64_t head;
    uint32_t idx;
  };
  std::vector<Item> items(n);
  parallel_ranges(n, 4096, [&](unsigned, uint64_t lo, uint64_t hi) {
    for (uint64_t i = lo; i < hi; i++) {
      uint64_t head = 0;
      for (int k = 0; k < 8; k++) head = (head << 8) | addr20[20 * i + k];
      items[i] = {head, (uint32_t)i};
    }
  });
  auto less = [&](const Item& a, const Item& b) {
    if (a.head != b.head) return a.head < b.head;
    const int c = memcmp(addr20 + 20ull * a.idx + 8, addr20 + 20ull * b.idx + 8, 12);
    return c ? c < 0 : a.idx < b.idx;
  };
  unsigned pieces = 1;
  while (pieces * 2 <= host_threads() && n / (pieces * 2) >= 1024) pieces *= 2;
  auto cut = [&](unsigned p) { return items.begin() + (ptrdiff_t)(n * p / pieces); };
  run_threads(pieces, [&](unsigned t) { std::sort(cut(t), cut(t + 1), less); });
  for (unsigned width = 1; width < pieces; width *= 2)
    run_threads(pieces / (2 * width), [&](unsigned t) { std::inplace_merge(cut(2 * width * t), cut(2 * width * t + width), cut(2 * width * (t + 1)), less); });
  std::vector<uint32_t> idx(n);
  parallel_ranges(n, 4096, [&](unsigned, uint64_t lo, uint64_t hi) {
    for (uint64_t i = lo; i < hi; i++) idx[i] = items[i].idx;
  });
  return idx;
}

// ---- HD key sources: a BIP-32 wallet (include/zkpoa_hd_wallet.h) -------------------------------------------------------
// --hd-key <xprv | xpub>, --mnemonic <words> [--passphrase <text>] or --hd-seed 0x<hex> name a key; --hd-path leads from it
// to the account key, whose children --hd-first .. --hd-first + --hd-count - 1 are the accounts. Everything up to the
// account key's path is read and checked on the host, before the device is touched.
constexpr const char* kHdOptions[] = {"--hd-key", "--mnemonic", "--passphrase", "--hd-seed", "--hd-path", "--hd-first", "--hd-count"};

struct HdSource {
  bool given = false;
  uint8_t key[33] = {0}, chain[32] = {0};   // the key the path starts from
  std::string path;
  uint64_t first = 0, count = 0;
  bool is_public() const { return key[0] != 0; }
};

// an option's text, or with a leading @ the contents of that file without the blanks and line ends around it: a secret
// need not stand in the process list
std::string text_or_file(const std::string& v) {
  if (v.empty() || v[0] != '@') return v;
  MappedFile f(v.c_str() + 1);
  const char *b = f.begin(), *e = f.end();
  auto blank = [](char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; };
  while (b < e && blank(*b)) b++;
  while (e > b && blank(e[-1])) e--;
  return std::string(b, e);
}

HdSource hd_source(const Cli& cli) {
  HdSource hd;
  const int named = (int)cli.has("--hd-key") + (int)cli.has("--mnemonic") + (int)cli.has("--hd-seed");
  if (named == 0) {
    for (const char* o : kHdOptions)
      if (cli.has(o)) throw CliError(std::string(o) + " goes with --hd-key, --mnemonic or --hd-seed");
    return hd;
  }
  if (named > 1) throw CliError("--hd-key, --mnemonic and --hd-seed exclude each other");
  if (cli.has("--passphrase") && !cli.has("--mnemonic")) throw CliError("--passphrase goes with --mnemonic");
  hd.given = true;
  if (cli.has("--hd-key")) {
    uint32_t where[2];
    if (zkpoa_bip32_parse_key(text_or_file(cli.value("--hd-key")).c_str(), hd.key, hd.chain, where) != PROVER_OK)
      throw CliError("--hd-key is not an xprv / xpub (base58 alphabet, length, checksum, version or key)");
  } else {
    uint8_t seed[64];
    size_t seed_len = 64;
    if (cli.has("--mnemonic")) {
      if (zkpoa_bip39_seed(text_or_file(cli.value("--mnemonic")).c_str(), text_or_file(cli.value("--passphrase")).c_str(), seed) != PROVER_OK)
        throw CliError("--mnemonic and --passphrase are ASCII text of at most 4096 bytes (NFKD normalisation is not implemented)");
    } else {
      const std::string hex = text_or_file(cli.value("--hd-seed"));
      seed_len = hex.size() >= 2 ? (hex.size() - 2) / 2 : 0;
      if (seed_len < 16 || seed_len > 64 || !parse_hex_bytes(Span{hex.data(), hex.data() + hex.size()}, seed, seed_len))
        throw CliError("--hd-seed is 0x and 16 to 64 bytes of hex digits");
    }
    if (zkpoa_bip32_master(seed, seed_len, hd.key, hd.chain) != PROVER_OK) throw CliError("the seed has no master key (IL is zero or not below the group order)");
  }
  hd.path = cli.has("--hd-path") ? cli.value("--hd-path") : (cli.has("--hd-key") ? "m" : "m/44'/60'/0'/0");
  uint32_t levels[255], n_levels = 0;
  if (zkpoa_bip32_parse_path(hd.path.c_str(), levels, &n_levels) != PROVER_OK)
    throw CliError("--hd-path is not a path (m, m/0, m/44'/60'/0'/0; at most 255 levels): " + hd.path);
  for (uint32_t i = 0; i < n_levels; i++)
    if (hd.is_public() && (levels[i] >> 31)) throw CliError("--hd-path has a hardened level, which an xpub cannot derive: " + hd.path);
  cli.required("--hd-count");
  hd.count = cli.count("--hd-count", 0, "children up to 2^32");
  if (cli.has("--hd-first")) hd.first = cli.count("--hd-first", 0, "children to skip, up to 2^32");
  if (hd.first + hd.count > (1ull << 32)) throw CliError("--hd-first + --hd-count is at most 2^32");
  if (hd.is_public() && hd.first + hd.count > (1ull << 31)) throw CliError("an xpub has no hardened children: --hd-first + --hd-count is at most 2^31");
  return hd;
}

// The accounts of an HD source: the children first .. first + count - 1 of the key at the path, on the GPU. The balance
// of an account is its address mod 1000, so that the xprv and its xpub tell the same. A child that BIP-32 calls invalid
// is skipped, with a line on stderr.
void derive_hd(zkpoa_context* ctx, const HdSource& hd, uint64_t count, Keys& g) {
  uint8_t key[33], chain[32];
  if (zkpoa_bip32_derive_path(ctx, hd.key, hd.chain, hd.path.c_str(), key, chain) != PROVER_OK)
    throw InputError(std::string("zkpoa_bip32_derive_path: ") + zkpoa_last_error(ctx));
  std::vector<uint8_t> key33(33 * count + 1), chains(32 * count + 1), status(count + 1);
  g.addr.resize(20 * count + 1);
  g.pub.resize(64 * count + 1);
  if (zkpoa_bip32_children(ctx, key, chain, hd.first, count, key33.data(), chains.data(), g.pub.data(), g.addr.data(), status.data()) != PROVER_OK)
    throw InputError(std::string("zkpoa_bip32_children: ") + zkpoa_last_error(ctx));
  if (!hd.is_public()) g.key.resize(32 * count + 1);
  g.balance.resize(count);
  g.index.resize(count);
  for (uint64_t i = 0; i < count; i++) {
    if (status[i]) {
      fprintf(stderr, "ecdsa-sigs-parser: child %llu is invalid (BIP-32) and is skipped\n", (unsigned long long)(hd.first + i));
      continue;
    }
    if (!hd.is_public()) memcpy(&g.key[32 * g.n], &key33[33 * i + 1], 32);
    memmove(&g.addr[20 * g.n], &g.addr[20 * i], 20);
    memmove(&g.pub[64 * g.n], &g.pub[64 * i], 64);
    uint8_t a32[32] = {0};
    memcpy(a32 + 12, &g.addr[20 * g.n], 20);
    g.balance[g.n] = default_balance(U256::from_be(a32));
    g.index[g.n] = hd.first + i;
    g.n++;
  }
}

// the key source of the modes: exactly one of --keys <file>, --generate-keys <N> --seed <text> and an HD source
struct KeySource {
  std::string file, seed;
  uint64_t count = 0;
  bool generate = false;
  HdSource hd;
};

KeySource key_source(const Cli& cli) {
  KeySource src;
  src.hd = hd_source(cli);
  const bool file = cli.has("--keys");
  if ((int)file + (int)cli.has("--generate-keys") + (int)src.hd.given != 1)
    throw CliError(std::string(cli.mode) + " needs exactly one of --keys <file>, --generate-keys <N> --seed <text> and an HD source (--hd-key, --mnemonic, --hd-seed)");
  if (src.hd.given) {
    if (cli.has("--seed")) throw CliError("--seed goes with --generate-keys");
    return src;
  }
  if (file) {
    if (cli.has("--seed")) throw CliError("--seed goes with --generate-keys");
    src.file = cli.value("--keys");
    return src;
  }
  if (!cli.has("--seed")) throw CliError("--generate-keys needs --seed <text>");
  src.count = cli.count("--generate-keys", 0, "keys up to 2^32");
  src.seed = cli.value("--seed");
  if (src.seed.size() > 4084) throw CliError("--seed is at most 4084 bytes");
  src.generate = true;
  return src;
}

// with_balance: "0x<key>,<balance>" lines, for keys whose balance is not the default of a key file (an HD source's)
void write_key_file(const std::string& path, const Keys& g, bool with_balance) {
  write_entries(path, "", "", g.n, 72, [&](std::string& o, uint64_t i) {
    o += "0x";
    put_hex(o, &g.key[32 * i], 32);
    if (with_balance) {
      o += ",";
      g.balance[i].append_dec(o);
    }
    o += "\n";
  });
}

int sign_mode(const Cli& cli) {
  const KeySource src = key_source(cli);
  if (src.hd.given && src.hd.is_public()) throw CliError("sign needs private keys, and --hd-key is an xpub");
  if (cli.has("--message") == cli.has("--msghash")) throw CliError("sign needs either --message <text> or --msghash 0x<64 hex digits>");
  const std::string& out_path = cli.required("--output-path");
  uint8_t z[32];
  if (cli.has("--message")) {
    const std::string& msg = cli.value("--message");
    zkpoa_sha256(msg.data(), msg.size(), z);
  } else {
    const std::string& h = cli.value("--msghash");
    if (!parse_hex_bytes(Span{h.data(), h.data() + h.size()}, z, 32)) throw CliError("--msghash is not 0x + 64 hex digits");
  }
  ContextStart start(device_from_env());
  PhaseTimer lap("ecdsa-sigs-parser sign", 8);
  Keys g;
  if (!src.generate && !src.hd.given) read_keys(src.file, g);
  zkpoa_context* ctx = start.get();
  if (src.generate) derive_keys(ctx, src.seed, src.count, g);
  if (src.hd.given) derive_hd(ctx, src.hd, src.hd.count, g);
  lap("keys");
  const uint64_t n = g.n;
  printf("Signing with %llu keys..\n", (unsigned long long)n);
  std::vector<uint8_t> r(32 * n + 1), s(32 * n + 1), v(n + 1), pub(64 * n + 1), addr(20 * n + 1), status(n + 1);
  std::vector<char> text(42 * n + 1);
  if (zkpoa_ecdsa_sign(ctx, n, g.key.data(), z, 0, r.data(), s.data(), v.data(), pub.data(), addr.data(), status.data()) != PROVER_OK)
    throw InputError(std::string("zkpoa_ecdsa_sign: ") + zkpoa_last_error(ctx));
  for (uint64_t i = 0; i < n; i++)
    if (status[i])
      throw InputError("key " + std::to_string(g.line.empty() ? i + 1 : g.line[i]) +
                       (status[i] == 2 ? ": the nonce point's x coordinate is not below the group order (v cannot express it)"
                                       : ": the key is zero or not below the group order"));
  if (zkpoa_eth_address(ctx, pub.data(), n, addr.data(), text.data()) != PROVER_OK)
    throw InputError(std::string("zkpoa_eth_address: ") + zkpoa_last_error(ctx));
  lap("device");
  const std::vector<uint32_t> order = order_by_address(addr.data(), n);
  lap("sort");
  std::string zhex;
  put_hex(zhex, z, 32);
  write_entries(out_path, "[", "]", n, 420, [&](std::string& o, uint64_t k) {
    const uint64_t i = order[k];
    if (k) o += ",";
    o += "{\"signature\":{\"r\":\"0x";
    put_hex(o, &r[32 * i], 32);
    o += "\",\"s\":\"0x";
    put_hex(o, &s[32 * i], 32);
    o += "\",\"v\":" + std::to_string((unsigned)v[i]) + ",\"msghash\":\"0x" + zhex + "\"},\"address\":\"";
    o.append(&text[42 * i], 42);
    o += "\",\"balance\":\"";
    g.balance[i].append_dec(o);
    o += "n\"}";
  });
  if (cli.has("--write-keys")) write_key_file(cli.value("--write-keys"), g, src.hd.given);
  lap("write");
  printf("Wrote %llu signatures to %s\n", (unsigned long long)n, out_path.c_str());
  return 0;
}

int anon_set_mode(const Cli& cli) {
  const KeySource src = key_source(cli);
  cli.required("--num-addresses");
  const uint64_t total = cli.count("--num-addresses", 1, "addresses from 1 to 2^32");
  const std::string& out_path = cli.required("--output-path");
  ContextStart start(device_from_env());
  PhaseTimer lap("ecdsa-sigs-parser anon-set", 8);
  Keys g;
  if (!src.generate && !src.hd.given) read_keys(src.file, g);
  zkpoa_context* ctx = start.get();
  if (src.generate) derive_keys(ctx, src.seed, std::min(src.count, total), g);
  if (src.hd.given) derive_hd(ctx, src.hd, std::min(src.hd.count, total), g);
  const uint64_t owned = std::min(g.n, total);
  std::vector<uint8_t> addr(20 * total + 1);
  std::vector<U256> balance(total);
  if (src.hd.given) {   // the derivation gave the addresses already, and an xpub has no keys to give
    memcpy(addr.data(), g.addr.data(), 20 * owned);
    std::copy(g.balance.begin(), g.balance.begin() + (ptrdiff_t)owned, balance.begin());
  } else {
    std::vector<uint8_t> pub(64 * owned + 1), status(owned + 1);
    if (zkpoa_secp256k1_pubkey(ctx, owned, g.key.data(), pub.data(), addr.data(), status.data()) != PROVER_OK)
      throw InputError(std::string("zkpoa_secp256k1_pubkey: ") + zkpoa_last_error(ctx));
    for (uint64_t i = 0; i < owned; i++) {
      if (status[i]) throw InputError("key " + std::to_string(g.line.empty() ? i + 1 : g.line[i]) + ": the key is zero or not below the group order");
      balance[i] = g.balance[i];
    }
  }
  // the filler accounts: D_j = Keccak-256(seed || "anon" || be64(j)), address = its last 20 bytes, balance = its first 8
  // bytes (big-endian) mod 10^6; a million at a time
  const size_t len = src.seed.size() + 12;
  constexpr uint64_t kSlab = 1u << 20;
  std::vector<uint8_t> msgs, digests;
  for (uint64_t j0 = 0; owned + j0 < total; j0 += kSlab) {
    const uint64_t m = std::min(kSlab, total - owned - j0);
    msgs.resize(len * m);
    digests.resize(32 * m);
    parallel_ranges(m, 4096, [&](unsigned, uint64_t lo, uint64_t hi) {
      for (uint64_t j = lo; j < hi; j++) {
        uint8_t* q = &msgs[len * j];
        memcpy(q, src.seed.data(), src.seed.size());
        memcpy(q + src.seed.size(), "anon", 4);
        for (int k = 0; k < 8; k++) q[src.seed.size() + 4 + k] = (uint8_t)((j0 + j) >> (8 * (7 - k)));
      }
    });
    if (zkpoa_keccak256(ctx, msgs.data(), len, m, digests.data()) != PROVER_OK)
      throw InputError(std::string("zkpoa_keccak256: ") + zkpoa_last_error(ctx));
    parallel_ranges(m, 4096, [&](unsigned, uint64_t lo, uint64_t hi) {
      for (uint64_t j = lo; j < hi; j++) {
        const uint8_t* d = &digests[32 * j];
        memcpy(&addr[20 * (owned + j0 + j)], d + 12, 20);
        uint64_t head = 0;
        for (int k = 0; k < 8; k++) head = (head << 8) | d[k];
        balance[owned + j0 + j].v[0] = head % 1000000u;
      }
    });
  }
  lap("device");
  const std::vector<uint32_t> order = order_by_address(addr.data(), total);
  lap("sort");
  write_entries(out_path, "address,eth_balance\n", "", total, 100, [&](std::string& o, uint64_t k) {
    const uint64_t i = order[k];
    o += "0x000000000000000000000000";
    put_hex(o, &addr[20 * i], 20);
    o += ",";
    balance[i].append_dec(o);
    o += "\n";
  });
  lap("write");
  printf("Wrote an anonymity set of %llu addresses (%llu of them from keys) to %s\n", (unsigned long long)total, (unsigned long long)owned,
         out_path.c_str());
  return 0;
}

// the watch-only listing: the addresses of an HD source's children, in the order of their indices
int hd_list_mode(const Cli& cli) {
  const HdSource hd = hd_source(cli);
  if (!hd.given) throw CliError("hd-list needs an HD source: --hd-key <xprv | xpub>, --mnemonic <words> or --hd-seed 0x<hex>");
  const std::string& out_path = cli.required("--output-path");
  ContextStart start(device_from_env());
  PhaseTimer lap("ecdsa-sigs-parser hd-list", 8);
  Keys g;
  derive_hd(start.get(), hd, hd.count, g);
  std::vector<char> text(42 * g.n + 1);
  if (zkpoa_eth_address(start.get(), g.pub.data(), g.n, g.addr.data(), text.data()) != PROVER_OK)
    throw InputError(std::string("zkpoa_eth_address: ") + zkpoa_last_error(start.get()));
  lap("device");
  write_entries(out_path, "index,address\n", "", g.n, 56, [&](std::string& o, uint64_t i) {
    o += std::to_string(g.index[i]) + ",";
    o.append(&text[42 * i], 42);
    o += "\n";
  });
  lap("write");
  printf("Wrote %llu addresses to %s\n", (unsigned long long)g.n, out_path.c_str());
  return 0;
}

const char kUsage[] =
    "Usage: ecdsa-sigs-parser --signatures <in.json> --output-path <out.json>\n"
    "       ecdsa-sigs-parser sign (--keys <file> | --generate-keys <N> --seed <text> | <HD source: hd-list --help>)\n"
    "                         (--message <text> | --msghash 0x<64 hex>) --output-path <signatures.json> [--write-keys <file>]\n"
    "       ecdsa-sigs-parser anon-set (--keys <file> | --generate-keys <N> --seed <text> | <HD source: hd-list --help>)\n"
    "                         --num-addresses <M> --output-path <anonymity_set.csv>\n"
    "       ecdsa-sigs-parser layer-one-input --poa-input-data <parsed.json> --write-layer-one-data-to <out.json>\n"
    "                         [--account-start-index <i>] [--account-end-index <j>]\n"
    "       ecdsa-sigs-parser layer-two-input --poa-input-data <parsed.json> --merkle-root <merkle_root.json>\n"
    "                         --merkle-proofs <merkle_proofs.json> --layer-one-sanitized-proof <sanitized_proof.json>\n"
    "                         --write-x-coords-hash-to <hash.txt> --write-layer-two-data-to <out.json>\n"
    "                         [--account-start-index <i>] [--account-end-index <j>]\n"
    "       ecdsa-sigs-parser layer-three-input --merkle-root-path <merkle_root.json>\n"
    "                         --layer-two-sanitized-proof-paths <a.json,b.json,...> --write-layer-three-data-to <out.json>\n"
    "                         --blindingFactor <decimal or 0x-hex>\n"
    "       ecdsa-sigs-parser pedersen-check --poa-input-data <parsed.json> --layer-three-public-inputs <public.json>\n"
    "                         --blindingFactor <decimal or 0x-hex>\n";

// hd-list's own usage, which also spells the HD source that sign and anon-set take (kUsage keeps its sixteen lines)
const char kHdUsage[] =
    "Usage: ecdsa-sigs-parser hd-list <HD source> --output-path <addresses.csv>      (index,address per child)\n"
    "       <HD source>, also a key source of sign (private only) and anon-set: the children i = first .. first + N - 1 of a\n"
    "       BIP-32 key, as accounts with balance = address mod 1000\n"
    "         --hd-key <xprv...|xpub...|@file> | --mnemonic <words|@file> [--passphrase <text|@file>] | --hd-seed 0x<hex>\n"
    "         [--hd-path <path>]   from that key to the children's parent; default m/44'/60'/0'/0 (m for --hd-key)\n"
    "         [--hd-first <i>] --hd-count <N>\n"
    "       @file: the value is the file's text. The mnemonic's words and checksum are not checked; ASCII only.\n";

// the three modes of layer_inputs.hpp
int layer_two_cli(const Cli& cli) {
  const BatchRange range = cli.batch_range();
  LayerTwoPaths p;
  p.input = cli.required("--poa-input-data");
  p.merkle_root = cli.required("--merkle-root");
  p.merkle_proofs = cli.required("--merkle-proofs");
  p.hash_out = cli.required("--write-x-coords-hash-to");
  p.layer_one_proof = cli.required("--layer-one-sanitized-proof");
  p.out = cli.required("--write-layer-two-data-to");
  return layer_two_mode(p, range);
}
int layer_three_cli(const Cli& cli) {
  return layer_three_mode(cli.required("--merkle-root-path"), cli.required("--layer-two-sanitized-proof-paths"),
                          cli.required("--write-layer-three-data-to"), cli.required("--blindingFactor"));
}
int pedersen_check_cli(const Cli& cli) {
  return pedersen_check_mode(cli.required("--poa-input-data"), cli.required("--layer-three-public-inputs"), cli.required("--blindingFactor"));
}

// How a mode answers a CliError: with "error: ..." and the usage text (exit status 2), with "Error: ..." as for any
// other failure (1), or with "error: ..." alone (2).
enum Answer { kWithUsage, kAsFailure, kBrief };
struct Mode {
  const char* name;               // argv[1]; the parser itself has none, and its options begin there
  std::vector<Option> options;    // the reference's names
  Answer misspelt, absent;        // the answer to a command line that cannot be read, and to one that lacks a required option
  bool help;                      // -h / --help print the usage (in layer-two-input -h is the hash path, as in the reference)
  int (*run)(const Cli&);
  const char* usage = kUsage;     // what its help and its kWithUsage answers print
};
std::vector<Option> with_hd(std::vector<Option> own) {   // a mode's own options and those of an HD source
  for (const char* o : kHdOptions) own.push_back({o, nullptr});
  return own;
}
const Mode kModes[] = {
    {"sign", with_hd({{"--keys", nullptr}, {"--generate-keys", nullptr}, {"--seed", nullptr}, {"--message", nullptr}, {"--msghash", nullptr},
                      {"--output-path", "-o"}, {"--write-keys", nullptr}}),
     kWithUsage, kWithUsage, false, sign_mode},
    {"anon-set", with_hd({{"--keys", nullptr}, {"--generate-keys", nullptr}, {"--seed", nullptr}, {"--num-addresses", "-n"},
                          {"--output-path", "-o"}}),
     kWithUsage, kWithUsage, false, anon_set_mode},
    {"hd-list", with_hd({{"--output-path", "-o"}}), kWithUsage, kWithUsage, true, hd_list_mode, kHdUsage},
    {"layer-one-input", {{"--poa-input-data", "-i"}, {"--write-layer-one-data-to", "-o"}, {"--account-start-index", "-s"},
                         {"--account-end-index", "-e"}},
     kAsFailure, kBrief, true, layer_one_mode},
    {"layer-two-input", {{"--poa-input-data", "-i"}, {"--merkle-root", "-t"}, {"--merkle-proofs", "-p"}, {"--write-x-coords-hash-to", "-h"},
                         {"--layer-one-sanitized-proof", "-d"}, {"--write-layer-two-data-to", "-o"}, {"--account-start-index", "-s"},
                         {"--account-end-index", "-e"}},
     kWithUsage, kAsFailure, false, layer_two_cli},
    {"layer-three-input", {{"--merkle-root-path", "-m"}, {"--layer-two-sanitized-proof-paths", "-p"}, {"--write-layer-three-data-to", "-o"},
                           {"--blindingFactor", nullptr}},
     kWithUsage, kAsFailure, false, layer_three_cli},
    {"pedersen-check", {{"--poa-input-data", "-i"}, {"--layer-three-public-inputs", "-p"}, {"--blindingFactor", nullptr}},
     kWithUsage, kAsFailure, false, pedersen_check_cli},
    {"", {{"--signatures", "-s"}, {"--output-path", "-o"}}, kAsFailure, kBrief, true, parse_mode},   // the last: any other first word
};

}  // namespace

int main(int argc, char** argv) {
  const Mode* mode = kModes;
  while (*mode->name && !(argc > 1 && !strcmp(argv[1], mode->name))) mode++;
  int rc = 0;
  try {
    const Cli cli = parse_options(argc, argv, *mode->name ? 2 : 1, mode->name, mode->options, mode->help);
    if (cli.has("--help")) printf("%s", mode->usage);
    else rc = mode->run(cli);
  } catch (const CliError& e) {
    const Answer how = e.absent ? mode->absent : mode->misspelt;
    if (how == kAsFailure) fprintf(stderr, "Error: %s\n", e.what());
    else fprintf(stderr, "error: %s\n%s", e.what(), how == kWithUsage ? mode->usage : "");
    rc = how == kAsFailure ? 1 : 2;
  } catch (const std::exception& e) {
    fprintf(stderr, "Error: %s\n", e.what());
    rc = 1;
  }
  // the output is complete and renamed into place (or the error is on stderr): leave without the HIP runtime's
  // teardown, as merkle-tree does
  fflush(stdout);
  fflush(stderr);
  _exit(rc);
}
