// The anonymity-set csv as `merkle-tree` and `zkpoa-audit` read it: heading line "address,eth_balance", then a 0x-prefixed
// hex address and a decimal balance per line (merkle_tree.rs:212-246), into two arrays of 4 x u64 limbs per row. Host only.
#pragma once
#include "host_files.hpp"
#include "host_text.hpp"

#include <memory>

namespace zkpoa {

static const uint64_t kR[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};

// a field element from its digits: decimal, or the hex digits of a csv address after its prefix
inline U256 parse_num(const char* b, const char* e, bool hex, const char* what) {
  U256 x;
  if (b == e) throw std::runtime_error(std::string("empty ") + what);
  if (!(hex ? x.parse_hex(b, e) : x.parse_dec(b, e))) {   // a character that is no digit, or digits of 2^256 and above
    bool digits = true;
    for (const char* q = b; q < e; q++) digits = digits && (hex ? hex_digit(*q) >= 0 : *q >= '0' && *q <= '9');
    throw std::runtime_error(digits ? std::string(what) + " does not fit 256 bits: " + std::string(b, e)
                                    : std::string("malformed ") + what + ": " + std::string(b, e));
  }
  // light-poseidon's hash_bytes_be refuses inputs that are not field elements (the Rust binary would panic)
  if (!x.below(kR)) throw std::runtime_error(std::string(what) + " is not below the BN254 scalar modulus: " + std::string(b, e));
  return x;
}

// ---- the anonymity set: a 10 M-line csv is ~650 MB of text, and a line-at-a-time reader would take longer over it than
// the GPU takes over the whole tree (0.12 s). The file is mapped, cut at line starts into one piece per thread, and every
// piece is parsed twice: lines counted first (so that each piece knows where its rows go), then converted in place.
// Same rules as before: blank lines are skipped, the first non-blank line is the heading, fields are trimmed of blanks
// and double quotes, an address is 0x-prefixed hex, a balance decimal, both below the scalar modulus.
inline bool is_trim(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n' || c == '"'; }
inline void trim_span(const char*& b, const char*& e) {
  while (b < e && is_trim(*b)) b++;
  while (e > b && is_trim(e[-1])) e--;
}
// calls f(line_begin, line_end) for every non-blank line of [b, e) (e at a line start or the end of the file)
template <class Fn>
inline void for_lines(const char* b, const char* e, Fn f) {
  while (b < e) {
    const char* nl = static_cast<const char*>(memchr(b, '\n', (size_t)(e - b)));
    const char* le = nl ? nl : e;
    const char *tb = b, *te = le;
    trim_span(tb, te);
    if (tb < te) f(b, le);
    b = nl ? nl + 1 : e;
  }
}
inline void parse_row(const char* b, const char* e, uint64_t* addr, uint64_t* bal) {
  const char* comma = static_cast<const char*>(memchr(b, ',', (size_t)(e - b)));
  if (!comma) throw std::runtime_error("Failed to find balance in line in csv file: " + std::string(b, e));
  const char *ab = b, *ae = comma, *bb = comma + 1, *be = e;
  trim_span(ab, ae);
  trim_span(bb, be);
  if (ae - ab < 3 || ab[0] != '0' || (ab[1] != 'x' && ab[1] != 'X'))
    throw std::runtime_error("address is not 0x-prefixed hex: " + std::string(ab, ae));
  const U256 av = parse_num(ab + 2, ae, true, "address"), bv = parse_num(bb, be, false, "balance");
  memcpy(addr, av.v, 32);
  memcpy(bal, bv.v, 32);
}
// rows x 4 limbs, NOT zero-filled: at 10 M rows the 640 MB would be touched once by one thread just to be overwritten --
// the parsing threads are the first to touch their own part
struct Limbs {
  std::unique_ptr<uint64_t[]> p;
  uint64_t rows = 0;
  void alloc(uint64_t n) {
    p.reset(new uint64_t[4 * (n ? n : 1)]);
    rows = n;
  }
  uint64_t* data() { return p.get(); }
};
inline void read_anonymity_set(const std::string& path, Limbs& addr, Limbs& bal) {
  const MappedFile map(path.c_str());
  if (!map.size) return;
  const char *base = map.begin(), *end = map.end();
  // the heading: the first non-blank line
  const char* body = end;
  {
    const char* b = base;
    while (b < end) {
      const char* nl = static_cast<const char*>(memchr(b, '\n', (size_t)(end - b)));
      const char* le = nl ? nl : end;
      const char *tb = b, *te = le;
      trim_span(tb, te);
      b = nl ? nl + 1 : end;
      if (tb < te) {
        body = b;
        break;
      }
    }
  }
  unsigned T = std::thread::hardware_concurrency();
  if (T > 16) T = 16;
  const long forced = opt_long(O_MERKLE_THREADS);
  if (forced) T = (unsigned)forced;
  if (T < 1) T = 1;
  if ((size_t)(end - body) < (1u << 16) && !forced) T = 1;
  std::vector<const char*> cut(T + 1, end);
  cut[0] = body;
  for (unsigned t = 1; t < T; t++) {   // piece boundaries moved forward to the next line start
    const char* p = body + (size_t)(end - body) / T * t;
    if (p < cut[t - 1]) p = cut[t - 1];
    const char* nl = p < end ? static_cast<const char*>(memchr(p, '\n', (size_t)(end - p))) : nullptr;
    cut[t] = nl ? nl + 1 : end;
  }
  std::vector<uint64_t> rows(T, 0);
  run_threads(T, [&](unsigned t) { for_lines(cut[t], cut[t + 1], [&](const char*, const char*) { rows[t]++; }); });
  std::vector<uint64_t> first(T + 1, 0);
  for (unsigned t = 0; t < T; t++) first[t + 1] = first[t] + rows[t];
  addr.alloc(first[T]);
  bal.alloc(first[T]);
  run_threads(T, [&](unsigned t) {
    uint64_t r = first[t];
    for_lines(cut[t], cut[t + 1], [&](const char* b, const char* e) {
      parse_row(b, e, addr.data() + 4 * r, bal.data() + 4 * r);
      r++;
    });
  });
}

}  // namespace zkpoa
