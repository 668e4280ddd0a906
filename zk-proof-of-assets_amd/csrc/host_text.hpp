// The text side of the host programs, in one place: 256-bit integers to and from decimal and hex (U256: the only host
// type that does this), and a JSON pull parser over text that is already in memory (Json: the parsed-signatures file is
// 1.6 GB at 2^20 entries and is never held as a tree). Host only, no HIP; g++ -std=c++17 compiles it alone
// (tools/host_text_check.cpp does). The range checks against r or q, and their messages, belong to the callers.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <stdexcept>
#include <string>

namespace zkpoa {

struct Span {
  const char *b, *e;
  size_t size() const { return (size_t)(e - b); }
  bool is(const char* s) const { return size() == strlen(s) && memcmp(b, s, size()) == 0; }
  std::string str() const { return std::string(b, e); }
};

inline int hex_digit(char c) {
  if (c >= '0' && c <= '9') return c - '0';
  if ((c | 32) >= 'a' && (c | 32) <= 'f') return (c | 32) - 'a' + 10;
  return -1;
}

struct U256 {
  uint64_t v[4] = {0, 0, 0, 0};   // least significant first
  // 32 bytes; limb by limb, so that a compiler turns each inner loop into one load or store
  static U256 from_le(const uint8_t* b) {
    U256 x;
    for (int k = 0; k < 4; k++)
      for (int j = 0; j < 8; j++) x.v[k] |= (uint64_t)b[8 * k + j] << (8 * j);
    return x;
  }
  static U256 from_be(const uint8_t* b) {
    U256 x;
    for (int k = 0; k < 4; k++)
      for (int j = 0; j < 8; j++) x.v[3 - k] |= (uint64_t)b[8 * k + j] << (8 * (7 - j));
    return x;
  }
  void to_le(uint8_t* out) const {
    for (int k = 0; k < 4; k++)
      for (int j = 0; j < 8; j++) out[8 * k + j] = (uint8_t)(v[k] >> (8 * j));
  }
  void to_be(uint8_t* out) const {
    for (int k = 0; k < 4; k++)
      for (int j = 0; j < 8; j++) out[8 * k + j] = (uint8_t)(v[3 - k] >> (8 * (7 - j)));
  }
  bool below(const uint64_t m[4]) const {
    for (int i = 3; i >= 0; i--)
      if (v[i] != m[i]) return v[i] < m[i];
    return false;
  }
  bool mul_add(uint64_t mul, uint64_t add) {   // *this = *this * mul + add; false on overflow
    unsigned __int128 carry = add;
    for (int i = 0; i < 4; i++) {
      const unsigned __int128 cur = (unsigned __int128)v[i] * mul + carry;
      v[i] = (uint64_t)cur;
      carry = cur >> 64;
    }
    return carry == 0;
  }
  // The three parsers: false (and a value that means nothing) when there is no digit, on a character that is no digit of
  // the base, and for 2^256 and above. Any number of leading zeros.
  bool parse_dec(const char* b, const char* e) {   // digits only; 19 of them per step
    *this = U256();
    if (b == e) return false;
    while (e - b > 1 && *b == '0') b++;
    if (e - b > 78) return false;
    while (b < e) {
      uint64_t chunk = 0, scale = 1;
      for (int k = 0; k < 19 && b < e; k++, b++) {
        if (*b < '0' || *b > '9') return false;
        chunk = chunk * 10 + (uint64_t)(*b - '0');
        scale *= 10;
      }
      if (!mul_add(scale, chunk)) return false;
    }
    return true;
  }
  bool parse_hex(const char* b, const char* e) {   // hex digits of either case, no prefix
    *this = U256();
    if (b == e) return false;
    while (e - b > 1 && *b == '0') b++;
    if (e - b > 64) return false;
    for (int pos = 0; b < e; pos++) {   // digit pos from the right goes to its place
      const int d = hex_digit(*--e);
      if (d < 0) return false;
      v[pos / 16] |= (uint64_t)d << (4 * (pos % 16));
    }
    return true;
  }
  bool parse_number(const char* b, const char* e) {   // 0x / 0X and hex, or decimal
    if (e - b >= 2 && b[0] == '0' && (b[1] | 32) == 'x') return parse_hex(b + 2, e);
    return parse_dec(b, e);
  }
  void append_dec(std::string& out) const {   // 19 digits per pass
    uint64_t t[4] = {v[0], v[1], v[2], v[3]};
    uint64_t part[5];
    int parts = 0;
    while (t[0] | t[1] | t[2] | t[3]) {
      unsigned __int128 rem = 0;
      for (int k = 3; k >= 0; k--) {
        const unsigned __int128 cur = (rem << 64) | t[k];
        t[k] = (uint64_t)(cur / 10000000000000000000ull);
        rem = cur % 10000000000000000000ull;
      }
      part[parts++] = (uint64_t)rem;
    }
    if (!parts) {
      out.push_back('0');
      return;
    }
    char buf[24];
    out.append(buf, (size_t)snprintf(buf, sizeof(buf), "%llu", (unsigned long long)part[parts - 1]));
    for (int k = parts - 2; k >= 0; k--) out.append(buf, (size_t)snprintf(buf, sizeof(buf), "%019llu", (unsigned long long)part[k]));
  }
  std::string dec() const {
    std::string out;
    append_dec(out);
    return out;
  }
};

// "0x" + exactly 2 * bytes hex digits -> bytes
inline bool parse_hex_bytes(const Span& s, uint8_t* out, size_t bytes) {
  if (s.size() != 2 + 2 * bytes || s.b[0] != '0' || s.b[1] != 'x') return false;
  for (size_t i = 0; i < bytes; i++) {
    const int hi = hex_digit(s.b[2 + 2 * i]), lo = hex_digit(s.b[3 + 2 * i]);
    if (hi < 0 || lo < 0) return false;
    out[i] = (uint8_t)(16 * hi + lo);
  }
  return true;
}

// Neither JSON reader (this one and the tree of mini_json.hpp) follows objects and arrays nested deeper than this; the
// deepest real file nests 7. (The tree reader also counts a scalar or a key as a level, so it refuses one inside the
// 32nd container; the pull parser does not look at depth where it reads a scalar: that is the hot loop of a 1.6 GB file.)
constexpr int kJsonMaxDepth = 32;

// JSON, pulled over [p, e): the caller says what it expects next; whatever it does not know it skips.
struct Json {
  const char *p, *e;
  int depth = 0;
  [[noreturn]] void fail(const char* what) const { throw std::runtime_error(std::string("malformed JSON: ") + what); }
  // into a container; it is left with depth--. A failure abandons the parse, so nothing has to put depth back then.
  void enter() {
    if (++depth > kJsonMaxDepth) fail("nesting too deep");
  }
  void ws() {
    while (p < e && (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r')) p++;
  }
  bool at(char c) {
    ws();
    return p < e && *p == c;
  }
  bool take(char c) {
    if (!at(c)) return false;
    p++;
    return true;
  }
  void expect(char c, const char* what) {
    if (!take(c)) fail(what);
  }
  // a string without escapes (no key or number of these files has any): the characters between the quotes
  Span string() {
    expect('"', "a string was expected");
    const char* b = p;
    while (p < e && *p != '"') {
      if (*p == '\\') fail("an escape in a key or a number string");
      p++;
    }
    if (p >= e) fail("unterminated string");
    return Span{b, p++};
  }
  Span number() {
    ws();
    const char* b = p;
    while (p < e && (*p == '-' || *p == '+' || *p == '.' || (*p >= '0' && *p <= '9') || (*p | 32) == 'e')) p++;
    if (b == p) fail("a number was expected");
    return Span{b, p};
  }
  Span scalar() { return at('"') ? string() : number(); }   // a number, bare or as a string
  void skip() {   // any value; the strings and keys inside it may hold escapes
    ws();
    if (p >= e) fail("a value was expected");
    if (*p == '"') {
      p++;
      while (p < e && *p != '"') p += (*p == '\\' && p + 1 < e) ? 2 : 1;
      if (p >= e) fail("unterminated string");
      p++;
    } else if (*p == '{' || *p == '[') {
      enter();
      const bool obj = *p++ == '{';
      if (!take(obj ? '}' : ']')) {
        do {
          if (obj) {
            if (!at('"')) fail("a string was expected");
            skip();
            expect(':', "':' was expected");
          }
          skip();
        } while (take(','));
        expect(obj ? '}' : ']', obj ? "'}' was expected" : "']' was expected");
      }
      depth--;
    } else {
      const char* b = p;
      while (p < e && *p != ',' && *p != '}' && *p != ']' && *p != ' ' && *p != '\n' && *p != '\t' && *p != '\r') p++;
      if (b == p) fail("a value was expected");
    }
  }
  template <class Fn>
  void object(Fn member) {   // member(key) consumes the value
    enter();
    expect('{', "an object was expected");
    if (!take('}')) {
      do {
        const Span key = string();
        expect(':', "':' was expected");
        member(key);
      } while (take(','));
      expect('}', "'}' was expected");
    }
    depth--;
  }
  template <class Fn>
  uint64_t array(Fn element) {   // element(index) consumes the value; returns the length
    enter();
    expect('[', "an array was expected");
    uint64_t i = 0;
    if (!take(']')) {
      do element(i++);
      while (take(','));
      expect(']', "']' was expected");
    }
    depth--;
    return i;
  }
  void end() {
    ws();
    if (p != e) fail("text after the value");
  }
};

}  // namespace zkpoa
