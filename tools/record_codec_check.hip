// Host-only check of the setup commands' parsers, meant for a sanitizer build (no GPU, no HIP runtime call):
//   hipcc -std=c++17 -O1 -g --offload-host-only -Xarch_host -fsanitize=address,undefined \
//         -I zk-proof-of-assets_amd/csrc tools/record_codec_check.hip -o tools/record_codec_check
//   tools/record_codec_check [file.ptau | file.zkey]...
// U256::parse_number (csrc/host_text.hpp) on accepted and refused texts; RecordParams (csrc/phase2.hpp) written and parsed back
// for an empty record, a name alone and a beacon with a 255-byte name and a 255-byte beacon, and every truncation of the
// written bytes refused; for each file named, write_section7(parse_section7(x)) == x (.ptau) or the same for section 10
// (.zkey) over the section's bytes. Exit status 0 and "ok", or the first failure.
#include "binfile.hpp"
#include "host_text.hpp"
#include "phase1.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iterator>

namespace zkpoa {   // phase1.hpp declares them; only fresh_challenge and verify_records, which are not called here, use them
template <> Affine<HFq> host_generator<HFq>() { return {}; }
template <> Affine<HFq2> host_generator<HFq2>() { return {}; }
}

namespace p1 = zkpoa::phase1;
namespace p2 = zkpoa::phase2;

#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
      exit(1);                                                   \
    }                                                            \
  } while (0)

static bool parses(const std::string& s, uint8_t out[32]) {
  // an exact-size copy with no terminator: a read past `end` is the sanitizer's to find
  std::vector<char> v(s.begin(), s.end());
  zkpoa::U256 x;
  const bool ok = x.parse_number(v.data(), v.data() + v.size());
  x.to_le(out);
  return ok;
}

static void check_parser() {
  uint8_t a[32], b[32], c[32], want[32] = {0};
  CHECK(parses("305419896", a) && parses("0x12345678", b) && parses("0X12345678", c));
  want[0] = 0x78, want[1] = 0x56, want[2] = 0x34, want[3] = 0x12;
  CHECK(!memcmp(a, want, 32) && !memcmp(b, want, 32) && !memcmp(c, want, 32));
  CHECK(parses("0xabCDef", a) && a[0] == 0xef && a[1] == 0xcd && a[2] == 0xab);
  CHECK(parses("0", a) && parses("0x0", b) && !memcmp(a, b, 32));
  const std::string max_hex = "0x" + std::string(64, 'f');
  const std::string max_dec = "115792089237316195423570985008687907853269984665640564039457584007913129639935";
  memset(want, 0xff, 32);
  CHECK(parses(max_hex, a) && parses(max_dec, b) && !memcmp(a, want, 32) && !memcmp(b, want, 32));
  for (const char* bad : {"", "0x", "0X", "x", "12a", "0x12g", "1,", "1 ", " 1", "-1", "+1", "0x1,", "1x2", "00x1",
                          "115792089237316195423570985008687907853269984665640564039457584007913129639936"})
    CHECK(!parses(bad, a));
  CHECK(!parses("0x1" + std::string(64, '0'), a));
}

static void round_trip(const p2::RecordParams& r) {
  std::vector<uint8_t> w;
  r.write(w);
  CHECK(w.size() == r.len());
  {
    const std::vector<uint8_t> exact(w);   // capacity == size
    p2::RecordParams back;
    CHECK(back.parse(exact.data(), exact.size(), "refused") == exact.size());
    CHECK(back.type == r.type && back.name == r.name && back.beacon == r.beacon &&
          back.num_iterations_exp == (r.type == 1 ? r.num_iterations_exp : 0));
  }
  for (size_t cut = 0; cut < w.size(); cut++) {
    const std::vector<uint8_t> part(w.begin(), w.begin() + cut);
    bool threw = false;
    try {
      p2::RecordParams back;
      back.parse(part.data(), part.size(), "refused");
    } catch (const std::runtime_error& e) {
      threw = !strcmp(e.what(), "refused");
    }
    CHECK(threw);
  }
}

static void check_params() {
  p2::RecordParams r;
  round_trip(r);
  r.name = "alice";
  round_trip(r);
  r.type = 1;
  r.name = std::string(255, 'n');
  r.beacon.assign(255, 0xb7);
  r.num_iterations_exp = 30;
  r.check("beacon");
  round_trip(r);
  r.beacon.clear();   // a beacon of no bytes still carries its tags
  r.name.clear();
  round_trip(r);
  for (int what = 0; what < 3; what++) {
    p2::RecordParams bad;
    bad.type = 1;
    if (what == 0) bad.name = std::string(256, 'n');
    if (what == 1) bad.beacon.assign(256, 1);
    if (what == 2) bad.num_iterations_exp = 31;
    bool threw = false;
    try {
      bad.check("cmd");
    } catch (const std::runtime_error& e) {
      threw = strstr(e.what(), what == 2 ? "30" : "255 bytes") != nullptr;
    }
    CHECK(threw);
  }
  // a type above 1, an unknown tag, a length that runs past the params
  const uint8_t type2[8] = {2, 0, 0, 0, 0, 0, 0, 0}, tag9[9] = {0, 0, 0, 0, 1, 0, 0, 0, 9},
                long_name[11] = {0, 0, 0, 0, 3, 0, 0, 0, 1, 2, 'a'};
  for (const auto& b : {std::vector<uint8_t>(type2, type2 + 8), std::vector<uint8_t>(tag9, tag9 + 9),
                        std::vector<uint8_t>(long_name, long_name + 11)}) {
    bool threw = false;
    try {
      p2::RecordParams back;
      back.parse(b.data(), b.size(), "refused");
    } catch (const std::runtime_error&) {
      threw = true;
    }
    CHECK(threw);
  }
}

static void check_file(const char* path) {
  std::ifstream f(path, std::ios::binary);
  const std::vector<uint8_t> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::map<uint32_t, zkpoa::Sec> secs;
  const bool ptau = buf.size() >= 4 && !memcmp(buf.data(), "ptau", 4);
  CHECK(zkpoa::bin_scan(buf.data(), buf.size(), ptau ? "ptau" : "zkey", 1, secs) == zkpoa::kBinOk);
  const uint32_t id = ptau ? 7 : 10;
  CHECK(secs.count(id));
  const std::vector<uint8_t> x(buf.begin() + secs[id].off, buf.begin() + secs[id].off + secs[id].len);   // exact size
  size_t records;
  std::vector<uint8_t> y;
  if (ptau) {
    const std::vector<p1::Record> r = p1::parse_section7(x.data(), x.size());
    records = r.size();
    y = p1::write_section7(r);
  } else {
    const p2::Transcript t = p2::parse_section10(x.data(), x.size());
    records = t.records.size();
    y = p2::write_section10(t);
  }
  CHECK(x == y);
  for (size_t cut = x.size() > 300 ? x.size() - 300 : 0; cut < x.size(); cut++) {   // the tail: the last record's params
    const std::vector<uint8_t> part(x.begin(), x.begin() + cut);
    bool threw = false;
    try {
      if (ptau) (void)p1::parse_section7(part.data(), part.size());
      else (void)p2::parse_section10(part.data(), part.size());
    } catch (const std::runtime_error&) {
      threw = true;
    }
    CHECK(threw);
  }
  printf("%s: section %u, %zu record(s), %zu bytes round-trip\n", path, id, records, x.size());
}

int main(int argc, char** argv) {
  check_parser();
  check_params();
  for (int i = 1; i < argc; i++) check_file(argv[i]);
  printf("ok\n");
  return 0;
}
