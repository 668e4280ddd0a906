// Host check of the entry writer of csrc/host_files.hpp (put_text, put_entries with and without its round hook,
// write_entries): the header's own text, compiled by g++ alone, no HIP and no device.
// Build: g++ -O2 -std=c++17 -pthread -I zk-proof-of-assets_amd/csrc tools/entry_writer_check.cpp -o entry_writer_check
// Use:   entry_writer_check DIR N      (tests/test_entry_writer.py drives it; ENTRY_WRITER_CHECK_FLAGS adds compiler flags,
//                                       e.g. "-O1 -g -fsanitize=address,undefined": no GPU, never on a GPU machine)
// Writes N entries three ways into DIR and reads each file back: prints "ok N entries, R rounds" and exits 0, or
// "FAILED: <what>" and exits 1.
#include "host_files.hpp"

#include <fstream>
#include <sstream>

using namespace zkpoa;

static std::string slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  std::stringstream s;
  s << f.rdbuf();
  return s.str();
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const std::string dir = argv[1];
  const uint64_t n = strtoull(argv[2], nullptr, 10);
  try {
    auto entry = [](std::string& o, uint64_t i) { o += (i ? ",\n  " : "\n  ") + std::to_string(i * i); };
    std::string want = "[";
    for (uint64_t i = 0; i < n; i++) entry(want, i);
    want += n ? "\n]" : "]";
    // head + entries + tail in one call
    write_entries(dir + "/a.json", "[", n ? "\n]" : "]", n, 12, entry);
    if (slurp(dir + "/a.json") != want) throw std::runtime_error("write_entries wrote other bytes");
    // the round hook: every round is announced once, in order, before its entries are formatted; what it fetched is
    // what the round's entries see
    AtomicFile fo((dir + "/b.json").c_str());
    uint64_t off = 0, rounds = 0, next = 0;
    std::vector<uint64_t> fetched;
    put_text(fo, off, "[");
    put_entries(fo, off, n, 64, 12,
                [&](uint64_t i0, uint64_t count) {
                  if (i0 != next || count == 0 || count > kEntryRound) throw std::runtime_error("rounds out of order");
                  next = i0 + count;
                  rounds++;
                  fetched.assign(count, 0);
                  for (uint64_t j = 0; j < count; j++) fetched[j] = (i0 + j) * (i0 + j);
                },
                [&](std::string& o, uint64_t i) { o += (i ? ",\n  " : "\n  ") + std::to_string(fetched[i - (next - fetched.size())]); });
    put_text(fo, off, n ? "\n]" : "]");
    if (next != n) throw std::runtime_error("the rounds do not cover the entries");
    if (slurp(dir + "/b.json") != "") throw std::runtime_error("a file appeared before its commit");
    fo.commit();
    if (slurp(dir + "/b.json") != want) throw std::runtime_error("put_entries with a round hook wrote other bytes");
    // an entry that throws: the error comes out, and nothing is left under the name
    bool threw = false;
    try {
      write_entries(dir + "/c.json", "[", "]", n + 1, 12, [&](std::string&, uint64_t i) {
        if (i == n) throw std::runtime_error("entry");
      });
    } catch (const std::runtime_error&) {
      threw = true;
    }
    if (!threw || slurp(dir + "/c.json") != "") throw std::runtime_error("a failed write left a file or no error");
    printf("ok %llu entries, %llu rounds\n", (unsigned long long)n, (unsigned long long)rounds);
    return 0;
  } catch (const std::exception& e) {
    printf("FAILED: %s\n", e.what());
    return 1;
  }
}
