// The ceremony file (.ptau) as the `powersoftau` commands open it (PtauInput) and write it (PtauFile), the piece size of a
// command that streams its sections 2-6 through HBM (ptau_piece) and the hash form of those sections
// (hash_form_ptau_sections). Host code over csrc/setup_common.hip.h and csrc/phase1.hpp: no kernel is defined here.
#pragma once
#include "phase1.hpp"
#include "setup_common.hip.h"

namespace {

// An input: mapped for its section table, section 7 and single points (the point sections stream with pread), sections
// 1-7 present and of the lengths the header's power gives. records: section 7 is parsed here; a command with checks of
// its own that come first (`verify`: sections 12-15) calls parse_records() after them, `prepare phase2` copies the
// section unread. preparable: the power is checked (ptau_check_preparable) before the section lengths, so that no file
// of power 28 need exist to be refused.
struct PtauInput {
  MappedFile f;
  std::map<uint32_t, Sec> ps;
  PtauShape shape;
  std::vector<zkpoa::phase1::Record> records;
  explicit PtauInput(const char* path, bool with_records = true, bool preparable = false) : f(path), ps(bin_sections(f, "ptau", 1, "ptau")) {
    if (preparable && ps.count(1)) ptau_check_preparable(ptau_header(f, ps[1]));
    shape = ptau_power_sections(f, ps);
    if (with_records) parse_records();
  }
  void parse_records() { records = zkpoa::phase1::parse_section7(f.p + ps[7].off, ps[7].len); }
  enum Lagrange { kNone, kSome, kAll };   // of sections 12-15 (Lagrange form)
  Lagrange lagrange() const {
    const size_t n = ps.count(12) + ps.count(13) + ps.count(14) + ps.count(15);
    return n == 4 ? kAll : (n ? kSome : kNone);
  }
  // a command whose output holds new powers writes sections 1-7 only
  void warn_lagrange_dropped(const char* command) const {
    if (lagrange() != kNone)
      fprintf(stderr, "zkpoa: %s: sections 12-15 (Lagrange form) of the input are dropped: they would be stale; "
                      "run `powersoftau prepare phase2` on the result\n", command);
  }
};

// a ceremony file of sections 1-7 whose section 7 has len7 bytes, sized, its table and its header (section 1) written
struct PtauFile : SectionFile {
  static std::array<uint64_t, 7> lens(uint32_t power, uint64_t len7) {
    std::array<uint64_t, 7> l{{4 + 32 + 8, 0, 0, 0, 0, 0, len7}};
    for (const PowerSec& sc : ptau_power_secs(power)) l[sc.id - 1] = sc.bytes();
    return l;
  }
  static constexpr uint32_t kIds[7] = {1, 2, 3, 4, 5, 6, 7};
  const uint32_t power;
  PtauFile(const char* path, uint32_t pw, uint32_t ceremony, uint64_t len7)
      : SectionFile(path, "ptau", kIds, lens(pw, len7).data(), 7), power(pw) {
    uint8_t s1[44];
    const uint32_t n8 = 32;
    memcpy(s1, &n8, 4);
    memcpy(s1 + 4, HFqParams::P, 32);
    memcpy(s1 + 36, &power, 4);
    memcpy(s1 + 40, &ceremony, 4);
    put(1, s1, 44);
  }
};

// points per piece of a command that streams sections 2-6 through HBM: bytes_per_point of device buffers (what the
// command allocates per point of a piece) in a quarter of the free HBM, 2 x 128 MiB of pinned read-back buffers at most;
// from power 20 up no section is ever whole on the host
uint64_t ptau_piece(zkpoa_context* ctx, uint64_t N, uint64_t bytes_per_point) {
  constexpr uint64_t kMaxPiece = 1ull << 20;
  uint64_t piece = (uint64_t)ctx->opt_ptau_piece_points;
  if (!piece) piece = piece_from_free_hbm(bytes_per_point, 1ull << 12, kMaxPiece);
  return std::min<uint64_t>(std::min<uint64_t>(piece, kMaxPiece), 2 * N);
}

// The hash form of sections 2-6 of a ceremony file of 2^power (fd, its section table) into hs's hasher: what a
// nextChallenge covers and a challenge file holds. The sections stream through d_piece (piece_points x 128 B of device
// memory; upload_ms: as for_each_piece). Stream: HashStream of csrc/phase2_dev.hip.h, left out of this header so that a
// unit that only opens a file (csrc/ptau_prepare.hip) does not take in its kernels.
template <class Stream>
void hash_form_ptau_sections(zkpoa_context* ctx, Stream& hs, int fd, const std::map<uint32_t, Sec>& ps, uint32_t power,
                             void* d_piece, uint64_t piece_points, double* upload_ms = nullptr) {
  for (const PowerSec& sc : ptau_power_secs(power))
    for_each_piece(ctx, fd, ps.at(sc.id).off, sc.count, sc.unit(), piece_points, d_piece,
                   [&](uint64_t, uint64_t cnt) { hs.points(d_piece, cnt, sc.group, false); }, upload_ms);
}

}  // namespace
