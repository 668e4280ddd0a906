// The proofs file of `zkpoa-audit --state-proofs` and zkpoa_anon_set_state_check_file: JSON Lines, one object per line,
// each either what `eth_getProof(address, [], block)` returns or its JSON-RPC envelope with that object under "result".
// Read are "address" (0x + 40 hex digits, either case) and "accountProof" (an array of 0x-hex strings, root first);
// every other member is skipped, the node's claimed "balance" included: nothing the file claims is trusted, only what
// its nodes prove. Lines come in any order; blank lines are skipped.
//
// The file is mapped and handed out in slabs of lines, bounded by proof count and by text bytes (a node's bytes are half
// its text). The host threads go over a slab's lines twice, as anon_set_file.hpp goes over the csv: first counting nodes
// and bytes, so that every line knows where its nodes go, then writing them straight into the 8-aligned blob that
// include/zkpoa_state_proof.h describes. A malformed line is an error that names its number. Host only, no HIP.
#pragma once
#include "anon_set_file.hpp"

namespace zkpoa {

struct ProofSlab {
  uint64_t items = 0, first_line = 0;   // first_line: the file's line number (from 1) of item 0
  std::vector<uint8_t> address20;       // items x 20 B
  std::vector<uint64_t> first_node;     // items + 1
  std::vector<uint64_t> node_offset;    // T
  std::vector<uint32_t> node_length;    // T
  std::vector<uint8_t> nodes;           // the blob, zero between nodes
};

// One line: node(hex digits begin, end) for every node in order; -> the address's 40 hex digits.
template <class Fn>
inline Span proof_line(const char* b, const char* e, Fn node) {
  Json js{b, e};
  Span address{nullptr, nullptr};
  bool proof = false;
  auto inner = [&](const Span& key) {
    if (key.is("address")) {
      address = js.string();
    } else if (key.is("accountProof")) {
      if (proof) js.fail("\"accountProof\" twice");
      proof = true;
      js.array([&](uint64_t) {
        const Span h = js.string();
        if (h.size() < 2 || h.b[0] != '0' || (h.b[1] | 32) != 'x') js.fail("a node is not 0x-prefixed hex");
        if (h.size() % 2) js.fail("a node has an odd number of hex digits");
        if (h.size() / 2 - 1 > (1u << 20)) js.fail("a node of more than 2^20 bytes");
        node(h.b + 2, h.e);
      });
    } else {
      js.skip();
    }
  };
  bool enveloped = false;
  js.object([&](const Span& key) {
    if (key.is("result")) {
      if (enveloped || proof || address.b) js.fail("\"result\" beside a proof");
      enveloped = true;
      js.object(inner);
    } else if (enveloped && (key.is("address") || key.is("accountProof"))) {
      js.fail("\"result\" beside a proof");
    } else {
      inner(key);
    }
  });
  js.end();
  if (!address.b || !proof) js.fail(enveloped || address.b || proof ? "\"address\" and \"accountProof\" are both needed"
                                                                      : "neither a proof nor an envelope with \"result\"");
  if (address.size() != 42 || address.b[0] != '0' || (address.b[1] | 32) != 'x') js.fail("\"address\" is not 0x and 40 hex digits");
  for (const char* q = address.b + 2; q < address.e; q++)
    if (hex_digit(*q) < 0) js.fail("\"address\" is not 0x and 40 hex digits");
  return Span{address.b + 2, address.e};
}

inline void hex_to_bytes(const char* b, const char* e, uint8_t* out, Json& js_for_errors) {
  for (; b < e; b += 2) {
    const int hi = hex_digit(b[0]), lo = hex_digit(b[1]);
    if (hi < 0 || lo < 0) js_for_errors.fail("a character that is no hex digit");
    *out++ = (uint8_t)(16 * hi + lo);
  }
}

struct ProofFile {
  MappedFile map;
  const char* cur;
  uint64_t line_no = 0;   // lines consumed so far
  explicit ProofFile(const char* path) : map(path), cur(map.begin()) {}

  // The next slab: at most max_items proofs and, but for a single longer line, at most max_text bytes of text.
  // false: the file is used up (slab.items = 0).
  bool next(ProofSlab& slab, uint64_t max_items, uint64_t max_text) {
    struct Line {
      const char *b, *e;
      uint64_t no, nodes, bytes;
    };
    std::vector<Line> lines;
    const char* end = map.end();
    uint64_t text = 0;
    while (cur && cur < end && lines.size() < max_items) {
      const char* nl = static_cast<const char*>(memchr(cur, '\n', (size_t)(end - cur)));
      const char* le = nl ? nl : end;
      const char *tb = cur, *te = le;
      while (tb < te && (*tb == ' ' || *tb == '\t' || *tb == '\r')) tb++;
      while (te > tb && (te[-1] == ' ' || te[-1] == '\t' || te[-1] == '\r')) te--;
      if (tb < te) {
        if (!lines.empty() && text + (uint64_t)(te - tb) > max_text) break;
        text += (uint64_t)(te - tb);
        lines.push_back(Line{tb, te, line_no + 1, 0, 0});
      }
      line_no++;
      cur = nl ? nl + 1 : end;
    }
    slab = ProofSlab();
    slab.items = lines.size();
    if (lines.empty()) return false;
    slab.first_line = lines[0].no;
    auto numbered = [](const Line& l, const std::exception& ex) {
      return std::runtime_error("state proofs: line " + std::to_string(l.no) + ": " + ex.what());
    };
    parallel_ranges(lines.size(), 64, [&](unsigned, uint64_t lo, uint64_t hi) {
      for (uint64_t i = lo; i < hi; i++) {
        Line& l = lines[i];
        try {
          proof_line(l.b, l.e, [&](const char* hb, const char* he) {
            l.nodes++;
            l.bytes += ((uint64_t)(he - hb) / 2 + 7) & ~7ull;
          });
        } catch (const std::exception& ex) {
          throw numbered(l, ex);
        }
      }
    });
    slab.first_node.assign(lines.size() + 1, 0);
    std::vector<uint64_t> at(lines.size() + 1, 0);
    for (size_t i = 0; i < lines.size(); i++) {
      slab.first_node[i + 1] = slab.first_node[i] + lines[i].nodes;
      at[i + 1] = at[i] + lines[i].bytes;
    }
    if (slab.first_node.back() >> 32) throw std::runtime_error("state proofs: 2^32 nodes or more in one slab");
    slab.address20.resize(20 * lines.size());
    slab.node_offset.resize(slab.first_node.back());
    slab.node_length.resize(slab.first_node.back());
    slab.nodes.assign(at.back(), 0);
    parallel_ranges(lines.size(), 64, [&](unsigned, uint64_t lo, uint64_t hi) {
      for (uint64_t i = lo; i < hi; i++) {
        const Line& l = lines[i];
        Json where{l.b, l.e};   // for the messages of the second pass
        try {
          uint64_t k = slab.first_node[i], off = at[i];
          const Span a = proof_line(l.b, l.e, [&](const char* hb, const char* he) {
            const uint64_t len = (uint64_t)(he - hb) / 2;
            slab.node_offset[k] = off;
            slab.node_length[k] = (uint32_t)len;
            hex_to_bytes(hb, he, slab.nodes.data() + off, where);
            k++;
            off += (len + 7) & ~7ull;
          });
          hex_to_bytes(a.b, a.e, slab.address20.data() + 20 * i, where);
        } catch (const std::exception& ex) {
          throw numbered(l, ex);
        }
      }
    });
    return true;
  }
};

}  // namespace zkpoa
