// Ethereum Merkle-Patricia trie proofs, checked on the device (include/zkpoa_state_proof.h): the RLP the walk needs, a
// word-wise Keccak-256 absorb for nodes that lie 8-aligned in one blob, and the walk itself as a ZK_HD function, so that
// a host build can run the very same code over the same arrays (tools/mpt_host_check.hip does, under a sanitizer).
//
// Two kernels (state_proof.hip launches them): `hash`, one lane per NODE in an order bucketed by Keccak block count, so
// that a wave runs a uniform number of permutations, and `walk`, one lane per ITEM, which compares digests and follows
// the 64 nibbles of the key. A lane never reads outside its node: every length that RLP states is compared with what is
// left of the node before it is used, in 64-bit arithmetic that cannot wrap.
//
// Embedded children (a child node shorter than 32 bytes, stored inline as a list) are refused with a status of their
// own, kStatusChild. In the account trie they cannot occur: a leaf carries an account of at least 70 bytes (two 32-byte
// hashes, nonce, balance and their headers), so every node, and every node above it, is at least 32 bytes long and is
// referred to by hash. That keeps the walk free of recursion.
#pragma once
#include "keccak.hip.h"

namespace zkpoa {
namespace mpt {

// zkpoa_state_proof.h: ZKPOA_MPT_* (ABI)
enum Status : uint32_t {
  kStatusPresent = 0, kStatusAbsent = 1, kStatusNoNodes = 2, kStatusHash = 3, kStatusRlp = 4, kStatusChild = 5,
  kStatusShort = 6, kStatusLong = 7, kStatusHexPrefix = 8, kStatusAccount = 9
};

// ---- Keccak-256 of a message that starts on an 8-byte boundary: 64-bit loads, the 0x01 / 0x80 padding built in registers.
// No byte at or after msg + len is used: the last, partial word is masked, so what pads the blob does not matter; the
// word that holds byte len - 1 is read whole, so the buffer must reach the next multiple of 8 (state_proof.hip: rounded up).
ZK_HD void keccak256_words(const uint64_t* msg, uint32_t len, uint64_t (&digest)[4]) {
  uint64_t a[25];
#pragma unroll
  for (int i = 0; i < 25; i++) a[i] = 0;
  const uint32_t blocks = len / keccak::kRate + 1;
  const uint32_t full = len / 8, tail = len % 8;   // whole words; bytes of the partial one
  const uint32_t last = blocks * (keccak::kRate / 8) - 1;
#pragma unroll 1
  for (uint32_t blk = 0; blk < blocks; blk++) {
#pragma unroll
    for (int w = 0; w < keccak::kRate / 8; w++) {
      const uint32_t j = blk * (keccak::kRate / 8) + w;
      uint64_t word = 0;
      if (j < full) word = msg[j];
      else if (j == full) word = (tail ? (msg[j] & ((1ull << (8 * tail)) - 1)) : 0ull) | (1ull << (8 * tail));
      if (j == last) word |= 0x8000000000000000ull;
      a[w] ^= word;
    }
    keccak::f1600(a);
  }
#pragma unroll
  for (int i = 0; i < 4; i++) digest[i] = a[i];
}

// ---- RLP: one item of [p, end) of a node. Offsets are relative to the node's first byte.
struct Item {
  uint32_t payload, len;   // the string's bytes or the list's payload
  uint32_t next;           // the offset after the item
  bool list, ok;
};
ZK_HD Item rlp_item(const uint8_t* node, uint32_t p, uint32_t end) {
  Item it{0, 0, 0, false, false};
  if (p >= end) return it;
  const uint32_t b = node[p];
  uint64_t payload, len;
  if (b < 0x80) {
    payload = p;
    len = 1;
  } else {
    it.list = b >= 0xc0;
    const uint32_t base = it.list ? 0xc0 : 0x80;
    if (b - base <= 55) {
      payload = (uint64_t)p + 1;
      len = b - base;
    } else {
      const uint32_t ll = b - base - 55;   // 1..8 length bytes; a node is below 2^32 bytes, so more than 4 cannot fit
      if (ll > 4 || (uint64_t)p + 1 + ll > end) return it;
      len = 0;
      for (uint32_t k = 0; k < ll; k++) len = (len << 8) | node[p + 1 + k];
      payload = (uint64_t)p + 1 + ll;
    }
  }
  if (payload + len > end) return it;
  it.payload = (uint32_t)payload;
  it.len = (uint32_t)len;
  it.next = (uint32_t)(payload + len);
  it.ok = true;
  return it;
}

// nibble `pos` (0 = most significant of byte 0) of a key
ZK_HD uint32_t key_nibble(const uint8_t* key32, uint32_t pos) {
  const uint32_t b = key32[pos >> 1];
  return (pos & 1) ? (b & 15) : (b >> 4);
}

struct Walked {
  uint32_t status, where;
  uint64_t value_offset, value_len;   // status 0: the value's bytes within `nodes`
};

// One item's proof: nodes first .. last - 1 (root first), their digests already in `digests` (4 words per node).
// root: 4 words, the 32 bytes in order when stored little-endian, as the digests are.
ZK_HD Walked walk(const uint8_t* nodes, const uint64_t* node_offset, const uint32_t* node_length, const uint64_t* digests,
                  uint64_t first, uint64_t last, const uint8_t* key32, const uint64_t (&root)[4]) {
  Walked out{kStatusNoNodes, 0, 0, 0};
  if (first >= last) {
    // Keccak-256 of the RLP of the empty string, the root of a trie without keys
    if (root[0] == 0xa655cc1b171fe856ull && root[1] == 0x6ef8c092e64583ffull && root[2] == 0xc0ad6c991be0485bull &&
        root[3] == 0x21b463e3b52f6201ull)
      out.status = kStatusAbsent;
    return out;
  }
  uint64_t expect[4] = {root[0], root[1], root[2], root[3]};
  uint32_t pos = 0;        // nibbles of the key used up
  bool ended = false;      // the walk has its answer: whatever follows is one node too many
  for (uint64_t k = first; k < last; k++) {
    out.where = (uint32_t)(k - first);
    if (ended) {
      out.status = kStatusLong;
      out.value_offset = out.value_len = 0;
      return out;
    }
    const uint64_t* d = digests + 4 * k;
    if (d[0] != expect[0] || d[1] != expect[1] || d[2] != expect[2] || d[3] != expect[3]) {
      out.status = kStatusHash;
      return out;
    }
    const uint8_t* node = nodes + node_offset[k];
    const uint32_t len = node_length[k];
    out.status = kStatusRlp;
    const Item top = rlp_item(node, 0, len);
    if (!top.ok || !top.list || top.next != len) return out;
    // the items: their number, and the two a walk can need -- the path (item 0) and the one it follows or returns
    const uint32_t want = pos < 64 ? 1 + key_nibble(key32, pos) : 17;   // as a branch's item; a 2-item node: item 1
    Item head{0, 0, 0, false, false}, second = head, chosen = head;
    uint32_t count = 0;
    for (uint32_t p = top.payload; p < top.next; count++) {
      const Item it = rlp_item(node, p, top.next);
      if (!it.ok || count == 17) return out;
      if (count == 0) head = it;
      if (count == 1) second = it;
      if (count + 1 == want) chosen = it;
      p = it.next;
    }
    if (count != 2 && count != 17) return out;
    if (count == 17) {
      if (pos >= 64) {
        out.status = kStatusHexPrefix;
        return out;
      }
      pos++;
      if (!chosen.list && chosen.len == 0) {   // no such child: the key is not in the trie
        out.status = kStatusAbsent;
        ended = true;
        continue;
      }
      if (chosen.list || chosen.len != 32) {
        out.status = kStatusChild;
        return out;
      }
      for (int w = 0; w < 4; w++) {
        uint64_t x = 0;
        for (int j = 0; j < 8; j++) x |= (uint64_t)node[chosen.payload + 8 * w + j] << (8 * j);
        expect[w] = x;
      }
      out.status = kStatusShort;   // should the proof end here
      continue;
    }
    // extension or leaf: the hex-prefix path
    if (head.list) return out;
    out.status = kStatusHexPrefix;
    if (head.len == 0) return out;
    const uint32_t flag = node[head.payload] >> 4;
    if (flag > 3) return out;
    const bool odd = flag & 1, leaf = flag & 2;
    if (!odd && (node[head.payload] & 15)) return out;
    const uint32_t path_len = 2 * (head.len - 1) + (odd ? 1 : 0);
    if (path_len > 64 - pos) return out;
    bool same = true;
    for (uint32_t j = 0; j < path_len; j++) {
      const uint32_t q = odd ? j + 1 : j + 2;   // nibble index within the path's bytes
      const uint32_t b = node[head.payload + (q >> 1)];
      same = same && ((q & 1) ? (b & 15) : (b >> 4)) == key_nibble(key32, pos + j);
    }
    if (leaf) {
      if (second.list) {
        out.status = kStatusRlp;
        return out;
      }
      ended = true;
      if (same && path_len == 64 - pos) {
        out.status = kStatusPresent;
        out.value_offset = node_offset[k] + second.payload;
        out.value_len = second.len;
      } else {
        out.status = kStatusAbsent;
      }
      continue;
    }
    if (!same) {
      out.status = kStatusAbsent;
      ended = true;
      continue;
    }
    if (second.list || second.len != 32) {
      out.status = kStatusChild;
      return out;
    }
    pos += path_len;
    for (int w = 0; w < 4; w++) {
      uint64_t x = 0;
      for (int j = 0; j < 8; j++) x |= (uint64_t)node[second.payload + 8 * w + j] << (8 * j);
      expect[w] = x;
    }
    out.status = kStatusShort;
  }
  if (out.status == kStatusShort) out.where = (uint32_t)(last - first);   // where the missing node would stand
  if (out.status != kStatusPresent) out.value_offset = out.value_len = 0;
  return out;
}

// The value of an account leaf: a list of nonce, balance, storage root, code hash. false: it is no account.
struct Account {
  uint64_t nonce;
  uint8_t balance[32], storage_root[32], code_hash[32];   // the balance big-endian
};
ZK_HD bool account(const uint8_t* value, uint32_t len, Account& acc) {
  const Item top = rlp_item(value, 0, len);
  if (!top.ok || !top.list || top.next != len) return false;
  Item f[4];
  uint32_t p = top.payload;
  for (int i = 0; i < 4; i++) {
    f[i] = rlp_item(value, p, top.next);
    if (!f[i].ok || f[i].list) return false;
    p = f[i].next;
  }
  if (p != top.next) return false;
  if (f[0].len > 8 || f[1].len > 32 || f[2].len != 32 || f[3].len != 32) return false;
  if ((f[0].len && value[f[0].payload] == 0) || (f[1].len && value[f[1].payload] == 0)) return false;   // leading zero
  acc.nonce = 0;
  for (uint32_t j = 0; j < f[0].len; j++) acc.nonce = (acc.nonce << 8) | value[f[0].payload + j];
  for (uint32_t j = 0; j < 32; j++) {
    acc.balance[j] = j + f[1].len >= 32 ? value[f[1].payload + (j + f[1].len - 32)] : 0;
    acc.storage_root[j] = value[f[2].payload + j];
    acc.code_hash[j] = value[f[3].payload + j];
  }
  return true;
}

}  // namespace mpt
}  // namespace zkpoa
