// A stable index of the anonymity set's addresses: the row numbers ordered by (address, row), by an LSD radix sort over
// the bytes of the 32-byte keys, and the adjacent compare over that order which finds duplicate addresses exactly.
//
// The published set is the prover's file, so nothing here may depend on how its keys are distributed: no hashing, no
// pass whose cost grows with the size of a group of equal keys. Only the permutation moves (4 B per row and pass); a
// pass reads its digit from the key in place, keys[row * 32 + byte].
//   diff     : OR over all rows of key ^ key[0], 256 bits. A byte position whose OR is zero holds one value in every
//              row: sorting by it moves nothing, the pass is skipped (real addresses: the top 12 bytes, 20 passes left).
//              It costs one streaming read of the keys whatever they hold.
//   count    : per pass, one workgroup of 256 per tile of 2048 rows: the tile's histogram of the pass's digit, stored
//              plainly at hist[digit * tiles + tile] -- no global atomics.
//   scan     : the shared u32 scan (msm.hip.h) over that table: digit-major, tile-minor, so the exclusive prefix is where
//              each (digit, tile) run starts in the output, tiles in order.
//   scatter  : ranks the tile again the same way and writes every row to run start + rank.
// Stability. lds_count_rank of msm_sort.hip.h orders the entries of a bucket by the arrival of LDS atomics, which is
// arbitrary between waves; an LSD sort needs every pass to keep the previous order. Here a tile's rows are taken in the
// order (wave, round, lane) -- row e = tile * 2048 + wave * 512 + round * 64 + lane -- and ranked without atomics: within
// a round the lanes with one digit are found by 8 ballots over the digit's bits and ranked by lane number; a wave keeps
// its own running count per digit in LDS, read by the whole wave in one instruction before the group's first lane
// stores the sum back; the waves of a tile are ordered by the prefix of their counts, the tiles by the scan.
// All equal keys, two values, keys sharing 31 bytes: the same instructions run as for random keys, fewer passes.
//   find     : what queries the index. One lane per query, a lower-bound and an upper-bound binary search over
//              keys[perm[.]]: the number of rows with the query's key and, the order being stable, the lowest of them.
#pragma once
#include "msm.hip.h"   // the u32 scan
#include "zkpoa_internal.hpp"

namespace zkpoa {

constexpr uint32_t kAnonWg = 256;      // threads of a workgroup: 4 waves
constexpr uint32_t kAnonRounds = 8;    // rows per thread
constexpr uint32_t kAnonTile = kAnonWg * kAnonRounds;
constexpr uint32_t kAnonNoRow = 0xffffffffu;   // n < 2^32: no row has this number

inline uint32_t anon_tiles(uint64_t n) { return (uint32_t)((n + kAnonTile - 1) / kAnonTile); }

// out8 |= key[r] ^ key[0] over all rows (out8 zeroed by the caller); keys as 2 n vectors of 16 B
static __global__ __launch_bounds__(kAnonWg) void anon_diff_kernel(const uint4* __restrict__ keys, uint64_t n,
                                                                   uint32_t* __restrict__ out8) {
  const uint64_t total = 2 * n, stride = (uint64_t)gridDim.x * kAnonWg;   // even: a thread stays on one half of the key
  uint64_t i = (uint64_t)blockIdx.x * kAnonWg + threadIdx.x;
  const uint4 first = keys[threadIdx.x & 1u];
  uint4 acc = make_uint4(0, 0, 0, 0);
  for (; i < total; i += stride) {
    const uint4 v = keys[i];
    acc.x |= v.x ^ first.x;
    acc.y |= v.y ^ first.y;
    acc.z |= v.z ^ first.z;
    acc.w |= v.w ^ first.w;
  }
#pragma unroll
  for (int o = 2; o < 64; o <<= 1) {   // lanes of one parity hold the same half
    acc.x |= __shfl_xor(acc.x, o);
    acc.y |= __shfl_xor(acc.y, o);
    acc.z |= __shfl_xor(acc.z, o);
    acc.w |= __shfl_xor(acc.w, o);
  }
  const uint32_t lane = threadIdx.x & 63u;
  if (lane < 2) {   // one atomic per wave, half and word, and only where a bit is set
    uint32_t* dst = out8 + 4 * lane;
    if (acc.x) atomicOr(dst + 0, acc.x);
    if (acc.y) atomicOr(dst + 1, acc.y);
    if (acc.z) atomicOr(dst + 2, acc.z);
    if (acc.w) atomicOr(dst + 3, acc.w);
  }
}

static __global__ __launch_bounds__(kAnonWg) void anon_iota_kernel(uint32_t* __restrict__ perm, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * kAnonWg + threadIdx.x;
  if (i < n) perm[i] = (uint32_t)i;
}

// The rows of tile `tile` in the order of perm_in (nullptr: the identity), their digit (byte `byte` of the key) and
// their rank among the rows of the same wave with the same digit. cnt[wave][digit] is left holding each wave's counts;
// the caller synchronises before it reads another wave's.
ZK_DEV void anon_tile_rank(const uint8_t* __restrict__ keys, const uint32_t* __restrict__ perm_in, uint64_t n, uint32_t byte,
                           uint32_t tile, volatile uint32_t (*cnt)[256], uint32_t (&row)[kAnonRounds],
                           uint32_t (&dig)[kAnonRounds], uint32_t (&loc)[kAnonRounds]) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t w = 0; w < kAnonWg / 64; w++) cnt[w][threadIdx.x] = 0;
  const uint64_t base = (uint64_t)tile * kAnonTile + wave * (64 * kAnonRounds) + lane;
#pragma unroll
  for (uint32_t k = 0; k < kAnonRounds; k++) {
    const uint64_t e = base + 64 * k;
    row[k] = e < n ? (perm_in ? perm_in[e] : (uint32_t)e) : kAnonNoRow;
  }
#pragma unroll
  for (uint32_t k = 0; k < kAnonRounds; k++) dig[k] = row[k] < n ? keys[(uint64_t)row[k] * 32 + byte] : 0;   // (no row: >= n)
  __syncthreads();
  const uint64_t lanes_below = (1ull << lane) - 1;
#pragma unroll
  for (uint32_t k = 0; k < kAnonRounds; k++) {
    const bool valid = row[k] != kAnonNoRow;
    uint64_t same = __ballot(valid);   // the valid lanes of this round with this lane's digit
#pragma unroll
    for (uint32_t b = 0; b < 8; b++) {
      const bool bit = (dig[k] >> b) & 1u;
      const uint64_t with = __ballot(bit);
      same &= bit ? with : ~with;
    }
    const uint32_t before = (uint32_t)__popcll(same & lanes_below);
    // one load for the whole wave, then one store by each group's first lane: a wave's LDS accesses keep their order
    const uint32_t seen = cnt[wave][dig[k]];
    if (valid && before == 0) cnt[wave][dig[k]] = seen + (uint32_t)__popcll(same);
    loc[k] = seen + before;
  }
}

// hist[digit * tiles + tile] <- rows of the tile with that digit
static __global__ __launch_bounds__(kAnonWg) void anon_count_kernel(const uint8_t* __restrict__ keys,
                                                                    const uint32_t* __restrict__ perm_in, uint64_t n,
                                                                    uint32_t byte, uint32_t tiles, uint32_t* __restrict__ hist) {
  __shared__ uint32_t cnt[kAnonWg / 64][256];
  uint32_t row[kAnonRounds], dig[kAnonRounds], loc[kAnonRounds];
  anon_tile_rank(keys, perm_in, n, byte, blockIdx.x, cnt, row, dig, loc);
  __syncthreads();
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t w = 0; w < kAnonWg / 64; w++) sum += cnt[w][threadIdx.x];
  hist[(uint64_t)threadIdx.x * tiles + blockIdx.x] = sum;
}

// start[digit * tiles + tile]: the exclusive scan of hist. perm_out[start + rank in the tile] <- row
static __global__ __launch_bounds__(kAnonWg) void anon_scatter_kernel(const uint8_t* __restrict__ keys,
                                                                      const uint32_t* __restrict__ perm_in, uint64_t n,
                                                                      uint32_t byte, uint32_t tiles,
                                                                      const uint32_t* __restrict__ start,
                                                                      uint32_t* __restrict__ perm_out) {
  __shared__ uint32_t cnt[kAnonWg / 64][256];
  __shared__ uint32_t first[kAnonWg / 64][256];   // where a wave's rows of a digit begin in the output
  uint32_t row[kAnonRounds], dig[kAnonRounds], loc[kAnonRounds];
  anon_tile_rank(keys, perm_in, n, byte, blockIdx.x, cnt, row, dig, loc);
  __syncthreads();
  uint32_t run = start[(uint64_t)threadIdx.x * tiles + blockIdx.x];
#pragma unroll
  for (uint32_t w = 0; w < kAnonWg / 64; w++) {
    first[w][threadIdx.x] = run;
    run += cnt[w][threadIdx.x];
  }
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t k = 0; k < kAnonRounds; k++)
    if (row[k] != kAnonNoRow) {
      const uint64_t dst = (uint64_t)first[wave][dig[k]] + loc[k];
      if (dst < n) perm_out[dst] = row[k];   // always true for a consistent table; a bound all the same
    }
}

// Over the sorted order: res[0] += rows whose key equals that of the row before them in the order (stable: an earlier
// row), res[1] = min over those of (row << 32 | the row before), res[2] |= 1 when the order is not the identity.
static __global__ __launch_bounds__(kAnonWg) void anon_adjacent_kernel(const uint4* __restrict__ keys,
                                                                       const uint32_t* __restrict__ perm, uint64_t n,
                                                                       unsigned long long* __restrict__ res) {
  __shared__ unsigned long long sh[3][kAnonWg / 64];
  unsigned long long dups = 0, pair = ~0ull, moved = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kAnonWg;
  for (uint64_t i = (uint64_t)blockIdx.x * kAnonWg + threadIdx.x; i < n; i += stride) {
    const uint32_t a = perm[i];
    if (a != i) moved = 1;   // (also whatever is no row number at all)
    if (i == 0) continue;
    const uint32_t p = perm[i - 1];
    if (a >= n || p >= n) continue;   // no permutation of the rows: reported as moved, never followed into the keys
    const uint4 a0 = keys[2 * (uint64_t)a], a1 = keys[2 * (uint64_t)a + 1];
    const uint4 p0 = keys[2 * (uint64_t)p], p1 = keys[2 * (uint64_t)p + 1];
    const uint32_t d = (a0.x ^ p0.x) | (a0.y ^ p0.y) | (a0.z ^ p0.z) | (a0.w ^ p0.w) | (a1.x ^ p1.x) | (a1.y ^ p1.y) |
                       (a1.z ^ p1.z) | (a1.w ^ p1.w);
    if (d == 0) {
      dups++;
      const unsigned long long pr = ((unsigned long long)a << 32) | p;
      pair = pr < pair ? pr : pair;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    dups += __shfl_xor(dups, o);
    const unsigned long long q = __shfl_xor(pair, o);
    pair = q < pair ? q : pair;
    moved |= __shfl_xor(moved, o);
  }
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sh[0][wave] = dups;
    sh[1][wave] = pair;
    sh[2][wave] = moved;
  }
  __syncthreads();
  if (threadIdx.x == 0) {   // one atomic per workgroup and result, and only when it changes something
#pragma unroll
    for (uint32_t w = 1; w < kAnonWg / 64; w++) {
      dups += sh[0][w];
      pair = sh[1][w] < pair ? sh[1][w] : pair;
      moved |= sh[2][w];
    }
    if (dups) atomicAdd(res + 0, dups);
    if (pair != ~0ull) atomicMin(res + 1, pair);
    if (moved) atomicOr(res + 2, 1ull);
  }
}

// The index's order: keys as 256-bit little-endian integers, most significant limb first (the last pass of the sort is
// byte 31). -1, 0, 1 for a below, equal to, above b; a key is two 16-byte vectors.
ZK_DEV int anon_key_compare(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  const uint32_t a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
  const uint32_t b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
  int c = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) c = a[j] != b[j] ? (a[j] < b[j] ? -1 : 1) : c;   // the highest limb that differs decides
  return c;
}

// One lane per query: the equal run of the query in keys[perm[.]], by a lower-bound and an upper-bound binary search.
// count <- its length, first <- the row at its start (stable index: the lowest such row), kAnonNoRow for an empty run.
// Every probe is one dependent 4 B read of perm and two 16 B reads of the key. An entry of perm that is no row number is
// not followed: the query reports no match.
static __global__ __launch_bounds__(kAnonWg) void anon_find_kernel(const uint4* __restrict__ keys, uint64_t n,
                                                                   const uint32_t* __restrict__ perm,
                                                                   const uint4* __restrict__ queries, uint64_t m,
                                                                   uint32_t* __restrict__ first, uint32_t* __restrict__ count) {
  const uint64_t i = (uint64_t)blockIdx.x * kAnonWg + threadIdx.x;
  if (i >= m) return;
  const uint4 q0 = queries[2 * i], q1 = queries[2 * i + 1];
  bool sound = true;
  // lower bound: the first position whose key is not below the query; above: the lowest position seen to hold a larger key
  uint64_t lo = 0, hi = n, above = n;
  while (lo < hi && sound) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    const uint32_t row = perm[mid];
    if (row >= n) {
      sound = false;
      break;
    }
    const int c = anon_key_compare(keys[2 * (uint64_t)row], keys[2 * (uint64_t)row + 1], q0, q1);
    if (c < 0) lo = mid + 1;
    else hi = mid;
    if (c > 0) above = mid;
  }
  const uint64_t begin = lo;
  // upper bound: the first position in [begin, above) whose key is above the query
  hi = above;
  while (lo < hi && sound) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    const uint32_t row = perm[mid];
    if (row >= n) {
      sound = false;
      break;
    }
    const int c = anon_key_compare(keys[2 * (uint64_t)row], keys[2 * (uint64_t)row + 1], q0, q1);
    if (c <= 0) lo = mid + 1;
    else hi = mid;
  }
  const bool found = sound && lo > begin;
  count[i] = found ? (uint32_t)(lo - begin) : 0;
  first[i] = found ? perm[begin] : kAnonNoRow;
}

// Device memory of one index: the other permutation buffer, the (digit, tile) table and its scan
struct AnonSetWork {
  uint32_t tiles;
  DevBuf perm2, hist, start, block_sums, misc;   // misc: 8 words of the diff, then the scan's total
  explicit AnonSetWork(uint64_t n)
      : tiles(anon_tiles(n)), perm2(n * 4), hist((size_t)256 * tiles * 4), start(((size_t)256 * tiles + 1) * 4),
        block_sums((((size_t)256 * tiles + kScanTile - 1) / kScanTile + 1) * 4), misc(64) {}
};

// d_perm <- the stable order of the n keys, enqueued on st; one small read-back in the middle (which bytes differ at
// all). Returns the number of passes that ran.
inline int anon_set_index(hipStream_t st, AnonSetWork& wk, const void* d_keys, uint64_t n, uint32_t* d_perm) {
  if (n == 0) return 0;
  if (n >> 32) throw HipError("anon set: at most 2^32 - 1 rows");
  uint32_t* diff_dev = static_cast<uint32_t*>(wk.misc.p);
  ZK_HIP(hipMemsetAsync(diff_dev, 0, 64, st));
  const uint64_t vecs = 2 * n;
  const uint32_t diff_blocks = (uint32_t)std::min<uint64_t>(1024, (vecs + kAnonWg - 1) / kAnonWg);
  hipLaunchKernelGGL(anon_diff_kernel, dim3(diff_blocks), dim3(kAnonWg), 0, st, static_cast<const uint4*>(d_keys), n, diff_dev);
  uint8_t diff[32];
  ZK_HIP(hipMemcpyAsync(diff, diff_dev, 32, hipMemcpyDeviceToHost, st));
  ZK_HIP(hipStreamSynchronize(st));
  int passes = 0;
  for (int b = 0; b < 32; b++) passes += diff[b] != 0;
  if (passes == 0) {   // every key is the same (or there is one): the order is the file's
    hipLaunchKernelGGL(anon_iota_kernel, dim3((uint32_t)((n + kAnonWg - 1) / kAnonWg)), dim3(kAnonWg), 0, st, d_perm, n);
    return 0;
  }
  const uint8_t* keys = static_cast<const uint8_t*>(d_keys);
  uint32_t* hist = static_cast<uint32_t*>(wk.hist.p);
  uint32_t* start = static_cast<uint32_t*>(wk.start.p);
  uint32_t* bufs[2] = {d_perm, static_cast<uint32_t*>(wk.perm2.p)};
  int left = passes;   // the last pass writes d_perm: pass j of P writes buffer (P - 1 - j) & 1
  const uint32_t* in = nullptr;
  for (uint32_t b = 0; b < 32; b++) {
    if (!diff[b]) continue;
    left--;
    uint32_t* out = bufs[left & 1];
    hipLaunchKernelGGL(anon_count_kernel, dim3(wk.tiles), dim3(kAnonWg), 0, st, keys, in, n, b, wk.tiles, hist);
    scan_u32(st, hist, 256 * wk.tiles, 0, 0, start, static_cast<uint32_t*>(wk.block_sums.p), diff_dev + 8, nullptr);
    hipLaunchKernelGGL(anon_scatter_kernel, dim3(wk.tiles), dim3(kAnonWg), 0, st, keys, in, n, b, wk.tiles, start, out);
    in = out;
  }
  return passes;
}

// res (3 x u64 on the device) <- the adjacent compare over d_perm, enqueued on st
inline void anon_set_adjacent(hipStream_t st, const void* d_keys, const uint32_t* d_perm, uint64_t n, void* d_res) {
  ZK_HIP(hipMemsetAsync(d_res, 0, 24, st));
  ZK_HIP(hipMemsetAsync(static_cast<char*>(d_res) + 8, 0xff, 8, st));
  if (n == 0) return;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>(2048, (n + kAnonWg - 1) / kAnonWg);
  hipLaunchKernelGGL(anon_adjacent_kernel, dim3(blocks), dim3(kAnonWg), 0, st, static_cast<const uint4*>(d_keys), d_perm, n,
                     static_cast<unsigned long long*>(d_res));
}

// d_first, d_count (m words each) <- the equal run of each of the m queries in the index d_perm of the n keys, enqueued
// on st. n = 0: every count is 0 and neither keys nor perm is read.
inline void anon_set_find(hipStream_t st, const void* d_keys, uint64_t n, const uint32_t* d_perm, const void* d_queries,
                          uint64_t m, uint32_t* d_first, uint32_t* d_count) {
  if (m == 0) return;
  if (n >> 32 || m >> 32) throw HipError("anon set: at most 2^32 - 1 rows and queries");
  hipLaunchKernelGGL(anon_find_kernel, dim3((uint32_t)((m + kAnonWg - 1) / kAnonWg)), dim3(kAnonWg), 0, st,
                     static_cast<const uint4*>(d_keys), n, d_perm, static_cast<const uint4*>(d_queries), m, d_first, d_count);
}

}  // namespace zkpoa
