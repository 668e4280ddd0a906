// Internal C++ view of the opaque handles declared in include/zkpoa_prover.h.
#pragma once
#include "../../include/zkpoa_prover.h"
#include "device_ctx.hpp"
#include "fast_upload.hpp"
#include "host_curve.hpp"
#include "msm_plan.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <string>
#include <vector>

namespace zkpoa {
struct NttEngine;
struct MsmTable;    // msm.hip.h: fixed-base table 2^(c*j) * P_i of one base array
struct MsmSorted;   // msm.hip.h: the result of an MSM's sort phase
void msm_table_release(MsmTable* t);   // delete, where the type is complete (msm_g1.hip)
struct MsmTableFree {
  void operator()(MsmTable* t) const { msm_table_release(t); }
};
typedef std::unique_ptr<MsmTable, MsmTableFree> MsmTablePtr;
}

struct zkpoa_poseidon_state;   // poseidon.hip: device copy of the Poseidon parameters

namespace zkpoa {
// The slots of zkpoa_context::ms: the ids of zkpoa_last_ms, 0 to 10 in this order. The ids are ABI and do not move, and
// include/zkpoa_prover.h says what each holds: a new slot goes before kMsCount, and into that comment.
enum MsSlot : int {
  kMsMsm, kMsMsmAccum, kMsNtt, kMsChain, kMsMsmPhase, kMsProve, kMsSelfCheck, kMsMerkleBuild, kMsLaneBatch, kMsAnonIndex,
  kMsAnonFind, kMsCount
};
// an MSM fills {whole, accumulation} through one `float* ms2` (msm_run.hip.h), which for the context is `ms` itself
static_assert(kMsMsm == 0 && kMsMsmAccum == 1, "msm_run's ms2 = ctx->ms needs the two MSM slots first and adjacent");
}  // namespace zkpoa

// Teardown (~zkpoa_context, zkpoa_api.hip): the device is drained and the background thread joined -- it may still be
// inside uploader.add_streams --, the NTT and Poseidon state go, then the members in reverse order of declaration: the
// events, the uploader (its own streams, events and pinned block), and last `dev` (the lanes and the copy stream).
struct zkpoa_context {
  zkpoa_context() = default;
  ~zkpoa_context();
  zkpoa_context(const zkpoa_context&) = delete;
  zkpoa_context& operator=(const zkpoa_context&) = delete;
  zkpoa::DeviceCtx dev;
  zkpoa_poseidon_state* poseidon = nullptr;
  zkpoa::NttEngine* ntt = nullptr;
  zkpoa::FastUploader uploader;   // pinned, multi-threaded host -> HBM path for zkey sections / witnesses
  std::string last_error;
  float ms[zkpoa::kMsCount] = {};   // zkpoa_last_ms, by MsSlot
  float io_ms[2] = {0, 0};   // last prove from a host buffer: [0] witness -> HBM (host clock), [1] its bytes / 1e6
  float lane_ms[zkpoa::DeviceCtx::kLanes][2] = {};   // per-lane {whole MSM, accumulation kernel} of the last MSM
  double lane_adds[zkpoa::DeviceCtx::kLanes] = {};   // per-lane mixed additions of that kernel (non-zero digits)
  int opt_msm_c = 0;    // forced window width; 0 (or out of range) = the cost model
  int opt_msm_k0 = 0;   // experiments: forced level-0 piece length; 0 (or out of range) = the rule (msm_plan.hpp)
  long opt_msm_max_points = 0;   // 0 = default (2^27): larger MSMs run in chunks
  long opt_ptau_piece_points = 0;   // powersoftau contribute / beacon: points per piece; 0 = derived from free HBM
  long opt_ptau_mul_slab = 0;       // scalar_mul_each: points per launch; 0 = 2^20 (tests: cross a slab border at a small size)
  long opt_state_proof_slab = 0;    // zkpoa_mpt_verify and its kin: items per slab; 0 = 2^20 (tests: the same)
  // Set when a lane's workspace for a whole MSM did not fit in HBM (found out by a failed reservation: msm_run, or
  // ahead of a proof: prover.hip budget_lane_workspaces): from then on the MSMs of that lane take at most this many
  // points at a time (never below 2^16); 0 = no limit of this kind.
  std::atomic<uint64_t> oom_max_points[zkpoa::DeviceCtx::kLanes] = {};
  uint64_t msm_points_limit(int lane) const {
    uint64_t lim = opt_msm_max_points ? (uint64_t)opt_msm_max_points : (1ull << 27);
    const uint64_t o = oom_max_points[lane].load();
    return o && o < lim ? o : lim;
  }
  uint64_t msm_points_limit_min() const {
    uint64_t lim = msm_points_limit(0);
    for (int l = 1; l < zkpoa::DeviceCtx::kLanes; l++) lim = std::min(lim, msm_points_limit(l));
    return lim;
  }
  static uint64_t below(uint64_t points) {   // the largest power of two below `points`, at least 2^16
    uint64_t want = 1ull << 16;
    while (want * 2 < points) want *= 2;
    return want;
  }
  // called with the size that failed; false when there is nothing smaller to try
  bool shrink_after_oom(int lane, uint64_t failed_points) {
    if (failed_points <= (1ull << 16)) return false;
    const uint64_t want = below(failed_points);
    uint64_t cur = oom_max_points[lane].load();
    while ((cur == 0 || cur > want) && !oom_max_points[lane].compare_exchange_weak(cur, want)) {
    }
    return true;
  }
  // HBM the key of a staged one-shot prove has still to allocate (prover.hip load_prove_staged); the lanes' arenas read it
  std::atomic<int64_t> key_hold_back{0};
  int opt_prove_serial = 0;      // measurement: run the stages of a prove one at a time (solo device times)
  // split chain: the witness copy of zkpoa_split_stage1 is enqueued on lane 0; the other lanes' MSMs wait for it
  zkpoa::DevEvent ev_witness;   // created by the first caller of record_witness_event
  bool ev_witness_set = false;
  // (the start / stop pair of every lane is the lane's: Lane::ev_a, ev_b)
  // the H chain's own pair: a prove reads it after the H MSM, which has recorded lane 0's pair again by then
  zkpoa::DevEvent ev_chain_a, ev_chain_b;
  // "the witness is in place up to here on st": the MSMs of the other lanes wait for it (prove_partials)
  void record_witness_event(hipStream_t st) {
    if (!ev_witness) ev_witness.create(hipEventDisableTiming);
    ZK_HIP(hipEventRecord(ev_witness, st));
    ev_witness_set = true;
  }
};

struct zkpoa_msm_table {   // C-ABI handle of a fixed-base table (zkpoa_msm_table_build)
  zkpoa::MsmTablePtr t;
  int group = 1;
};

namespace zkpoa {
void set_err(char* buf, unsigned long cap, const std::string& msg);

// host-clock milliseconds since t0 (the phase times of ZKPOA_VERBOSE and of zkpoa_context::ms / io_ms)
inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// hipFree waits for the whole device, copies in flight included. While a one-shot prove overlaps the key upload with
// compute, temporaries are therefore parked in the calling thread's sink and freed after the proof.
inline std::vector<void*>*& deferred_free_sink() {
  static thread_local std::vector<void*>* sink = nullptr;
  return sink;
}
inline void free_deferred(std::vector<void*>& sink) {   // once the device has drained
  for (void* p : sink) (void)hipFree(p);
  sink.clear();
}

// (DevMem, the owning handle of whatever outlives a call, is in device_handles.hpp: it never lands in a sink by being
// destroyed.)
struct DevBuf {  // a call's temporary device allocation: parked in the thread's deferred_free_sink() when one is set
  void* p = nullptr;
  explicit DevBuf(size_t bytes) { ZK_HIP(hipMalloc(&p, bytes ? bytes : 1)); }
  ~DevBuf() {
    if (!p) return;
    if (deferred_free_sink()) deferred_free_sink()->push_back(p);
    else (void)hipFree(p);
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  void up(const void* src, size_t bytes, size_t at = 0) {   // blocking host -> device copy to byte `at`
    if (bytes) ZK_HIP(hipMemcpy(static_cast<char*>(p) + at, src, bytes, hipMemcpyHostToDevice));
  }
};

// ---- the shape of a one-shot entry point ------------------------------------------------------------------------------
// The caller's arrays onto the device (LaneIn; LaneOut for results), the launches on lane 0's stream over
// blocks_of(n, threads) workgroups -- inside timed() when the call reports its kernel time --, finish(), down().
// Large pageable inputs go through ctx->uploader into a DevBuf instead: LaneIn is the plain blocking copy.
inline uint32_t blocks_of(uint64_t lanes, uint32_t threads) { return (uint32_t)((lanes + threads - 1) / threads); }

inline void finish(hipStream_t st) {
  ZK_HIP(hipStreamSynchronize(st));
  ZK_HIP(hipGetLastError());
}

// One array of a call on the device: n items of `each` bytes, which is said here and nowhere else. Buf is DevBuf, or
// lane_batch.hip.h's SecretBuf (with its stream as the last argument) for keys and nonces.
template <class Buf>
struct LaneArray {
  Buf buf;
  size_t each;
  uint64_t n;
  template <class... A>
  LaneArray(size_t each_, uint64_t n_, A... a) : buf(each_ * n_, a...), each(each_), n(n_) {}
  template <class T>
  T* at(uint64_t i0) const {   // item i0, where a launch over the items from i0 on begins
    return reinterpret_cast<T*>(static_cast<char*>(buf.p) + each * i0);
  }
};
// uploaded from the caller's array. An operand the call does not use is given n = 0: nothing is read from `host`,
// which may then be null, and at(0) is still a pointer into device memory.
template <class Buf = DevBuf>
struct LaneIn : LaneArray<Buf> {
  template <class... A>
  LaneIn(const void* host, size_t each_, uint64_t n_, A... a) : LaneArray<Buf>(each_, n_, a...) {
    this->buf.up(host, each_ * n_);
  }
};
template <class Buf = DevBuf>
struct LaneOut : LaneArray<Buf> {   // down() copies it into the caller's array
  void* host;
  template <class... A>
  LaneOut(void* host_, size_t each_, uint64_t n_, A... a) : LaneArray<Buf>(each_, n_, a...), host(host_) {}
  void down() const { ZK_HIP(hipMemcpy(host, this->buf.p, this->each * this->n, hipMemcpyDeviceToHost)); }
};
template <class Buf = DevBuf>
struct LaneInOut : LaneOut<Buf> {   // transformed in place: uploaded from the caller's array, and down() copies it back
  template <class... A>
  LaneInOut(void* host_, size_t each_, uint64_t n_, A... a) : LaneOut<Buf>(host_, each_, n_, a...) {
    this->buf.up(host_, each_ * n_);
  }
};

// launch(i0, m) for the items i0 .. i0 + m - 1, at most `slab` of them at a time
template <class Fn>
void for_slabs(uint64_t n, uint64_t slab, Fn launch) {
  for (uint64_t i0 = 0; i0 < n; i0 += slab) launch(i0, std::min(slab, n - i0));
}

// The kernel time of a call, into a slot of zkpoa_context::ms: start(), the launches, stop(), then read(), which waits
// for the stream, checks the last error and sets the slot (add: adds to what it holds). Only what lies between start()
// and stop() is timed; more may be enqueued between stop() and read(). A call that can return before its launches sets
// its slot to 0 first. One timer per event pair at a time.
struct KernelTimer {
  zkpoa_context* ctx;
  hipStream_t st;
  hipEvent_t a, b;
  static KernelTimer lane0(zkpoa_context* ctx, hipStream_t st) { return {ctx, st, ctx->dev.lanes[0].ev_a, ctx->dev.lanes[0].ev_b}; }
  static KernelTimer chain(zkpoa_context* ctx, hipStream_t st) { return {ctx, st, ctx->ev_chain_a, ctx->ev_chain_b}; }
  void start() { ZK_HIP(hipEventRecord(a, st)); }
  void stop() { ZK_HIP(hipEventRecord(b, st)); }
  // read() without the wait and the check, for a caller that has waited for later work of the stream by other means
  void store(MsSlot slot, bool add = false) {
    float ms = 0;
    ZK_HIP(hipEventElapsedTime(&ms, a, b));
    ctx->ms[slot] = add ? ctx->ms[slot] + ms : ms;
  }
  void read(MsSlot slot, bool add = false) {
    finish(st);
    store(slot, add);
  }
};
// the common case: nothing between the launches and the wait
template <class Fn>
void timed(zkpoa_context* ctx, hipStream_t st, MsSlot slot, Fn launches, bool add = false) {
  KernelTimer t = KernelTimer::lane0(ctx, st);
  t.start();
  launches();
  t.stop();
  t.read(slot, add);
}


// per-group entry points, each compiled in its own translation unit (msm_g1.hip, msm_g2.hip, ...)
// The request (msm_plan.hpp) of an MSM of this context over n points at once: the context's options, and the window
// width of the fixed-base table the MSM runs through (table_c > 0: merged form) -- else the forced width, else the model's.
// density: that of the scalars (msm_density), nullptr = uniform. for_g2: the sort feeds a G2 accumulation.
inline MsmRequest msm_request(const zkpoa_context* ctx, uint64_t n, int table_c, bool for_g2, const double* density) {
  return MsmRequest{n, table_c > 0 ? table_c : ctx->opt_msm_c, table_c > 0, for_g2, density, ctx->opt_msm_k0};
}
// One MSM, in chunks of at most the lane's point limit; a chunked MSM gives up `table`. density: of these scalars.
void msm_run_g1(zkpoa_context* ctx, int lane_id, const void* d_bases, const void* d_scalars, uint64_t n, uint8_t* out,
                float* ms2, const MsmTable* table = nullptr, const double* density = nullptr);
void msm_run_g2(zkpoa_context* ctx, int lane_id, const void* d_bases, const void* d_scalars, uint64_t n, uint8_t* out,
                float* ms2, const MsmTable* table = nullptr, const double* density = nullptr);
// tables: built on lane 0's stream (synchronised on return); c = 0 picks the width from the cost model (uniform scalars)
MsmTablePtr msm_table_build_g1(zkpoa_context* ctx, const void* d_bases, uint64_t n, int c);
MsmTablePtr msm_table_build_g2(zkpoa_context* ctx, const void* d_bases, uint64_t n, int c);
size_t msm_table_bytes_g1(uint64_t n, int c);
size_t msm_table_bytes_g2(uint64_t n, int c);
const void* msm_table_data(const MsmTable* t);
void msm_table_info(const MsmTable* t, uint64_t out[4]);   // n, c, W, bytes
// bytes of lane workspace the named parts of the request's plan reserve (msm.hip.h msm_sort/accum_workspace_bytes):
// a whole MSM is its sort and one accumulation in the same arena; an accumulation over another lane's sort is that alone.
enum MsmPart : unsigned { kMsmSort = 1, kMsmAccumG1 = 2, kMsmAccumG2 = 4 };
// guard: sized for the arena's guard mode (ZKPOA_WS_GUARD; the caller reads the option, this function does not).
size_t msm_workspace(const MsmRequest& req, unsigned parts, bool guard);   // 0 for req.n == 0
// non-zero digits per scalar for every window width (index c, 4..25) of n scalars on the device; synchronises st
// (d_scratch: 256 B of device memory of the caller's -- no allocation here: a hipFree would wait for every lane)
void msm_density(hipStream_t st, const void* d_scalars, uint64_t n, double out[32], void* d_scratch);
void group_add_run_g1(zkpoa_context* ctx, const void* a, const void* b, void* out, uint64_t n);
void group_add_run_g2(zkpoa_context* ctx, const void* a, const void* b, void* out, uint64_t n);
// zkpoa_field_prim / zkpoa_curve_prim (hooks.hip.h): an unknown op throws, also for n == 0
void field_prim_run_g1(zkpoa_context* ctx, int field, int op, const void* in, void* out, uint64_t n, int raw);
void field_prim_run_g2(zkpoa_context* ctx, int op, const void* in, void* out, uint64_t n, int raw);
void curve_prim_run_g1(zkpoa_context* ctx, int op, const void* a, const void* b, const uint32_t* k, void* out,
                       uint64_t n);
void fq29_prim_run(zkpoa_context* ctx, int op, const void* in, void* out, uint64_t n, int raw);
void curve_prim_run_g2(zkpoa_context* ctx, int op, const void* a, const void* b, const uint32_t* k, void* out,
                       uint64_t n);
void gen_bases_g1(zkpoa_context* ctx, const uint8_t a_le[32], const uint8_t b_le[32], uint64_t i0, uint64_t n, void* d_out);
void gen_bases_g2(zkpoa_context* ctx, const uint8_t a_le[32], const uint8_t b_le[32], uint64_t i0, uint64_t n, void* d_out);
// shared-sort form (prover: the A, B1 and B2 queries use the same witness scalars): sort once on `lane`
// (stream synchronised on return), then accumulate each base array on its own lane.
// The sorting lane also accumulates a G1 array afterwards (room for that is reserved in the same arena). The owner
// keeps the result alive until every accumulation over it has returned. (std::default_delete needs the complete type:
// only a translation unit that includes msm.hip.h can own one.)
std::unique_ptr<MsmSorted> msm_sort_run(zkpoa_context* ctx, int lane_id, const void* d_scalars, const MsmRequest& req);
void msm_accum_g1(zkpoa_context* ctx, int lane_id, const MsmSorted* sr, bool own_arena, const void* d_bases,
                  uint8_t* out, float* ms2);
void msm_accum_g2(zkpoa_context* ctx, int lane_id, const MsmSorted* sr, bool own_arena, const void* d_bases,
                  uint8_t* out, float* ms2);
// ec_ntt_g1.hip / ec_ntt_g2.hip (ec_ntt.hip.h): the inverse NTT over curve points. The work of transforms of up to
// 2^log_max points: the XYZZ buffer and the twiddles; one transform at a time uses it.
struct EcNttWork {
  uint32_t log_max;
  DevBuf work, tw;
  EcNttWork(uint32_t lm, size_t work_bytes, size_t tw_bytes) : log_max(lm), work(work_bytes), tw(tw_bytes) {}
};
inline size_t ec_intt_work_bytes(int group, uint32_t log_max) {   // device memory of an EcNttWork
  return ((size_t)(group == 2 ? 256 : 128) << log_max) + (log_max ? (size_t)32 << (log_max - 1) : 32);
}
EcNttWork* ec_intt_work_g1(zkpoa_context* ctx, uint32_t log_max);   // delete when done; twiddles built on lane 0's stream
EcNttWork* ec_intt_work_g2(zkpoa_context* ctx, uint32_t log_max);
// enqueued on lane 0's stream: d_out[j] = sum_i (w_n^(-ij) / n) d_in[i], n = 2^log_n <= 2^log_max; d_out may be d_in
void ec_intt_g1(zkpoa_context* ctx, EcNttWork& wk, const void* d_in, uint32_t log_n, void* d_out);
void ec_intt_g2(zkpoa_context* ctx, EcNttWork& wk, const void* d_in, uint32_t log_n, void* d_out);
// ptau_mul_g1.hip / ptau_mul_g2.hip (ptau_contribute.hip.h): d_out[i] = k_i * P_i enqueued on lane 0's stream (not
// synchronised), wire form in and out, scalars standard form; flags: one zeroed device word, |= 1 for a scalar >= r.
// n < 2^32. d_scratch: scalar_mul_each_scratch_gX(n, slab) bytes of the caller's; slab = points per launch, 0 = 2^20.
size_t scalar_mul_each_scratch_g1(uint64_t n, uint64_t slab);
size_t scalar_mul_each_scratch_g2(uint64_t n, uint64_t slab);
void scalar_mul_each_g1(zkpoa_context* ctx, const void* d_points, const void* d_scalars, uint64_t n, void* d_out, uint32_t* d_flags,
                        void* d_scratch, uint64_t slab);
void scalar_mul_each_g2(zkpoa_context* ctx, const void* d_points, const void* d_scalars, uint64_t n, void* d_out, uint32_t* d_flags,
                        void* d_scratch, uint64_t slab);
// the two by group (1: G1, 2: G2): the one place that branches
inline size_t scalar_mul_each_scratch(int group, uint64_t n, uint64_t slab) {
  return group == 2 ? scalar_mul_each_scratch_g2(n, slab) : scalar_mul_each_scratch_g1(n, slab);
}
inline void scalar_mul_each(zkpoa_context* ctx, int group, const void* d_points, const void* d_scalars, uint64_t n, void* d_out,
                            uint32_t* d_flags, void* d_scratch, uint64_t slab) {
  if (group == 2) scalar_mul_each_g2(ctx, d_points, d_scalars, n, d_out, d_flags, d_scratch, slab);
  else scalar_mul_each_g1(ctx, d_points, d_scalars, n, d_out, d_flags, d_scratch, slab);
}
// ptau_response.hip: hash form (compressed: compressed form) -> wire form on lane 0's stream. convert() enqueues n points
// of group 1 / 2 from d_bytes into d_out (n x 64 / 128 B); a point that cannot be converted leaves its index and what is
// wrong with it in `first` (the smallest index of all convert() calls since the last require()). require() synchronises
// the stream and throws "<what>: point <i0 + index>: <why>" for it.
struct FormConverter {
  zkpoa_context* ctx;
  DevBuf first;
  explicit FormConverter(zkpoa_context* c);
  void convert(bool compressed, int group, const void* d_bytes, uint64_t n, void* d_out);
  void require(uint64_t i0, const char* what);
};
// ntt.hip
// the first use of a size builds its plan and every table (hipMalloc, kernels on st); later calls find it ready
void ntt_prepare(zkpoa_context* ctx, hipStream_t st, uint32_t k);
// batch > 1: that many vectors of 2^k elements, `stride` bytes apart, transformed together (one launch per pass)
void ntt_to_odd_coset(zkpoa_context* ctx, hipStream_t st, void* d_data, uint32_t k, uint32_t batch = 1, size_t stride = 0);
void ntt_natural(zkpoa_context* ctx, hipStream_t st, void* d_data, uint32_t k, bool inverse);
// unscaled, unpermuted halves of a transform: DIF natural -> bit-reversed, DIT bit-reversed -> natural
void ntt_dif(zkpoa_context* ctx, hipStream_t st, void* d_data, uint32_t k, bool inverse, uint32_t batch = 1, size_t stride = 0);
void ntt_dit(zkpoa_context* ctx, hipStream_t st, void* d_data, uint32_t k, bool inverse, uint32_t batch = 1, size_t stride = 0);
// H-scalar chain split over G ranks: the step between the two exchanges (ntt.hip.h, ntt_split_mid_kernel)
void ntt_split_mid(zkpoa_context* ctx, hipStream_t st, const void* in, void* out, uint32_t k, uint32_t G, uint32_t h,
                   uint32_t rank_stride);
void ntt_release(zkpoa_context* ctx);
void poseidon_release(zkpoa_context* ctx);
// anon_set.hip: host queries (m x 32 B) looked up among n keys on the device through their stable index, which is built
// into `perm` first when that is still empty; first, count: host, m words. ms[kMsAnonFind] <- the kernels' time.
void anon_set_find_indexed(zkpoa_context* ctx, const void* d_keys, uint64_t n, DevMem& perm, const void* queries, uint64_t m,
                           uint32_t* first, uint32_t* count);
}  // namespace zkpoa

#define ZK_API_BEGIN(ctx)  \
  if (!(ctx)) return PROVER_ERROR; \
  try {                    \
    ZK_HIP(hipSetDevice((ctx)->dev.device));
#define ZK_API_END(ctx)                 \
  }                                     \
  catch (const std::exception& e) {     \
    (ctx)->last_error = e.what();       \
    return PROVER_ERROR;                \
  }                                     \
  return PROVER_OK;

