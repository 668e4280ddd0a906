// The run-time options of the library and its commands, in one place: every ZKPOA_* environment variable is one row of
// the table below (argv has to stay rapidsnark's, so the environment is all the configuration there is), and nothing
// else in csrc/ calls getenv for one. A row is addressed by its O_<NAME> constant: a misspelt name does not compile.
// Host only, libc and the standard library: the libc-only `prover` client and a plain g++ program include it too
// (tools/options_check.cpp lists the table and is how tests/test_options_host.py checks every row; INTEGRATION.md
// carries the same table for the user).
//
// What a value means, by the row's kind:
//   flag    unset or empty = the row's default; "0" = off; anything else = on
//   int     whole string, base 10, errno checked, within [lo, hi]; unset or empty = the default
//   choice  one of the row's words -> its index in the list; unset or empty = the default
//   text    the string as it is, or null when unset; the site has its own parser (a list, a 256-bit number)
// A value that is none of that is an input error under a strict row (OptionError: the message names the variable, the
// value and the range) and gives the default under a lenient one. A latched row is read at its first use in the
// process and keeps that value (a latched text row: its site keeps what it parsed); the others are read at every use
// (tests change them between calls).
#pragma once
#include <assert.h>
#include <errno.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <stdexcept>
#include <string>

namespace zkpoa {

enum OptKind { kOptFlag, kOptInt, kOptChoice, kOptText };
enum OptBad { kLenient, kStrict };     // (a text row: what its site's own parser does with a malformed value)
enum OptWhen { kEveryUse, kLatched };
enum OptUse { kKnob, kHook };          // a hook serves tests, experiments and measurements only

//  X(NAME, kind, lo, hi, words, default, bad value, read, use, own message of a strict row or null, meaning)
#define ZKPOA_OPTION_TABLE(X)                                                                                                              \
  X(VERBOSE, kOptFlag, 0, 1, nullptr, 0, kLenient, kEveryUse, kKnob, nullptr, "phase timings on stderr (per request in a resident server)") \
  X(R, kOptText, 0, 0, nullptr, 0, kStrict, kEveryUse, kHook, nullptr, "decimal: fixes the blinding scalar r; a warning is printed, such proofs are not zero-knowledge") \
  X(S, kOptText, 0, 0, nullptr, 0, kStrict, kEveryUse, kHook, nullptr, "decimal: fixes the blinding scalar s, as ZKPOA_R")               \
  X(JSON, kOptChoice, 0, 0, "rapidsnark|snarkjs", 0, kLenient, kEveryUse, kKnob, nullptr, "byte style of proof.json and public.json") \
  X(DEVICE, kOptInt, 0, 1023, nullptr, 0, kStrict, kEveryUse, kKnob, "ZKPOA_DEVICE: not a device index: %s", "the one HIP device to use (the prover also checks it against the device count)") \
  X(DEVICES, kOptText, 0, 0, nullptr, 0, kStrict, kEveryUse, kKnob, nullptr, "comma-separated HIP devices, one rank each (1 to 8), or auto") \
  X(MULTI_MIN_POWER, kOptInt, 0, 64, nullptr, 24, kStrict, kEveryUse, kKnob, nullptr, "automatic device choice: a key with a domain of 2^this or more takes every free GPU") \
  X(SHARD_BLOCK_LOG, kOptInt, 0, 24, nullptr, -1, kStrict, kEveryUse, kKnob, nullptr, "log2 of the block-cyclic shard block: 0 = contiguous ranges, 4 to 24; -1 = by key size") \
  X(GPU_LOCK_WAIT_S, kOptInt, 0, 86400, nullptr, 1800, kStrict, kEveryUse, kKnob, nullptr, "seconds to wait for a busy GPU's lock file before sharing the GPU") \
  X(LANE_WORKSPACE_MAX_MB, kOptInt, 0, 1l << 20, nullptr, 0, kStrict, kEveryUse, kKnob, "ZKPOA_LANE_WORKSPACE_MAX_MB='%s' is not a number of MiB", "cap of each MSM lane's workspace in MiB; 0 = whatever HBM holds") \
  X(SELFCHECK, kOptChoice, 0, 0, "1|0|off|all|2", 0, kLenient, kEveryUse, kKnob, nullptr, "pairing check before a proof is written: 1 = a key's first proof, 0 / off = never, all / 2 = every proof") \
  X(PRECOMP, kOptChoice, 0, 0, "idle|0|off|eager", 0, kLenient, kEveryUse, kKnob, nullptr, "when a resident key gets its fixed-base tables: from idle time, never, or at its second use") \
  X(PRECOMP_AFTER, kOptInt, 1, 1000000000, nullptr, 64, kLenient, kEveryUse, kKnob, nullptr, "PRECOMP=idle: proofs after which a key gets its tables inside a request all the same") \
  X(KEY_CACHE, kOptInt, 0, 1000000, nullptr, 2, kLenient, kEveryUse, kKnob, nullptr, "proving keys kept resident by the file entry points; 0 = none") \
  X(OVERLAP, kOptFlag, 0, 1, nullptr, 1, kLenient, kEveryUse, kKnob, nullptr, "one-shot prove: overlap the key upload with the compute") \
  X(DETACH_EXIT, kOptChoice, 0, 0, "auto|0|always", 0, kLenient, kEveryUse, kKnob, nullptr, "worker process for a command that holds tens of GB: by size, never, always (tests)") \
  X(UPLOAD_THREADS, kOptInt, 1, 16, nullptr, 8, kLenient, kEveryUse, kKnob, nullptr, "host threads of the staged upload")                \
  X(UPLOAD_STREAMS, kOptInt, 0, 8, nullptr, -1, kLenient, kEveryUse, kKnob, nullptr, "the uploader's own streams; -1 = 1, or 3 when GPU_MAX_HW_QUEUES >= 8") \
  X(UPLOAD_AFFINITY, kOptChoice, 0, 0, "gpu|off", 0, kLenient, kEveryUse, kKnob, nullptr, "keep the staging threads on the GPU's NUMA node, or wherever the scheduler puts them") \
  X(UPLOAD_STREAM_PRIO, kOptChoice, 0, 0, "high|normal|low", 0, kLenient, kEveryUse, kHook, nullptr, "priority of the uploader's own streams (measurement)") \
  X(LANE_PRIO, kOptChoice, 0, 0, "ladder|flat|none|ladder2|top1", 0, kLenient, kEveryUse, kHook, nullptr, "stream priority pattern of the MSM lanes (measurement)") \
  X(WITNESS_TABLE_C, kOptInt, 4, 25, nullptr, 0, kLenient, kEveryUse, kHook, nullptr, "window width of the A / B / C fixed-base tables; 0 = by the cost model (experiments)") \
  X(NO_DENSITY, kOptFlag, 0, 1, nullptr, 0, kLenient, kEveryUse, kHook, nullptr, "plan the witness MSMs without the measured digit density (measurement)") \
  X(NO_SPARSE, kOptFlag, 0, 1, nullptr, 0, kLenient, kLatched, kHook, nullptr, "keep the dense entry form of the MSM sort (measurement)") \
  X(SCAN, kOptChoice, 0, 0, "1|3", 0, kLenient, kLatched, kHook, nullptr, "the MSM lane's scans in one launch or in three (measurement)") \
  X(NTT_TILE, kOptInt, 10, 11, nullptr, 0, kLenient, kLatched, kHook, nullptr, "log2 of the NTT tile; 0 = by transform size (measurement, tests)") \
  X(EXCHANGE, kOptChoice, 0, 0, "peer|copy", 0, kLenient, kLatched, kKnob, nullptr, "multi-GPU exchanges: peer-to-peer stores, or hipMemcpyPeerAsync") \
  X(SETUP_THREADS, kOptInt, 1, 256, nullptr, 0, kLenient, kEveryUse, kKnob, nullptr, "host threads of the setup commands (at most 32 are used); 0 = the host's") \
  X(MERKLE_THREADS, kOptInt, 1, 256, nullptr, 0, kStrict, kEveryUse, kKnob, "ZKPOA_MERKLE_THREADS must be 1..256, not '%s'", "host threads reading merkle-tree's anonymity set; 0 = the host's, at most 16") \
  X(STRICT, kOptFlag, 0, 1, nullptr, 0, kLenient, kEveryUse, kKnob, nullptr, "prover: exit 5 instead of proving in-process after the resident server failed") \
  X(SERVER, kOptText, 0, 0, nullptr, 0, kLenient, kEveryUse, kKnob, nullptr, "prover: 1 or /path/to.sock = hand the proof to a resident server; unset, empty or 0 = off") \
  X(SERVER_IDLE_S, kOptInt, 1, 1000000000, nullptr, 600, kLenient, kEveryUse, kKnob, nullptr, "the server exits after this many seconds without work") \
  X(SERVER_IDLE_WORK_MS, kOptInt, 0, 1000000000, nullptr, 300, kLenient, kEveryUse, kKnob, nullptr, "the server starts the library's idle work after this many ms without a request") \
  X(SERVER_WORKERS, kOptInt, 1, 8, nullptr, 2, kLenient, kEveryUse, kKnob, nullptr, "threads serving the server's requests")            \
  X(SERVER_RCV_TIMEOUT_S, kOptInt, 1, 1000000000, nullptr, 10, kLenient, kEveryUse, kKnob, nullptr, "the server drops a client that says nothing for this many seconds") \
  X(SERVER_TIMEOUT_S, kOptInt, 1, 1000000000, nullptr, 1800, kLenient, kEveryUse, kKnob, nullptr, "a client waits this many seconds for the server's answer") \
  X(SERVER_KILL_WEDGED, kOptFlag, 0, 1, nullptr, 0, kLenient, kEveryUse, kKnob, nullptr, "a client that timed out ends the server it was talking to") \
  X(SERVER_TEST_CRASH, kOptFlag, 0, 1, nullptr, 0, kLenient, kLatched, kHook, nullptr, "tests: the server dies with a request in hand")  \
  X(TEST_STALE_EXCHANGE, kOptInt, 0, 1000000000, nullptr, 0, kLenient, kLatched, kHook, nullptr, "tests: rank 0 withholds its first exchange in the n-th multi-rank proof") \
  X(TEST_FAIL_RANK, kOptText, 0, 0, nullptr, 0, kLenient, kLatched, kHook, nullptr, "tests: g[:phase], rank g fails at the start of that phase") \
  X(WS_GUARD, kOptFlag, 0, 1, nullptr, 0, kLenient, kEveryUse, kHook, nullptr, "tests: guard bytes behind every region of an MSM lane's workspace, checked when each phase ends") \
  X(TEST_WS_CLOBBER, kOptInt, 0, 1000000000, nullptr, 0, kLenient, kEveryUse, kHook, nullptr, "tests: under WS_GUARD the host overwrites one byte of the arena's k-th guard before a check; 0 = off") \
  X(DELTA, kOptText, 0, 0, nullptr, 0, kStrict, kEveryUse, kHook, nullptr, "zkpoa-setup zkey contribute: the secret delta, for reproducible keys") \
  X(PHASE1_S, kOptText, 0, 0, nullptr, 0, kStrict, kEveryUse, kHook, nullptr, "powersoftau contribute: s_tau,s_alpha,s_beta of the contribution record") \
  X(PHASE2_S, kOptText, 0, 0, nullptr, 0, kStrict, kEveryUse, kHook, nullptr, "zkey contribute: the s of the contribution record's g1_s")

enum Opt {
#define X(id, ...) O_##id,
  ZKPOA_OPTION_TABLE(X)
#undef X
  kOptCount
};

struct OptRow {
  const char* name;
  OptKind kind;
  long lo, hi;         // int
  const char* words;   // choice: "a|b|c"
  long dflt;           // flag: 0 / 1; int: the value (outside [lo, hi] where it stands for "automatic"); choice: an index
  OptBad bad;
  OptWhen when;
  OptUse use;
  const char* bad_fmt;   // a strict row that keeps a message of its own: one %s, the value
  const char* meaning;
};
inline const OptRow& opt_row(Opt id) {
  static const OptRow rows[kOptCount] = {
#define X(id, ...) {"ZKPOA_" #id, __VA_ARGS__},
      ZKPOA_OPTION_TABLE(X)
#undef X
  };
  return rows[id];
}

struct OptionError : std::runtime_error {   // a malformed value under a strict row: an input error
  using std::runtime_error::runtime_error;
};

// ---- per-request overlay -----------------------------------------------------------------------------------------------
// A resident server answers several clients from several threads and must not change its environment per request:
// zkpoa_set_thread_options gives the calling thread values of the four request rows that take precedence over the
// environment (an empty string = "unset for this thread even if the environment has it"). A SideTask inherits the
// overlay of the thread that starts it (host_threads.hpp), so every line of one proof follows its request.
struct OptOverlay {
  bool active = false;
  std::string r, s, json, verbose;
};
inline OptOverlay& opt_overlay() {
  static thread_local OptOverlay o;
  return o;
}

inline const char* opt_text(Opt id) {   // every read of a variable goes through here
  const OptOverlay& o = opt_overlay();
  if (o.active) {
    const std::string* v = id == O_R ? &o.r : id == O_S ? &o.s : id == O_JSON ? &o.json : id == O_VERBOSE ? &o.verbose : nullptr;
    if (v) return v->empty() ? nullptr : v->c_str();
  }
  return getenv(opt_row(id).name);
}

// the typed value of `e` under row id (an int within [lo, hi]); a text row is asked as a flag
inline long opt_parse(Opt id, const char* e, long lo, long hi, const char* bad_fmt) {
  const OptRow& r = opt_row(id);
  if (!e || !*e) return r.kind == kOptText ? 0 : r.dflt;
  if (r.kind == kOptFlag || r.kind == kOptText) return strcmp(e, "0") != 0;
  if (r.kind == kOptChoice) {
    const size_t len = strlen(e);
    long i = 0;
    for (const char* w = r.words; w && !strchr(e, '|'); w = strchr(w, '|') ? strchr(w, '|') + 1 : nullptr, i++)
      if (!strncmp(w, e, len) && (w[len] == '|' || !w[len])) return i;
  } else {
    char* end = nullptr;
    errno = 0;
    const long v = strtol(e, &end, 10);
    if (!errno && end != e && !*end && v >= lo && v <= hi) return v;
  }
  if (r.bad == kLenient) return r.dflt;
  if (bad_fmt) {
    std::string msg(strlen(bad_fmt) + strlen(e), '\0');
    msg.resize((size_t)snprintf(&msg[0], msg.size() + 1, bad_fmt, e));
    throw OptionError(msg);
  }
  throw OptionError(std::string(r.name) + "='" + e + "' is not " +
                    (r.kind == kOptInt ? "an integer in [" + std::to_string(lo) + ", " + std::to_string(hi) + "]" : std::string("one of ") + r.words));
}

inline long opt_value(Opt id, OptKind kind) {
  const OptRow& r = opt_row(id);
  assert(r.kind == kind || (kind == kOptFlag && r.kind == kOptText));
  (void)kind;
  if (r.when == kEveryUse) return opt_parse(id, opt_text(id), r.lo, r.hi, r.bad_fmt);
  struct Latch {
    std::once_flag once;
    long v;
  };
  static Latch latch[kOptCount];
  std::call_once(latch[id].once, [&] { latch[id].v = opt_parse(id, opt_text(id), r.lo, r.hi, r.bad_fmt); });
  return latch[id].v;
}

inline bool opt_flag(Opt id) { return opt_value(id, kOptFlag) != 0; }   // a flag row; a text row: set to something but "0"
inline long opt_long(Opt id) { return opt_value(id, kOptInt); }
inline int opt_choice(Opt id) { return (int)opt_value(id, kOptChoice); }   // index into the row's words
// an int row read at every use, held to a range the site learns at run time (a device index: below the device count);
// the message of a strict row then names that range
inline long opt_long(Opt id, long lo, long hi) { return opt_parse(id, opt_text(id), lo, hi, nullptr); }

// ---- the verbose log: one line of ZKPOA_VERBOSE output on stderr, the whole text given by the caller ---------------------
inline bool opt_verbose() { return opt_flag(O_VERBOSE); }
__attribute__((format(printf, 1, 2))) inline void vlog(const char* fmt, ...) {
  if (!opt_verbose()) return;
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
}

}  // namespace zkpoa
