// The prover's request layer: what every `prover` call and every server request runs between the three request entry
// points of the C ABI (groth16_prover, groth16_prover_zkey_file, zkpoa_groth16_prover_files: prover.hip) and the stages
// of a proof (prove_partials / load_prove_staged: prover.hip; multi_prove_partials: multi_device.hip.h):
// zkey + witness -> find or load a key -> prove -> self-check -> the two JSON texts.
// Included by prover.hip inside its anonymous namespace, after multi_device.hip.h: zkpoa_zkey and the lane types are
// private to that translation unit, and a second one would compile the MSM and NTT templates twice.
#pragma once

// ---- JSON (byte formats pinned by the reference's committed fixtures) --------
std::string fq_dec(const uint8_t* le_mont) { return HFq::from_bytes(le_mont).to_dec(); }
bool all_zero(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (p[i]) return false;
  return true;
}

std::string proof_json(const uint8_t pts[256], int style) {
  // coordinates as decimal strings
  std::string a[3], b[3][2], c[3];
  auto g1 = [&](const uint8_t* p, std::string out[3]) {
    if (all_zero(p, 64)) { out[0] = "0"; out[1] = "1"; out[2] = "0"; return; }
    out[0] = fq_dec(p); out[1] = fq_dec(p + 32); out[2] = "1";
  };
  g1(pts, a);
  g1(pts + 192, c);
  const uint8_t* pb = pts + 64;
  if (all_zero(pb, 128)) {
    b[0][0] = "0"; b[0][1] = "0"; b[1][0] = "1"; b[1][1] = "0"; b[2][0] = "0"; b[2][1] = "0";
  } else {
    b[0][0] = fq_dec(pb); b[0][1] = fq_dec(pb + 32); b[1][0] = fq_dec(pb + 64); b[1][1] = fq_dec(pb + 96);
    b[2][0] = "1"; b[2][1] = "0";
  }
  std::string o;
  auto q = [](const std::string& s) { return "\"" + s + "\""; };
  if (style == 0) {  // rapidsnark / nlohmann dump(): one line, no spaces
    o += "{\"pi_a\":[" + q(a[0]) + "," + q(a[1]) + "," + q(a[2]) + "],";
    o += "\"pi_b\":[[" + q(b[0][0]) + "," + q(b[0][1]) + "],[" + q(b[1][0]) + "," + q(b[1][1]) + "],[" + q(b[2][0]) +
         "," + q(b[2][1]) + "]],";
    o += "\"pi_c\":[" + q(c[0]) + "," + q(c[1]) + "," + q(c[2]) + "],";
    o += "\"protocol\":\"groth16\"}";
  } else {  // snarkjs: JSON.stringify(obj, null, 1)
    auto g1s = [&](const char* key, const std::string v[3]) {
      return std::string(" \"") + key + "\": [\n  " + q(v[0]) + ",\n  " + q(v[1]) + ",\n  " + q(v[2]) + "\n ],\n";
    };
    o += "{\n";
    o += g1s("pi_a", a);
    o += " \"pi_b\": [\n";
    for (int i = 0; i < 3; i++) {
      o += "  [\n   " + q(b[i][0]) + ",\n   " + q(b[i][1]) + "\n  ]";
      o += (i < 2) ? ",\n" : "\n";
    }
    o += " ],\n";
    o += g1s("pi_c", c);
    o += " \"protocol\": \"groth16\",\n \"curve\": \"bn128\"\n}";
  }
  return o;
}

std::string public_json(const uint8_t* pub, uint64_t n, int style) {
  std::string o;
  if (style == 0) {
    o = "[";
    for (uint64_t i = 0; i < n; i++) {
      HFr v = HFr::from_bytes(pub + 32 * i).to_mont();
      o += (i ? ",\"" : "\"") + v.to_dec() + "\"";
    }
    o += "]";
  } else {
    if (n == 0) return "[]";
    o = "[\n";
    for (uint64_t i = 0; i < n; i++) {
      HFr v = HFr::from_bytes(pub + 32 * i).to_mont();
      o += " \"" + v.to_dec() + "\"" + (i + 1 < n ? ",\n" : "\n");
    }
    o += "]";
  }
  return o;
}

int emit(const std::string& s, char* buffer, unsigned long* size) {
  if (!size) return PROVER_ERROR;
  unsigned long needed = (unsigned long)s.size() + 1;
  if (!buffer || *size < needed) {
    *size = needed;
    return PROVER_ERROR_SHORT_BUFFER;
  }
  memcpy(buffer, s.c_str(), needed);
  *size = needed;
  return PROVER_OK;
}

// ---- where a request's results go --------------------------------------------------------------------------------------
// The six output arguments of a request entry point, filled there and handed down by reference: nothing between the C
// ABI and the two operations below looks at them.
struct ProveOut {
  char* proof;
  unsigned long* proof_size;
  char* pub;
  unsigned long* public_size;
  char* err;
  unsigned long err_cap;
  // record a failure; returns `code`, so that a failing exit is one statement
  int fail(int code, const std::string& msg) const {
    set_err(err, err_cap, msg);
    return code;
  }
  // write both JSON texts, or report a short buffer (both sizes are set either way)
  int write(const std::string& proof_text, const std::string& public_text) const {
    const int r1 = emit(proof_text, proof, proof_size), r2 = emit(public_text, pub, public_size);
    return r1 == PROVER_OK && r2 == PROVER_OK ? PROVER_OK : fail(PROVER_ERROR_SHORT_BUFFER, "output buffer too small");
  }
};

// the code of a failure + its message; call inside a catch (...) block. *hip_failed <- it was a HIP runtime failure.
int classify_current_exception(const ProveOut& out, bool* hip_failed = nullptr) {
  try {
    throw;
  } catch (const ProverError& e) {
    return out.fail(e.code, e.what());
  } catch (const HipError& e) {            // HIP runtime failure: the context and its cached keys are suspect
    if (hip_failed) *hip_failed = true;
    return out.fail(PROVER_ERROR_RUNTIME, e.what());
  } catch (const std::bad_alloc&) {
    return out.fail(PROVER_ERROR_RUNTIME, "out of host memory");
  } catch (const std::system_error& e) {   // a stage thread could not be started
    return out.fail(PROVER_ERROR_RUNTIME, e.what());
  } catch (const std::exception& e) {
    return out.fail(PROVER_ERROR, e.what());
  }
}

std::mutex g_prove_mutex;   // one-shot entry points share the process-wide context: one proof at a time
// The file entry point is entered by several threads of a resident server. Two stages, two locks: g_stage_mutex covers
// the key cache and the upload of a request's witness into a free staging buffer of its key; g_prove_mutex the proof
// itself. A request whose key is resident and already has its tables stages its witness while the request before it
// is still proving -- at the layer-three size that is 31 ms of PCIe time per proof taken off the proof-to-proof period.
// Anything that changes the cache or a key (a load, the second-use table build, an eviction) waits until no staged
// request is pending and then holds both locks.
std::mutex g_stage_mutex;
std::condition_variable g_stage_cv;
int g_staged_users = 0;

// ---- from the partial sums to the output --------------------------------------------------------------------------------
// r, s from the environment (ZKPOA_R / ZKPOA_S, decimal; test use) -> pointers, or null for /dev/urandom
struct EnvBlinding {
  uint8_t rb[32], sb[32];
  const uint8_t *r = nullptr, *s = nullptr;
  EnvBlinding() {
    const char *er = opt_text(O_R), *es = opt_text(O_S);
    if (er || es) {
      static bool warned = false;
      if (!warned) {
        warned = true;
        fprintf(stderr, "zkpoa: WARNING: blinding scalars fixed by ZKPOA_R / ZKPOA_S (test use): proofs made this way are "
                        "not zero-knowledge; unset them in production\n");
      }
    }
    if (er) {
      if (!parse_decimal_mod_r(er, rb)) throw ProverError(PROVER_ERROR, "ZKPOA_R is not a decimal number");
      r = rb;
    }
    if (es) {
      if (!parse_decimal_mod_r(es, sb)) throw ProverError(PROVER_ERROR, "ZKPOA_S is not a decimal number");
      s = sb;
    }
  }
  EnvBlinding(const EnvBlinding&) = delete;
  EnvBlinding& operator=(const EnvBlinding&) = delete;
};

// proof points + public values -> the two JSON texts (ZKPOA_JSON style) + the ZKPOA_VERBOSE phase line
int emit_outputs(zkpoa_context* ctx, const zkpoa_zkey* zk, const uint8_t pts[256], const uint8_t* pub, const ProveOut& out,
                 double load_ms, uint64_t zkey_size, const char* how) {
  const int style = opt_choice(O_JSON);   // rapidsnark | snarkjs
  const int rc = out.write(proof_json(pts, style), public_json(pub, zk->nPublic, style));
  vlog("zkpoa: nVars=%u nPublic=%u domain=2^%u nCoefs=%llu | zkey %s %.1f ms (%.2f GB/s) | witness -> HBM %.2f ms "
       "(%.0f MB, %.1f GB/s) | h-chain %.2f ms, msm phase %.2f ms, prove %.2f ms, self-check %.2f ms\n",
       zk->nVars, zk->nPublic, zk->power, (unsigned long long)zk->nCoefs, how, load_ms,
       load_ms > 0 ? (double)zkey_size / load_ms / 1e6 : 0.0, ctx->io_ms[0], ctx->io_ms[1],
       ctx->io_ms[0] > 0 ? ctx->io_ms[1] / ctx->io_ms[0] : 0.0, ctx->ms[kMsChain], ctx->ms[kMsMsmPhase], ctx->ms[kMsProve], ctx->ms[kMsSelfCheck]);
  return rc;
}

// The tail every single-GPU path shares once it has its proof points: the public values from the witness view, the
// self-check of the key's first proof, the output. (The multi-GPU path has the same three steps around its repeat with
// copies: multi_prove_to_json.)
int check_and_emit(zkpoa_context* ctx, const zkpoa_zkey* zk, const uint8_t pts[256], const WtnsView& w, const ProveOut& out,
                   double load_ms, uint64_t zkey_size, const char* how) {
  std::vector<uint8_t> pub_store;
  const uint8_t* pubs = w.publics(zk->nPublic, pub_store);
  selfcheck(ctx, zk, pts, pubs);
  return emit_outputs(ctx, zk, pts, pubs, out, load_ms, zkey_size, how);
}

// prove with a resident key, JSON out; options from the environment (ZKPOA_R / ZKPOA_S / ZKPOA_JSON / ZKPOA_VERBOSE)
int prove_to_json(zkpoa_context* ctx, const zkpoa_zkey* zk, const WtnsSrc& wsrc, const ProveOut& out, double load_ms,
                  uint64_t zkey_size, bool cache_hit) {
  const EnvBlinding bl;
  WtnsView w = parse_wtns(wsrc);
  check_witness_len(w, zk);
  uint8_t pts[256];
  upload_and_prove(ctx, zk, w, bl.r, bl.s, pts);
  return check_and_emit(ctx, zk, pts, w, out, load_ms, zkey_size, cache_hit ? "cached," : "load");
}

// One-shot: load the key and prove, with the upload overlapped unless ZKPOA_OVERLAP=0. zk <- the loaded key, also when
// the proof fails after the load (the caller caches it or lets it go). The load time reported is the time to the end
// of the proof where load and prove are one phase.
int load_and_prove_to_json(zkpoa_context* ctx, const uint8_t* zkey, uint64_t zkey_size, const WtnsSrc& wsrc,
                           const ProveOut& out, KeyPtr& zk, int zkey_fd = -1) {
  const auto tl0 = std::chrono::steady_clock::now();
  if (opt_flag(O_OVERLAP)) {
    WtnsView w = parse_wtns(wsrc);
    const EnvBlinding bl;
    uint8_t parts[384], pts[256];
    const auto t0 = std::chrono::steady_clock::now();
    zk = load_prove_staged(ctx, zkey, zkey_size, w, parts, zkey_fd);
    if (zk) {
      assemble_proof(ctx, zk.get(), parts, bl.r, bl.s, t0, pts);
      return check_and_emit(ctx, zk.get(), pts, w, out, ctx->ms[kMsProve], zkey_size, "load overlapped with the prove:");
    }
  }
  zk = zkey_load_impl(ctx, zkey, zkey_size);
  return prove_to_json(ctx, zk.get(), wsrc, out, ms_since(tl0), zkey_size, false);
}

// witness -> proof JSON on a loaded MultiKey (the multi-GPU twin of prove_to_json)
int multi_prove_to_json(DeviceSet* ds, MultiKey* mk, const WtnsSrc& wsrc, const ProveOut& out, uint64_t zkey_size,
                        bool cache_hit) {
  zkpoa_zkey* z0 = mk->rank[0].shard.get();
  zkpoa_context* c0 = ds->ctx[0];
  WtnsView w = parse_wtns(wsrc);
  check_witness_len(w, z0);
  const EnvBlinding bl;
  uint8_t parts[384], pts[256];
  const auto t0 = std::chrono::steady_clock::now();
  multi_proof_counter()++;
  const bool kernel_exchange = ds->ids.size() > 1 && ds->peer_ok && !multi_force_copies();
  multi_prove_partials(ds, mk, w, parts);
  assemble_proof(c0, z0, parts, bl.r, bl.s, t0, pts);
  std::vector<uint8_t> pub_store;
  const uint8_t* pubs = w.publics(z0->nPublic, pub_store);
  // The peer-store exchanges rest on a memory-visibility rule that no run on a multi-GPU node has confirmed yet (DESIGN
  // section 6), so the pairing check that normally guards a key's first proof guards its first three here -- a stale
  // receive buffer can only show from the second proof on -- and a proof that fails it is not an error yet: it is
  // repeated with hipMemcpyPeerAsync exchanges (DMA, ordered by the runtime), which then stay on for this process.
  try {
    selfcheck(c0, z0, pts, pubs, kernel_exchange ? 3 : 1);
  } catch (const SelfCheckFailed&) {
    if (!kernel_exchange) throw;
    multi_copies_state().store(1);
    fprintf(stderr, "zkpoa: WARNING: a proof over %zu ranks failed its self-check with the peer-store exchanges; repeating it "
                    "with hipMemcpyPeerAsync exchanges, which stay on for the rest of this process (ZKPOA_EXCHANGE=copy makes "
                    "them the default; DESIGN.md section 6 names the suspects)\n", ds->ids.size());
    multi_prove_partials(ds, mk, w, parts);
    assemble_proof(c0, z0, parts, bl.r, bl.s, t0, pts);
    selfcheck(c0, z0, pts, pubs, ~0ull);   // this one must verify
  }
  vlog("zkpoa: one proof over %zu ranks: H-scalar chain %s, sections 5-8 %s, %.2f GB of fixed-base tables; prove %.2f ms\n",
       ds->ids.size(), mk->split ? "split (2 peer-to-peer exchanges)" : "replicated",
       z0->bc_log ? "block-cyclic" : "contiguous ranges", mk->table_bytes / 1e9, c0->ms[kMsProve]);
  return emit_outputs(c0, z0, pts, pubs, out, mk->load_ms, zkey_size, cache_hit ? "cached," : "sharded load");
}

// ---- device-resident key cache of groth16_prover_zkey_file ("optional device-resident zkey
// cache keyed by path+mtime") ----------------------------------------------------------------------------
// A long-lived caller (the prover server behind the CLI, or an FFI host process) proves many witnesses against
// the same few keys (full_workflow.sh: layer one and two once per batch); uploading 1-21 GB and rebuilding the
// CSR each time is most of a call. Keyed by (device, inode, size, mtime): a rewritten file is a different key.
// ZKPOA_KEY_CACHE = number of keys kept (default 2, 0 = off); least recently used goes first, and everything
// goes when an upload runs out of HBM.
// One container for both kinds of key: a whole key on one GPU (zkpoa_zkey), or a key sharded over the ranks of a
// multi-GPU process (MultiKey: G shard handles + their exchange buffers). An entry owns its key: a key that leaves the
// cache is released. Touched only under g_stage_mutex; changed only with both locks held and g_staged_users == 0.
uint64_t g_key_clock = 0;

size_t key_cache_capacity() { return (size_t)opt_long(O_KEY_CACHE); }

template <class Key, class Free>
struct KeyCache {
  typedef std::unique_ptr<Key, Free> Ptr;
  struct Cached {
    dev_t dev;
    ino_t ino;
    off_t size;
    struct timespec mtime;
    Ptr key;
    uint64_t last_use;
  };
  std::vector<Cached> entries;

  Key* find(const struct stat& sb) {   // a hit counts as a use
    for (auto& c : entries)
      if (c.dev == sb.st_dev && c.ino == sb.st_ino && c.size == sb.st_size && c.mtime.tv_sec == sb.st_mtim.tv_sec &&
          c.mtime.tv_nsec == sb.st_mtim.tv_nsec) {
        c.last_use = ++g_key_clock;
        return c.key.get();
      }
    return nullptr;
  }
  void make_room(size_t cap) {   // for one more key: least recently used goes first
    while (cap && entries.size() >= cap) {
      size_t lru = 0;
      for (size_t i = 1; i < entries.size(); i++)
        if (entries[i].last_use < entries[lru].last_use) lru = i;
      entries.erase(entries.begin() + (long)lru);
    }
  }
  void insert(const struct stat& sb, Ptr key) {
    entries.push_back({sb.st_dev, sb.st_ino, sb.st_size, sb.st_mtim, std::move(key), ++g_key_clock});
  }
  void erase(const Key* key) {
    for (size_t i = 0; i < entries.size(); i++)
      if (entries[i].key.get() == key) {
        entries.erase(entries.begin() + (long)i);
        return;
      }
  }
  void clear() {
    while (!entries.empty()) entries.pop_back();
  }
  // A load that hits a HipError with other keys resident is probably out of HBM: drop them all, clear the error on
  // every device of the set and retry alone.
  template <class Load>
  auto load_retrying_alone(const DeviceSet* ds, Load load) -> decltype(load()) {
    try {
      return load();
    } catch (const HipError&) {
      if (entries.empty()) throw;
    }
    clear();
    for (int d : ds->ids) {
      (void)hipSetDevice(d);
      (void)hipGetLastError();
    }
    return load();
  }
};

KeyCache<zkpoa_zkey, FreeKey> g_key_cache;
KeyCache<MultiKey, std::default_delete<MultiKey>> g_multi_cache;

// When a resident key gets its fixed-base tables (ZKPOA_PRECOMP). A whole set costs 0.25 s at the layer-one shape and
// 3-7 s at layers two and three -- twenty to thirty proofs' worth -- and saves ~10 % per proof, so it pays after a few
// hundred proofs. r02 / r03 built it on the request path at the key's SECOND use: a workflow of two batches
// (tests/4_sigs_2_batches_12_height) then spent 3.4 s on a 0.12 s proof. r04 default ("idle"): never on the request path
// -- zkpoa_idle_work builds one table per call when the library has nothing else to do (the `prover` server calls it
// after 300 ms without a request) -- except for a key that has served ZKPOA_PRECOMP_AFTER proofs (default 64) in a host
// that never calls it. "eager" = the r03 behaviour, "0" = never.
enum PrecompPolicy { kPrecompIdle, kPrecompOff, kPrecompOffWord, kPrecompEager };   // the row's words: idle | 0 | off | eager
// must this request build the key's tables before it proves? (done = proofs the key has served, settled / bytes = its tables)
bool tables_due_now(uint64_t done, bool settled, uint64_t bytes) {
  switch (opt_choice(O_PRECOMP)) {
    case kPrecompEager: return done == 1 && bytes == 0;
    case kPrecompIdle: return done >= (uint64_t)opt_long(O_PRECOMP_AFTER) && !settled && bytes == 0;
    default: return false;
  }
}

// ---- the requests ------------------------------------------------------------------------------------------------------
struct Fd {   // a descriptor the request opened: closed when the request ends
  int fd;
  explicit Fd(int f) : fd(f) {}
  ~Fd() {
    if (fd >= 0) close(fd);
  }
  Fd(const Fd&) = delete;
  Fd& operator=(const Fd&) = delete;
};

struct MappedFile {   // the zkey file, mapped for as long as something reads it (a load; the uploader streams from it)
  const uint8_t* p;
  uint64_t size;
  MappedFile(int fd, const struct stat& sb, const char* path) : size((uint64_t)sb.st_size) {
    void* map = mmap(nullptr, (size_t)size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (map == MAP_FAILED) throw ProverError(PROVER_ERROR, std::string("cannot mmap zkey file ") + path);
    p = reinterpret_cast<const uint8_t*>(map);
  }
  ~MappedFile() { munmap(const_cast<uint8_t*>(p), (size_t)size); }
  MappedFile(const MappedFile&) = delete;
  MappedFile& operator=(const MappedFile&) = delete;
};

// log2(domain) of a zkey image, for the automatic device selection (throws what zkey_parse throws)
uint32_t zkey_power(const uint8_t* buf, uint64_t size) {
  ZkeySections zs;
  return zkey_parse(buf, size, zs)->power;
}

int one_shot(const uint8_t* zkey, uint64_t zkey_size, const WtnsSrc& wsrc, const ProveOut& out) {
  std::string err;
  DeviceSet* ds = nullptr;
  int dcode = PROVER_ERROR;
  try {
    ds = process_devices(zkey_power(zkey, zkey_size), err, &dcode);
  } catch (const std::exception& e) {   // malformed key: nothing touches a GPU
    return out.fail(PROVER_ERROR, e.what());
  }
  if (!ds) return out.fail(dcode, err);
  zkpoa_context* ctx = ds->ctx[0];
  std::lock_guard<std::mutex> lk(g_prove_mutex);
  KeyPtr zk;   // the key lives for this call, whichever way it ends
  MultiKeyPtr mk;
  try {
    ZK_HIP(hipSetDevice(ctx->dev.device));
    if (ds->ids.size() > 1) {   // one proof over all ranks of the process
      mk = multi_key_load(ds, zkey, zkey_size);
      return multi_prove_to_json(ds, mk.get(), wsrc, out, zkey_size, false);
    }
    return load_and_prove_to_json(ctx, zkey, zkey_size, wsrc, out, zk);
  } catch (...) {
    return classify_current_exception(out);
  }
}

// A request on a key sharded over the ranks of the process; both locks held. Load, then prove; the second use of a
// key builds every shard's fixed-base tables, in parallel on the G devices.
int multi_file_prove(DeviceSet* ds, int fd, const struct stat& sb, const char* path, const WtnsSrc& wsrc,
                     const ProveOut& out) {
  int rc = PROVER_OK;
  bool hip_failed = false;
  MultiKey* mk = nullptr;
  MultiKeyPtr own;   // capacity 0: loaded, used once and released by the request
  try {
    const size_t cap = key_cache_capacity();
    mk = g_multi_cache.find(sb);
    const bool hit = mk != nullptr;
    if (!hit) {
      const MappedFile map(fd, sb, path);
      g_multi_cache.make_room(cap);
      own = g_multi_cache.load_retrying_alone(ds, [&] { return multi_key_load(ds, map.p, map.size); });
      mk = own.get();
      if (cap) g_multi_cache.insert(sb, std::move(own));
    }
    if (hit && tables_due_now(mk->proofs_done, mk->tables_tried, mk->table_bytes)) {
      const auto tp0 = std::chrono::steady_clock::now();
      multi_precompute(ds, mk);
      mk->tables_tried = true;
      vlog("zkpoa: fixed-base tables for the cached key on %zu ranks: %.2f GB in %.0f ms\n", ds->ids.size(),
           mk->table_bytes / 1e9, ms_since(tp0));
    }
    rc = multi_prove_to_json(ds, mk, wsrc, out, (uint64_t)sb.st_size, hit);
    mk->proofs_done++;
  } catch (...) {
    rc = classify_current_exception(out, &hip_failed);
  }
  // The shards of a key whose request died in the HIP runtime are not kept for the next request: the entry goes, and
  // with it the shards. This is the multi-GPU path's rule only -- on purpose: the single-GPU path keeps its cached key
  // after a HipError (single_file_prove).
  if (hip_failed) g_multi_cache.erase(mk);
  return rc;
}

// A request on a resident key in steady state (cached, tables built or not wanted): the witness goes into a free
// staging buffer under the stage lock -- which is then dropped -- and the proof runs under the prove lock. Enters with
// stage_lk held, leaves with it released.
int staged_prove(zkpoa_context* ctx, const zkpoa_zkey* zk, const WtnsSrc& wsrc, uint64_t zkey_size,
                 std::unique_lock<std::mutex>& stage_lk, hipStream_t cs, const ProveOut& out) {
  int rc = PROVER_OK, slot = -1;
  try {
    ZK_HIP(hipSetDevice(ctx->dev.device));
    WtnsView w = parse_wtns(wsrc);
    check_witness_len(w, zk);
    g_stage_cv.wait(stage_lk, [&] { return !zk->wbusy[0] || !zk->wbusy[1]; });
    slot = !zk->wbusy[0] ? 0 : 1;
    if (!zk->wbuf[slot]) zk->wbuf[slot].alloc((size_t)zk->nVars * 32);   // (the second one: two requests overlap for the first time)
    zk->wbusy[slot] = true;
    g_staged_users++;
    const auto tu = std::chrono::steady_clock::now();
    w.upload(ctx, zk->wbuf[slot].get(), 0, w.n, cs);      // on the copy stream(s): lane 0 may be busy with another proof's chain
    const float up_ms = (float)ms_since(tu);
    stage_lk.unlock();
    {
      std::lock_guard<std::mutex> lk(g_prove_mutex);
      zk->d_witness = zk->wbuf[slot].get();
      const EnvBlinding bl;
      uint8_t pts[256];
      prove_core(ctx, zk, bl.r, bl.s, pts);
      ctx->io_ms[0] = up_ms;
      ctx->io_ms[1] = (float)((double)w.n * 32 / 1e6);
      rc = check_and_emit(ctx, zk, pts, w, out, 0.0, zkey_size, "cached,");
      const_cast<zkpoa_zkey*>(zk)->proofs_done++;
    }
  } catch (...) {
    rc = classify_current_exception(out);
  }
  if (!stage_lk.owns_lock()) stage_lk.lock();
  if (slot >= 0) {
    zk->wbusy[slot] = false;
    g_staged_users--;
  }
  stage_lk.unlock();
  g_stage_cv.notify_all();
  return rc;
}

// A single-GPU request that changes the cache or a key (a miss, a table build, a first reuse); both locks held. A miss
// loads and proves in one overlapped phase.
int single_file_prove(zkpoa_context* ctx, const DeviceSet* ds, int fd, const struct stat& sb, const char* path,
                      const WtnsSrc& wsrc, const ProveOut& out) {
  int rc = PROVER_OK;
  // A key this request loaded and the cache did not take: released (after hipDeviceSynchronize) when the request ends.
  // That is capacity 0, and a proof that failed after its load (self-check, output): not cached, not leaked.
  KeyPtr own;
  try {
    ZK_HIP(hipSetDevice(ctx->dev.device));
    const size_t cap = key_cache_capacity();
    zkpoa_zkey* zk = g_key_cache.find(sb);
    if (zk) {
      zk->d_witness = zk->wbuf[0].get();   // nothing is staged now: back to the first buffer
      // a key that comes out of the cache is being reused: build its fixed-base tables now, once (ZKPOA_PRECOMP=0 off)
      if (tables_due_now(zk->proofs_done, zk->tables_settled, zk->table_bytes)) {
        const auto tp0 = std::chrono::steady_clock::now();
        try {
          uint64_t used = zkey_precompute(ctx, zk, 0);
          vlog("zkpoa: fixed-base tables for the cached key: %.2f GB in %.0f ms\n", used / 1e9, ms_since(tp0));
        } catch (const HipError&) {   // out of HBM: the classic form keeps working
          zk->release_tables();
          (void)hipGetLastError();
        }
        zk->tables_settled = true;
      }
      rc = prove_to_json(ctx, zk, wsrc, out, 0.0, (uint64_t)sb.st_size, true);
    } else {
      const MappedFile map(fd, sb, path);   // outlives the overlapped phase: the uploader streams from it
      g_key_cache.make_room(cap);
      rc = g_key_cache.load_retrying_alone(
          ds, [&] { return load_and_prove_to_json(ctx, map.p, map.size, wsrc, out, own, fd); });
      zk = own.get();
      if (cap) g_key_cache.insert(sb, std::move(own));
    }
    zk->proofs_done++;
  } catch (...) {
    rc = classify_current_exception(out);   // (a HipError does not evict here; the multi-GPU path does: multi_file_prove)
  }
  return rc;
}

int zkey_file_prove(const char* path, const WtnsSrc& wsrc, const ProveOut& out) {
  const Fd zkey(open(path, O_RDONLY));
  if (zkey.fd < 0) return out.fail(PROVER_ERROR, std::string("cannot open zkey file ") + path);
  struct stat sb;
  if (fstat(zkey.fd, &sb) != 0 || sb.st_size == 0) return out.fail(PROVER_ERROR, std::string("cannot stat zkey file ") + path);
  std::string err;
  DeviceSet* ds = nullptr;
  int dcode = PROVER_ERROR;
  try {
    uint32_t power = 0;
    if (!devices_ready()) {   // the first key of the process decides the device list: its domain size is in the header
      const MappedFile map(zkey.fd, sb, path);
      power = zkey_power(map.p, map.size);
    }
    ds = process_devices(power, err, &dcode);
  } catch (const std::exception& e) {   // malformed key: nothing touches a GPU
    return out.fail(PROVER_ERROR, e.what());
  }
  if (!ds) return out.fail(dcode, err);
  zkpoa_context* ctx = ds->ctx[0];
  std::unique_lock<std::mutex> stage_lk(g_stage_mutex);
  if (ds->ids.size() == 1) {   // steady state of a resident single-GPU key: stage the witness, then prove (two locks)
    if (const zkpoa_zkey* zk = g_key_cache.find(sb)) {
      const uint64_t done = zk->proofs_done.load();
      hipStream_t cs = ctx->dev.copy_stream_wait();
      if (done >= 1 && !tables_due_now(done, zk->tables_settled, zk->table_bytes) && cs)
        return staged_prove(ctx, zk, wsrc, (uint64_t)sb.st_size, stage_lk, cs, out);
    }
  }
  // everything else changes the cache or a key: alone, with both locks
  g_stage_cv.wait(stage_lk, [] { return g_staged_users == 0; });
  std::lock_guard<std::mutex> lk(g_prove_mutex);
  return ds->ids.size() > 1 ? multi_file_prove(ds, zkey.fd, sb, path, wsrc, out)
                            : single_file_prove(ctx, ds, zkey.fd, sb, path, wsrc, out);
}

// zkpoa_idle_work (prover.hip): one step of background work, or 0 when there is none or a request is in flight
int idle_work() {
  if (opt_choice(O_PRECOMP) != kPrecompIdle) return 0;
  std::unique_lock<std::mutex> stage_lk(g_stage_mutex, std::try_to_lock);
  if (!stage_lk.owns_lock() || g_staged_users) return 0;
  std::unique_lock<std::mutex> lk(g_prove_mutex, std::try_to_lock);
  if (!lk.owns_lock()) return 0;
  DeviceSet* ds = nullptr;
  {
    std::lock_guard<std::mutex> dl(g_devset_mutex);
    ds = g_devset;
  }
  if (!ds) return 0;
  try {
    if (ds->ids.size() > 1) {   // a sharded key: the whole set of tables in one step, no warm-up proof
      for (auto& c : g_multi_cache.entries)
        if (c.key->proofs_done >= 1 && c.key->table_bytes == 0 && !c.key->tables_tried) {
          const auto t0 = std::chrono::steady_clock::now();
          c.key->tables_tried = true;
          multi_precompute(ds, c.key.get());
          vlog("zkpoa: idle: fixed-base tables for the cached key on %zu ranks: %.2f GB in %.0f ms\n", ds->ids.size(),
               c.key->table_bytes / 1e9, ms_since(t0));
          return 1;
        }
      return 0;
    }
    zkpoa_zkey* pick = nullptr;   // the most recently used key that still wants tables
    uint64_t pick_use = 0;
    for (auto& c : g_key_cache.entries)
      if (c.key->proofs_done.load() >= 1 && !c.key->tables_settled && (!pick || c.last_use > pick_use)) {
        pick = c.key.get();
        pick_use = c.last_use;
      }
    zkpoa_context* ctx = ds->ctx[0];
    ZK_HIP(hipSetDevice(ctx->dev.device));
    if (!pick) {
      // Tables complete: one throw-away proof on the witness the key still holds. Building the tables gave the lanes'
      // workspaces back to the allocator, and the first proof through the tables would otherwise pay for regrowing them
      // (0.5-0.6 s at the layer-two / -three shapes) inside a request.
      for (auto& c : g_key_cache.entries)
        if (c.key->tables_settled && c.key->table_bytes && !c.key->warmed && c.key->d_witness && is_full_key(c.key.get())) {
          const auto t0 = std::chrono::steady_clock::now();
          c.key->warmed = true;
          uint8_t parts[384];
          prove_partials(ctx, c.key.get(), parts);
          vlog("zkpoa: idle: warm-up proof through the new tables: %.0f ms\n", ms_since(t0));
          return 1;
        }
      return 0;
    }
    const uint64_t before = pick->table_bytes;
    const auto t0 = std::chrono::steady_clock::now();
    try {
      (void)zkey_precompute(ctx, pick, 0, 1);
    } catch (const HipError&) {   // out of HBM: what exists stays, nothing more is tried
      (void)hipGetLastError();
      pick->tables_settled = true;
    }
    vlog("zkpoa: idle: fixed-base table step for the cached key: +%.2f GB in %.0f ms (%.2f GB so far%s)\n",
         (pick->table_bytes - before) / 1e9, ms_since(t0), pick->table_bytes / 1e9, pick->tables_settled ? ", complete" : "");
    return 1;
  } catch (const std::exception&) {
    return 0;
  }
}
