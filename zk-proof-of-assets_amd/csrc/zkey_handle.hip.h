// The device-resident proving key behind the C ABI's zkpoa_zkey: what it holds and owns, which shard of the five MSMs
// it covers, and the header points in their wire form. Every loader, the key cache, the resident server and the
// multi-GPU path share this one object.
// Included by prover.hip at file scope (the C ABI names the struct), after ProverError.
#pragma once

// The five points of a zkey header the prover needs. Wire form (zkpoa_zkey_header, zkpoa_prove_assemble,
// zkpoa_zkey_load_device): alpha1(64) beta1(64) beta2(128) delta1(64) delta2(128).
struct HeaderPoints {   // (members in wire order)
  Affine<HFq> alpha1, beta1;
  Affine<HFq2> beta2;
  Affine<HFq> delta1;
  Affine<HFq2> delta2;
};
static HeaderPoints header_points(const uint8_t* alpha1, const uint8_t* beta1, const uint8_t* beta2, const uint8_t* delta1,
                                  const uint8_t* delta2) {
  return {h_affine_from_bytes<HFq>(alpha1), h_affine_from_bytes<HFq>(beta1), h_affine_from_bytes<HFq2>(beta2),
          h_affine_from_bytes<HFq>(delta1), h_affine_from_bytes<HFq2>(delta2)};
}
static HeaderPoints header_points_from_bytes(const uint8_t in[448]) {   // the inverse of zkey_header_bytes
  return header_points(in, in + 64, in + 128, in + 256, in + 320);
}

// A and B queries without their points at infinity (abc.hip.h): compacted copies of the resident range of
// section 5 resp. 6 / 7, the wire of every kept point, pos[i] = kept points before resident wire i (a shard's
// slice of the compacted arrays is [pos[wlo - wbase], pos[wlo + wcnt - wbase])), and the gathered scalars.
struct CompactQuery {
  DevMem g1, g2, scalars;
  DevMem wire, pos;          // u32 each
  uint64_t res = 0;          // kept points in the resident range
  uint64_t lo = 0, cnt = 0;  // this shard's slice of them
};

// ---- device-resident proving key -------------------------------------------------------------------
// Every device array is a DevMem member, so the compiler's destructor gives back exactly what the handle owns. A
// handle that has touched a device is destroyed through FreeKey (below), which drains that device first.
struct zkpoa_zkey {
  int device = -1;   // HIP ordinal of the context the arrays live on; -1 while the handle is host state only
  uint32_t nVars = 0, nPublic = 0, domain = 0, power = 0;
  uint64_t nCoefs = 0;
  HeaderPoints hdr;
  // Verification key carried by the zkey itself (section 2: alpha1, beta2, gamma2, delta2; section 3: IC), wire
  // format alpha1(64) beta2(128) gamma2(128) delta2(128) IC[(nPublic+1) x 64]. Empty for keys assembled from
  // device buffers (zkpoa_zkey_load_device has no gamma2 / IC). Used by the self-check of the first proof(s).
  std::vector<uint8_t> vkey_points;
  mutable uint64_t selfchecks_done = 0;
  // The point sections: the handle's own uploads, or lent by the caller (zkpoa_zkey_load_device: DevMem::lent). dA, dB1
  // and dB2 are given up once their compacted copies exist (queries_compact).
  DevMem dA, dB1, dB2, dC, dH;
  DevMem d_row_ptr;           // u32; CSR of the coefficients by output row (build_csr)
  DevMem d_long;              // u32; constraints with more than kLongRow coefficients (abc.hip.h), n_long of them
  uint32_t n_long = 0;
  DevMem d_sig;               // u32
  DevMem d_vals;
  DevMem d_flag;              // u32; [0]: a witness value >= r was seen by the last prove (range_check_kernel)
  DevMem d_abc;               // 3 * domain * 32 B work area (A_T, B_T, C_T)
  // The witness, nVars * 32 B: the handle owns up to two buffers and d_witness is a view of the one the next prove
  // reads. Every loader allocates wbuf[0]; the resident prover (zkey_file_prove) allocates wbuf[1] when a second request
  // first overlaps, so that the witness of the NEXT request is uploaded while the current proof computes.
  mutable DevMem wbuf[2];
  mutable void* d_witness = nullptr;
  mutable bool wbusy[2] = {false, false};
  // Shard of the MSMs this handle covers: contiguous global index ranges. The device
  // buffers dA/dB1/dB2 start at global wire index `wbase`, dC at C-section index `cbase`, dH at `hbase`.
  uint64_t wlo = 0, wcnt = 0, wbase = 0;   // A, B1, B2: wire indices [wlo, wlo + wcnt)
  uint64_t clo = 0, ccnt = 0, cbase = 0;   // C: section indices (wire nPublic+1+idx)
  uint64_t hlo = 0, hcnt = 0, hbase = 0;   // H: domain indices
  // Split H-scalar chain (SURVEY.md 8e rows NTT / buildABC / joinABC): split_world = G > 1 ranks each own the
  // constraint rows c = split_rank (mod G) and end up with the H scalars of the odd-coset indices
  // i = split_rank (mod G), so the H points are sharded cyclically: dHs[t] = H[t*G + split_rank].
  uint32_t split_world = 0, split_rank = 0, split_log = 0;
  bool csr_local = false;        // CSR holds only this rank's rows, renumbered c >> split_log
  DevMem dHs;                    // cyclic H shard (always the handle's own), domain / split_world points
  mutable bool h_ready = false;  // d_abc[0 .. domain/split_world) holds this proof's H scalars (stage 3 done)
  uint64_t nCoefsLocal = 0;
  // Block-cyclic shard of sections 5-8 (bc_log > 0; shard handles only): this rank holds the blocks b = bc_rank
  // (mod bc_world) of 2^bc_log consecutive items -- wires for A / B1 / B2, section indices for C -- concatenated. A
  // contiguous range inherits whatever clustering a real witness has (bit-decomposition wires come in runs of cheap
  // 0 / 1 scalars, limbs in runs of full-width ones), so ranks would finish at different times; blocks of 2^16 wires
  // dealt round-robin even that out while every block is still one contiguous byte range of the file. Local index j
  // of a section <-> global index (((j >> L) * world + rank) << L) + (j & (2^L - 1)).
  uint32_t bc_log = 0, bc_rank = 0, bc_world = 1;
  DevMem d_cscal;                // block-cyclic handles: the C query's witness values, gathered per proof
  static uint64_t bc_count(uint64_t n, uint32_t L, uint64_t rank, uint64_t world) {
    const uint64_t B = 1ull << L, nb = (n + B - 1) >> L;
    if (nb <= rank) return 0;
    uint64_t cnt = ((nb - rank + world - 1) / world) << L;
    if ((nb - 1) % world == rank && (n & (B - 1))) cnt -= B - (n & (B - 1));
    return cnt;
  }
  CompactQuery qA, qB;
  // Fixed-base tables (msm.hip.h MsmTable; zkpoa_zkey_precompute): 2^(c*j) * P for every window j of a whole
  // resident base array -- the compacted A / B queries, section 8, section 9. An MSM uses its table only when it
  // covers exactly that array (a re-pointed shard of a resident key falls back to the classic form).
  MsmTablePtr tA, tB1, tB2, tC, tH;
  bool tH_cyclic = false;     // tH was built from the cyclic shard dHs (split handles), not from dH
  uint64_t table_bytes = 0;
  // incremental build (zkey_precompute_step: one table per call, from the resident prover's idle time)
  uint64_t table_budget = 0;  // fixed at the first step (half of the HBM free then)
  bool tables_settled = false;   // every table that is wanted and fits has been built (or an attempt failed)
  bool warmed = false;           // a throw-away proof has run since the tables settled (the lanes' workspaces regrown)
  // digit density of the last witness measured on this handle (msm_density: non-zero digits per scalar for every
  // window width). A circuit's witnesses all look alike (bits stay bits), so it is measured by the first proof only
  // and sizes the windows of later proofs and of the witness tables (zkey_precompute after a proof).
  mutable double witness_density[32];
  mutable bool have_density = false;
  std::atomic<uint64_t> proofs_done{0};   // groth16_prover_zkey_file's cache precomputes when a key is used a second time
  void release_tables() {
    for (MsmTablePtr* t : {&tA, &tB1, &tB2, &tC, &tH}) t->reset();
    table_bytes = 0;
    tH_cyclic = false;
    table_budget = 0;
    tables_settled = false;
    warmed = false;
  }
  void release_cyclic_h_table() {   // a new cyclic shard replaces dHs: the table built from the old one goes
    if (!tH_cyclic) return;
    uint64_t info[4];
    msm_table_info(tH.get(), info);
    table_bytes -= std::min(info[3], table_bytes);
    tH.reset();
    tH_cyclic = false;
  }
  // H scalars one proof leaves in d_abc: a rank of a split chain computes its domain / G, anyone else all of them
  static uint64_t split_h_count(uint64_t domain, uint64_t world) { return domain / world; }
  uint64_t h_scalar_count() const { return split_world > 1 ? split_h_count(domain, split_world) : domain; }
  static void split(uint64_t n, uint64_t rank, uint64_t world, uint64_t& lo, uint64_t& cnt) {
    uint64_t base = n / world, rem = n % world;
    lo = rank * base + (rank < rem ? rank : rem);
    cnt = base + (rank < rem ? 1 : 0);
  }
  void set_shard(uint64_t rank, uint64_t world) {
    split(nVars, rank, world, wlo, wcnt);
    split((uint64_t)nVars - nPublic - 1, rank, world, clo, ccnt);
    split(domain, rank, world, hlo, hcnt);
  }
};

// The one way a handle ends (zkpoa_zkey_free, a request's KeyPtr, the key cache, a MultiKey's ranks): whatever its
// device still runs may read the arrays, so the device drains before they go.
struct FreeKey {
  void operator()(zkpoa_zkey* zk) const {
    if (zk->device >= 0) {
      (void)hipSetDevice(zk->device);
      (void)hipDeviceSynchronize();
    }
    delete zk;
  }
};
typedef std::unique_ptr<zkpoa_zkey, FreeKey> KeyPtr;

// split chain: world must be a power of two <= 8 with world^2 <= domain (every rank owns whole slots of
// every other rank's transform)
static void check_split(const zkpoa_zkey* zk, uint64_t rank, uint64_t world) {
  if (world < 2 || world > 8 || (world & (world - 1)) || rank >= world)
    throw ProverError(PROVER_ERROR, "split chain: world must be 2, 4 or 8 and rank < world");
  if ((uint64_t)zk->domain < world * world)
    throw ProverError(PROVER_ERROR, "split chain: domain smaller than world^2");
}

static void set_split(zkpoa_zkey* zk, uint64_t rank, uint64_t world) {
  zk->split_world = (uint32_t)world;
  zk->split_rank = (uint32_t)rank;
  zk->split_log = world == 2 ? 1 : (world == 4 ? 2 : 3);
  zk->h_ready = false;
}

// shard flags of the loaders (include/zkpoa_prover.h ZKPOA_SHARD_*): bit 0 = split chain, bits 8-15 = block-cyclic log
static void set_block_cyclic(zkpoa_zkey* zk, uint64_t rank, uint64_t world, uint32_t bc_log) {
  if (bc_log == 0 || world <= 1) return;
  if (bc_log < 4 || bc_log > 24) throw ProverError(PROVER_ERROR, "zkey shard: block-cyclic block size must be 2^4 .. 2^24 items");
  zk->bc_log = bc_log;
  zk->bc_rank = (uint32_t)rank;
  zk->bc_world = (uint32_t)world;
  zk->wlo = zk->wbase = 0;
  zk->wcnt = zkpoa_zkey::bc_count(zk->nVars, bc_log, rank, world);
  zk->clo = zk->cbase = 0;
  zk->ccnt = zkpoa_zkey::bc_count((uint64_t)zk->nVars - zk->nPublic - 1, bc_log, rank, world);
}

// A new handle (its sizes set) becomes shard `rank` of `world`; world == 1: the whole key. Host state only: the
// ranges, whose resident arrays start at the ranges themselves, then the split chain and the block-cyclic deal.
static void shard_init(zkpoa_zkey* zk, uint64_t rank, uint64_t world, bool split, uint32_t bc_log) {
  if (world == 0 || rank >= world) throw ProverError(PROVER_ERROR, "zkey shard: rank/world out of range");
  zk->set_shard(rank, world);
  zk->wbase = zk->wlo; zk->cbase = zk->clo; zk->hbase = zk->hlo;
  if (split) {
    check_split(zk, rank, world);
    set_split(zk, rank, world);
    zk->hlo = zk->hbase = 0;
    zk->hcnt = 0;   // no contiguous H range on this handle: its H points are the cyclic shard dHs
  }
  set_block_cyclic(zk, rank, world, bc_log);
}

// Can the handle be re-pointed at another shard? Only when every section is resident from its first item in file
// order (loaded whole, not block-cyclic) and the CSR holds every row.
static bool resident_unsharded(const zkpoa_zkey* zk) {
  return !(zk->wbase || zk->cbase || zk->hbase || zk->csr_local || !zk->dH || zk->bc_log);
}

static bool is_full_key(const zkpoa_zkey* zk) {
  return zk->split_world <= 1 && zk->wlo == 0 && zk->wcnt == zk->nVars && zk->clo == 0 && zk->ccnt == (uint64_t)zk->nVars - zk->nPublic - 1 &&
         zk->hlo == 0 && zk->hcnt == zk->domain;
}

static void zkey_header_bytes(const zkpoa_zkey* zk, uint8_t out[448]) {
  h_affine_to_bytes<HFq>(zk->hdr.alpha1, out);
  h_affine_to_bytes<HFq>(zk->hdr.beta1, out + 64);
  h_affine_to_bytes<HFq2>(zk->hdr.beta2, out + 128);
  h_affine_to_bytes<HFq>(zk->hdr.delta1, out + 256);
  h_affine_to_bytes<HFq2>(zk->hdr.delta2, out + 320);
}
