// `merkle-tree` -- drop-in for the reference's Rust binary of the same name (scripts/merkle_tree.rs, Cargo.toml:18-20),
// exec'd at scripts/full_workflow.sh:371-380 as
//     merkle-tree --anon-set <anonymity_set.csv> --poa-input-data <parsed_sigs.json> --output-dir <dir>
// Writes <dir>/merkle_root.json and <dir>/merkle_proofs.json in the shapes merkle_tree.rs serialises (serde_json
// pretty printing: 2-space indent): the Poseidon Merkle root of the anonymity set and, for every owned address of the
// parsed-signatures file (in file order, located as the forward scan of merkle_tree.rs:329-346 locates them), its leaf,
// sibling path and index bits. The hashing runs on the GPU (libzkpoa_prover.so: csrc/poseidon.hip), and so do the lookup
// of the owned leaves (through the stable index of the tree's leaves) and the gather of their paths: a million owned
// addresses are one find and sixteen gathers, not 25 M copies. The reference's own note says 2.5 hours for a 10 M set on
// the CPU (merkle_tree.rs:3-5). Exit status 0 / non-zero + message, like the prover.
//     --any-order (not the reference's): the owned addresses may come in any order; entry i gets the lowest row whose
//     leaf equals it, and the output stays in the owned file's order.
#include "../../include/zkpoa_prover.h"
#include "anon_set_file.hpp"

#include <algorithm>
#include <chrono>
#include <memory>

using namespace zkpoa;

// This main is a client of the C ABI and sees the public header only, so the time slot it reads is the public id.
constexpr int kFindKernelsMsId = 10;   // zkpoa_last_ms: the kernels of the last find or path gather

// ---- the owned addresses: accountAttestations[].accountData.{address, balance}.__bigint__ (decimal), merkle_tree.rs:
// 296-327. The file is 1.6 GB at 2^20 entries: it is pulled through its mapping, and whatever else it holds is skipped.
struct Owned {
  std::vector<uint64_t> addr, bal;       // 4 limbs per entry
  std::vector<std::string> addr_s, bal_s;   // as given: the proofs file repeats them
};
static void read_owned(const std::string& path, Owned& o) {
  const MappedFile text(path.c_str());
  Json js{text.begin(), text.end()};
  bool seen = false;
  js.object([&](const Span& key) {
    if (!key.is("accountAttestations")) return js.skip();
    seen = true;
    js.array([&](uint64_t i) {
      Span field[2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // address, balance
      js.object([&](const Span& k1) {
        if (!k1.is("accountData")) return js.skip();
        js.object([&](const Span& k2) {
          const int f = k2.is("address") ? 0 : k2.is("balance") ? 1 : -1;
          if (f < 0) return js.skip();
          js.object([&](const Span& k3) {
            if (!k3.is("__bigint__")) return js.skip();
            field[f] = js.scalar();
          });
        });
      });
      if (!field[0].b || !field[1].b)
        throw std::runtime_error("entry " + std::to_string(i) + " has no accountData.{address, balance}.__bigint__");
      const U256 av = parse_num(field[0].b, field[0].e, false, "address"), bv = parse_num(field[1].b, field[1].e, false, "balance");
      o.addr.insert(o.addr.end(), av.v, av.v + 4);
      o.bal.insert(o.bal.end(), bv.v, bv.v + 4);
      o.addr_s.push_back(field[0].str());
      o.bal_s.push_back(field[1].str());
    });
  });
  js.end();
  if (!seen) throw std::runtime_error("no accountAttestations in " + path);
}

#define ZK_CALL(expr, what)                                                                       \
  do {                                                                                            \
    if ((expr) != PROVER_OK) throw std::runtime_error(std::string(what) + ": " + zkpoa_last_error(ctx)); \
  } while (0)

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char** argv) {
  const bool verbose = opt_verbose();
  std::string anon, poa, outdir;
  bool any_order = false;   // not the reference's: the owned addresses need not come in the set's order
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    auto val = [&](std::string& dst) {
      size_t eq = a.find('=');
      if (eq != std::string::npos) dst = a.substr(eq + 1);
      else if (i + 1 < argc) dst = argv[++i];
    };
    if (a == "-a" || a.rfind("--anon-set", 0) == 0) val(anon);
    else if (a == "-p" || a.rfind("--poa-input-data", 0) == 0) val(poa);
    else if (a == "-o" || a.rfind("--output-dir", 0) == 0) val(outdir);
    else if (a == "--any-order") any_order = true;
    else if (a == "-h" || a == "--help") {
      printf("Construct a Merkle Tree for the anonymity set of Ethereum addresses & balances.\n\n"
             "Usage: merkle-tree --anon-set <FILE_PATH> --poa-input-data <FILE_PATH> --output-dir <DIR_PATH> [--any-order]\n");
      return 0;
    }
  }
  if (anon.empty() || poa.empty() || outdir.empty()) {
    fprintf(stderr, "error: the following required arguments were not provided: --anon-set <FILE_PATH> "
                    "--poa-input-data <FILE_PATH> --output-dir <DIR_PATH>\n");
    return 2;
  }
  zkpoa_merkle* tree = nullptr;
  int rc = 0;
  try {
    printf("Initiating Merkle Tree build..\n");
    printf("Trying to read given file '\"%s\"'\n", anon.c_str());
    // csv: heading line "address,eth_balance", then 0x-prefixed hex address, decimal balance (merkle_tree.rs:212-246)
    ContextStart start(device_from_env());   // the device starts up while this thread reads the set
    Limbs addr, bal;
    const double t0 = now_s();
    read_anonymity_set(anon, addr, bal);
    const double t_read = now_s();
    const uint64_t n = addr.rows;
    if (n == 0) throw std::runtime_error("the anonymity set is empty");
    printf("Converting lines in '\"%s\"' into leaf nodes.. (leaf node = hash(address, balance))\n", anon.c_str());
    zkpoa_context* ctx = start.get();
    const double t_ctx = now_s();
    ZK_CALL(zkpoa_merkle_build(ctx, addr.data(), bal.data(), n, &tree), "merkle tree build");
    if (verbose)
      fprintf(stderr, "merkle-tree: read %llu rows %.3f s, waited %.3f s more for the device, leaves + tree (with the upload) %.3f s\n",
              (unsigned long long)n, t_read - t0, t_ctx - t_read, now_s() - t_ctx);
    uint64_t info[3];
    zkpoa_merkle_info(tree, info);
    printf("Done creating %llu leaves\n", (unsigned long long)n);
    printf("Number of leaves (after adding padding nodes): %llu\n", 1ull << info[1]);
    printf("Creating Merkle tree..\n");
    printf("Done creating Merkle tree of height %llu\n", (unsigned long long)info[1] + 1);   // rs_merkle depth()
    const double t_paths = now_s();
    Owned own;   // read before anything is written: a file that cannot be read leaves no output behind
    read_owned(poa, own);
    U256 root;
    ZK_CALL(zkpoa_merkle_root(ctx, tree, reinterpret_cast<uint8_t*>(root.v)), "merkle root");
    const std::string root_path = outdir + "/merkle_root.json", proofs_path = outdir + "/merkle_proofs.json";
    write_text_atomic(root_path, "{\n  \"__bigint__\": \"" + root.dec() + "\"\n}");
    printf("Root hash %s written to file \"%s\"\n", root.dec().c_str(), root_path.c_str());

    const uint64_t m = own.addr_s.size();
    std::vector<uint64_t> ohash(4 * (m ? m : 1));
    const double t_hash = now_s();
    if (m) ZK_CALL(zkpoa_poseidon2(ctx, own.addr.data(), own.bal.data(), m, ohash.data()), "owned leaf hashes");
    // Where the owned leaves are: through the tree's stable index of its leaves, on the device. By default the answer
    // is the forward scan's (merkle_tree.rs:329-346: the owned addresses must appear in the set in the same order, or
    // the Rust binary panics): the index's answer is taken only where the scan provably gives the same -- every owned
    // leaf is in the set exactly once and the rows do not go down (a repeated entry is fine: the scan does not advance
    // past a match). Everything else -- a leaf that is absent, out of order, or on several rows -- is the scan's to
    // decide. --any-order: entry i is the lowest row whose leaf equals it, whatever the order.
    const double t_find = now_s();
    std::vector<uint32_t> first(m ? m : 1), count(m ? m : 1);
    if (m) ZK_CALL(zkpoa_merkle_find(ctx, tree, ohash.data(), m, first.data(), count.data()), "find owned leaves");
    const float find_kernel_ms = zkpoa_last_ms(ctx, kFindKernelsMsId);
    std::vector<uint64_t> index(m);
    bool indexed = true;
    for (uint64_t i = 0; i < m; i++) {
      if (any_order) {
        if (count[i] == 0)
          throw std::runtime_error("Owned leaf " + own.addr_s[i] + " at index " + std::to_string(i) +
                                   " does not exist in the anonymity set");
      } else if (count[i] != 1 || (i && first[i] < first[i - 1])) {
        indexed = false;
        break;
      }
      index[i] = first[i];
    }
    if (!indexed) {
      // forward scan of the anonymity set for each owned leaf, in order
      std::vector<uint64_t> leaves(4 * n);
      ZK_CALL(zkpoa_merkle_leaves(ctx, tree, 0, n, leaves.data()), "read leaves");
      uint64_t pos = 0;
      for (uint64_t i = 0; i < m; i++) {
        while (pos < n && memcmp(&leaves[4 * pos], &ohash[4 * i], 32) != 0) pos++;
        if (pos >= n)
          throw std::runtime_error("Owned leaf " + own.addr_s[i] + " at index " + std::to_string(i) +
                                   " does not exist in the anonymity set");
        index[i] = pos;
      }
    }
    const double t_text = now_s();
    // merkle_proofs.json: three arrays of m entries, formatted by the host threads 2^16 entries at a time; the paths of
    // a round are gathered on the device just before its entries are formatted, so host memory does not grow with m
    const unsigned k = (unsigned)info[1];
    double paths_s = 0;
    float gather_kernel_ms = 0;
    AtomicFile fo(proofs_path.c_str());
    uint64_t off = 0;
    put_text(fo, off, "{\n  \"leaves\": [");
    put_entries(fo, off, m, 256, 260, [&](std::string& o, uint64_t i) {
      U256 h;
      memcpy(h.v, &ohash[4 * i], 32);
      o += i ? "," : "";
      o += "\n    {\n      \"address\": {\n        \"__bigint__\": \"";
      o += own.addr_s[i];
      o += "\"\n      },\n      \"balance\": {\n        \"__bigint__\": \"";
      o += own.bal_s[i];
      o += "\"\n      },\n      \"hash\": {\n        \"__bigint__\": \"";
      h.append_dec(o);
      o += "\"\n      }\n    }";
    });
    put_text(fo, off, m ? "\n  ],\n  \"path_elements\": [" : "],\n  \"path_elements\": [");
    std::vector<uint64_t> path(4 * (size_t)std::min<uint64_t>(m, kEntryRound) * k + 4);
    uint64_t path_i0 = 0;
    put_entries(fo, off, m, 64, 120 * (uint64_t)k + 16,
                [&](uint64_t i0, uint64_t cnt) {
                  const double t0 = now_s();
                  ZK_CALL(zkpoa_merkle_paths(ctx, tree, index.data() + i0, cnt, reinterpret_cast<uint8_t*>(path.data()), nullptr),
                          "merkle paths");
                  paths_s += now_s() - t0;
                  gather_kernel_ms += zkpoa_last_ms(ctx, kFindKernelsMsId);
                  path_i0 = i0;
                },
                [&](std::string& o, uint64_t i) {
                  o += i ? ",\n    [" : "\n    [";
                  for (unsigned l = 0; l < k; l++) {
                    U256 e;
                    memcpy(e.v, &path[4 * ((i - path_i0) * k + l)], 32);
                    o += l ? ",\n      {\n        \"__bigint__\": \"" : "\n      {\n        \"__bigint__\": \"";
                    e.append_dec(o);
                    o += "\"\n      }";
                  }
                  o += k ? "\n    ]" : "]";
                });
    put_text(fo, off, m ? "\n  ],\n  \"path_indices\": [" : "],\n  \"path_indices\": [");
    put_entries(fo, off, m, 256, 9 * (uint64_t)k + 16, [&](std::string& o, uint64_t i) {
      o += i ? ",\n    [" : "\n    [";
      for (unsigned l = 0; l < k; l++) {   // the index bit per level (merkle_tree.rs build_path_indices)
        o += l ? ",\n      " : "\n      ";
        o += (char)('0' + ((index[i] >> l) & 1));
      }
      o += k ? "\n    ]" : "]";
    });
    put_text(fo, off, m ? "\n  ]\n}" : "]\n}");
    fo.commit();
    if (verbose)
      fprintf(stderr, "merkle-tree: owned leaves: hashes %.3f s, find %.3f s (kernels %.2f ms, %s), paths %.3f s (gather kernels %.2f ms, "
                      "the rest is the read-back), text and file %.3f s\n", t_find - t_hash, t_text - t_find, find_kernel_ms,
              indexed ? "through the index" : "then the forward scan", paths_s, gather_kernel_ms, now_s() - t_text - paths_s);
    if (verbose) fprintf(stderr, "merkle-tree: %llu paths and both files %.3f s\n", (unsigned long long)m, now_s() - t_paths);
  } catch (const std::exception& e) {
    fprintf(stderr, "Error: %s\n", e.what());
    rc = 1;
  }
  // Both files are complete and renamed into place (or the error is on stderr): leave without the HIP runtime's
  // teardown, as `prover` does -- freeing the tree and the context's queues is ~0.1 s a one-shot command never gets back
  fflush(stdout);
  fflush(stderr);
  _exit(rc);
}
