// `zkpoa-audit` -- the verifier's side of the protocol, which the reference leaves unwritten ("Verifier: script still
// needs to be written", its README): the published anonymity set, the layer-three verification key, public.json and
// proof.json in, one verdict out.
//     zkpoa-audit --anon-set <anonymity_set.csv> --vkey <layer_three_vkey.json> --public <public.json> --proof <proof.json>
//                 [--commitment <64 hex>]
//                 [--state-proofs <proofs.jsonl> (--state-root <0x + 64 hex> | --block-header <0x-hex RLP | @file>)
//                  [--balance-unit wei|gwei|ether]]
// The set is read like `merkle-tree` reads it (anon_set_file.hpp); the duplicate check and the Merkle root run on the
// GPU, the commitment and the Groth16 verification on the host (zkpoa_assets_verify). One line per check on stdout, then
// "AUDIT OK" or "AUDIT FAILED: <names>". With --state-proofs the set's balances are checked against an Ethereum state
// root as well (zkpoa_anon_set_state_check_file: one eth_getProof result per line), which adds a line `state:` after
// `duplicates:` and, with --block-header, a first line `block:` with the header's hash for the auditor to compare with
// their own node or an explorer. Exit status 0 when every check passed, 1 when one failed, 2 for a usage error
// or input that cannot be read (then nothing is printed on stdout).
#include "../../include/zkpoa_prover.h"
#include "anon_set_file.hpp"

#include <chrono>

using namespace zkpoa;

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static std::string hex32(const uint8_t* b) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (int i = 0; i < 32; i++) {
    s.push_back(d[b[i] >> 4]);
    s.push_back(d[b[i] & 15]);
  }
  return s;
}

static std::string file_text(const std::string& path) {
  const MappedFile f(path.c_str());
  return std::string(f.begin(), f.end());
}

int main(int argc, char** argv) {
  const bool verbose = opt_verbose();
  std::string anon, vkey, pub, proof, commitment, state_proofs, state_root, block_header, balance_unit;
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    auto val = [&](std::string& dst) {
      size_t eq = a.find('=');
      if (eq != std::string::npos) dst = a.substr(eq + 1);
      else if (i + 1 < argc) dst = argv[++i];
    };
    if (a.rfind("--state-proofs", 0) == 0) val(state_proofs);
    else if (a.rfind("--state-root", 0) == 0) val(state_root);
    else if (a.rfind("--block-header", 0) == 0) val(block_header);
    else if (a.rfind("--balance-unit", 0) == 0) val(balance_unit);
    else if (a.rfind("--anon-set", 0) == 0) val(anon);
    else if (a.rfind("--vkey", 0) == 0) val(vkey);
    else if (a.rfind("--public", 0) == 0) val(pub);
    else if (a.rfind("--proof", 0) == 0) val(proof);
    else if (a.rfind("--commitment", 0) == 0) val(commitment);
    else if (a == "-h" || a == "--help") {
      printf("Check a published proof of assets: the anonymity set, its root, the commitment and the proof.\n\n"
             "Usage: zkpoa-audit --anon-set <FILE_PATH> --vkey <FILE_PATH> --public <FILE_PATH> --proof <FILE_PATH> "
             "[--commitment <64 hex>]\n"
             "       [--state-proofs <FILE_PATH> (--state-root <0x + 64 hex> | --block-header <0x-hex RLP | @FILE_PATH>) "
             "[--balance-unit wei|gwei|ether]]\n");
      return 0;
    } else {
      fprintf(stderr, "error: unexpected argument '%s'\n", a.c_str());
      return 2;
    }
  }
  if (anon.empty() || vkey.empty() || pub.empty() || proof.empty()) {
    fprintf(stderr, "error: the following required arguments were not provided: --anon-set <FILE_PATH> --vkey <FILE_PATH> "
                    "--public <FILE_PATH> --proof <FILE_PATH>\n");
    return 2;
  }
  // the state check: the proofs and exactly one source of the root, or none of its options
  const bool state = !state_proofs.empty();
  if (state ? state_root.empty() == block_header.empty() : !(state_root.empty() && block_header.empty() && balance_unit.empty())) {
    fprintf(stderr, "error: --state-proofs <FILE_PATH> goes with exactly one of --state-root <0x + 64 hex> and --block-header "
                    "<0x-hex RLP | @FILE_PATH>, and they and --balance-unit wei|gwei|ether only with it\n"
                    "Usage: zkpoa-audit --anon-set <FILE_PATH> --vkey <FILE_PATH> --public <FILE_PATH> --proof <FILE_PATH> "
                    "[--commitment <64 hex>] [--state-proofs <FILE_PATH> (--state-root <0x + 64 hex> | --block-header <0x-hex RLP | "
                    "@FILE_PATH>) [--balance-unit wei|gwei|ether]]\n");
    return 2;
  }
  int rc = 2;
  try {
    uint8_t root32[32], block_hash[32];
    uint64_t block_number = 0, unit = 1;
    if (state) {
      if (balance_unit == "gwei") unit = 1000000000ull;
      else if (balance_unit == "ether") unit = 1000000000000000000ull;
      else if (!balance_unit.empty() && balance_unit != "wei") throw std::runtime_error("--balance-unit takes wei, gwei or ether");
      if (!state_root.empty()) {
        if (!parse_hex_bytes(Span{state_root.data(), state_root.data() + state_root.size()}, root32, 32))
          throw std::runtime_error("--state-root takes 0x and 64 hex digits");
      } else {
        std::string text = block_header[0] == '@' ? file_text(block_header.substr(1)) : block_header;
        const char *b = text.data(), *e = b + text.size();
        trim_span(b, e);
        if (e - b < 2 || b[0] != '0' || (b[1] | 32) != 'x' || (e - b) % 2) throw std::runtime_error("--block-header takes 0x-prefixed hex");
        std::vector<uint8_t> rlp((size_t)(e - b) / 2 - 1);
        for (size_t i = 0; i < rlp.size(); i++) {
          const int hi = hex_digit(b[2 + 2 * i]), lo = hex_digit(b[3 + 2 * i]);
          if (hi < 0 || lo < 0) throw std::runtime_error("--block-header takes 0x-prefixed hex");
          rlp[i] = (uint8_t)(16 * hi + lo);
        }
        if (zkpoa_eth_block_header(rlp.data(), rlp.size(), block_hash, root32, &block_number) != PROVER_OK)
          throw std::runtime_error("--block-header: not the RLP of a block header");
      }
    }
    uint8_t expected[32];
    if (!commitment.empty()) {
      const std::string pre = "0x" + commitment;
      if (!parse_hex_bytes(Span{pre.data(), pre.data() + pre.size()}, expected, 32))
        throw std::runtime_error("--commitment takes 64 hex digits");
    }
    ContextStart start(device_from_env());   // the device starts up while this thread reads the files
    const std::string vk_text = file_text(vkey), pub_text = file_text(pub), proof_text = file_text(proof);
    Limbs addr, bal;
    const double t0 = now_s();
    read_anonymity_set(anon, addr, bal);
    const double t_read = now_s();
    zkpoa_context* ctx = start.get();
    const double t_ctx = now_s();
    uint32_t failed = 0;
    zkpoa_assets_report rep;
    if (zkpoa_assets_verify(ctx, addr.data(), bal.data(), addr.rows, vk_text.c_str(), pub_text.c_str(), proof_text.c_str(),
                            commitment.empty() ? nullptr : expected, &failed, &rep) != PROVER_OK)
      throw std::runtime_error(zkpoa_last_error(ctx));
    zkpoa_state_report srep;
    if (state) {
      if (zkpoa_anon_set_state_check_file(ctx, addr.data(), bal.data(), addr.rows, state_proofs.c_str(), root32, unit, &srep) != PROVER_OK)
        throw std::runtime_error(zkpoa_last_error(ctx));
      if (srep.first_bad_row != ~0ull) failed |= ZKPOA_ASSETS_STATE;
    }
    if (verbose)
      fprintf(stderr, "zkpoa-audit: read %llu rows %.3f s, waited %.3f s more for the device, all checks (with the upload) %.3f s\n",
              (unsigned long long)rep.rows, t_read - t0, t_ctx - t_read, now_s() - t_ctx);
    if (state && !block_header.empty())
      printf("block: number %llu, hash 0x%s\n", (unsigned long long)block_number, hex32(block_hash).c_str());
    printf("rows: %llu%s\n", (unsigned long long)rep.rows, rep.ascending ? " (addresses strictly ascending)" : "");
    if (rep.duplicate_rows) {
      U256 a;
      memcpy(a.v, addr.data() + 4 * rep.first_dup[1], 32);
      uint8_t be[32];
      a.to_be(be);
      printf("duplicates: %llu rows repeat an earlier address; first: rows %llu and %llu, address 0x%s\n",
             (unsigned long long)rep.duplicate_rows, (unsigned long long)rep.first_dup[0], (unsigned long long)rep.first_dup[1],
             hex32(be).c_str() + 24);
    } else {
      printf("duplicates: %s\n", rep.rows ? "none" : "the set is empty");
    }
    if (state) {
      printf("state: %llu proven present, %llu proven absent, %llu without a proof, %llu with failed proofs, %llu with another balance; "
             "%llu proofs read, %llu for addresses not in the set",
             (unsigned long long)srep.proven_present, (unsigned long long)srep.proven_absent, (unsigned long long)srep.rows_without_proof,
             (unsigned long long)srep.rows_failed, (unsigned long long)srep.rows_differ, (unsigned long long)srep.proofs_read,
             (unsigned long long)srep.proofs_not_in_set);
      auto address_of = [&](uint64_t row) {
        U256 a;
        memcpy(a.v, addr.data() + 4 * row, 32);
        uint8_t be[32];
        a.to_be(be);
        return hex32(be).substr(24);
      };
      if (srep.first_bad_row != ~0ull && srep.first_bad_kind != ZKPOA_STATE_BAD_BALANCE) {
        static const char* names[10] = {"present", "absent", "no nodes", "a node's hash differs", "malformed RLP", "a bad child reference",
                                        "the proof ends early", "nodes after the end", "a bad hex-prefix", "no account"};
        if (srep.first_bad_kind == ZKPOA_STATE_BAD_NO_PROOF)
          printf("; first: row %llu, address 0x%s, no proof", (unsigned long long)srep.first_bad_row, address_of(srep.first_bad_row).c_str());
        else
          printf("; first: row %llu, address 0x%s, %s at node %u", (unsigned long long)srep.first_bad_row,
                 address_of(srep.first_bad_row).c_str(), srep.first_bad_status < 10 ? names[srep.first_bad_status] : "?", srep.first_bad_where);
      }
      if (srep.first_diff_row != ~0ull) {
        U256 csv;
        memcpy(csv.v, bal.data() + 4 * srep.first_diff_row, 32);
        printf("; first other balance: row %llu, address 0x%s, chain balance %s wei%s against csv balance %s %s",
               (unsigned long long)srep.first_diff_row, address_of(srep.first_diff_row).c_str(),
               U256::from_be(srep.first_diff_chain_balance32).dec().c_str(), srep.first_diff_absent ? " (proven absent)" : "",
               csv.dec().c_str(), balance_unit.empty() ? "wei" : balance_unit.c_str());
      }
      printf("\n");
    }
    printf("root: %s (%s public.json)\n", U256::from_le(rep.root_le).dec().c_str(),
           (failed & ZKPOA_ASSETS_ROOT) ? "DIFFERS from" : "as in");
    printf("commitment: %s (%s)\n", hex32(rep.commitment).c_str(),
           !(failed & ZKPOA_ASSETS_COMMITMENT) ? (commitment.empty() ? "a point of ed25519" : "as expected")
           : hex32(rep.commitment) == std::string(64, '0') ? "signals 0..11 are NO point of ed25519" : "DIFFERS from --commitment");
    printf("proof: %s\n", (failed & ZKPOA_ASSETS_PROOF) ? "Invalid proof" : "OK");
    if (!failed) {
      printf("AUDIT OK\n");
    } else {
      std::string names;
      if (failed & ZKPOA_ASSETS_SET) names += " set";
      if (failed & ZKPOA_ASSETS_STATE) names += " state";
      if (failed & ZKPOA_ASSETS_ROOT) names += " root";
      if (failed & ZKPOA_ASSETS_COMMITMENT) names += " commitment";
      if (failed & ZKPOA_ASSETS_PROOF) names += " proof";
      printf("AUDIT FAILED:%s\n", names.c_str());
    }
    rc = failed ? 1 : 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "Error: %s\n", e.what());
    rc = 2;
  }
  // the verdict is out (or the error is on stderr): leave without the HIP runtime's teardown, as `merkle-tree` does
  fflush(stdout);
  fflush(stderr);
  _exit(rc);
}
