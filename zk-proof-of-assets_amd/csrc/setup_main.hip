// `zkpoa-setup` -- the GPU stand-in for the reference's key-generation command (scripts/g16_setup.sh:243-252):
//     snarkjs zkey new      <circuit.r1cs> <pot.ptau> <circuit_0.zkey>
//     snarkjs groth16 setup <circuit.r1cs> <pot.ptau> <circuit_0.zkey>
//     snarkjs zkey contribute <circuit_0.zkey> <circuit_final.zkey> --name="..." -e="..."     (:262-266)
//     snarkjs zkey beacon <in.zkey> <out.zkey> <beaconHash(hex)> <numIterationsExp> -n="..."  (:269-278)
//     snarkjs wtns check <circuit.r1cs> <witness.wtns>                                      (scripts/g16_verify.sh:205-210)
//     snarkjs zkey verify <circuit.r1cs> <pot.ptau> <circuit_final.zkey>                    (scripts/g16_verify.sh -z)
//     snarkjs powersoftau verify <pot.ptau>              (the TODO at g16_setup.sh:201 and g16_verify.sh:164)
//     snarkjs powersoftau prepare phase2 <in.ptau> <out.ptau>     (what makes a ceremony file usable by the commands above)
//     snarkjs powersoftau new bn128 <power> <out.ptau>            (snarkjs README steps 1-4 and 6: the ceremony file itself,
//     snarkjs powersoftau contribute <in.ptau> <out.ptau>          which the reference downloads,
//     snarkjs powersoftau beacon <in> <out> <beaconHash(hex)> <numIterationsExp>   scripts/machine_initialization.sh:377-385)
//     snarkjs powersoftau export challenge <in.ptau> [challenge]                 (snarkjs README step 5: a contribution by
//     snarkjs powersoftau challenge contribute bn128 <challenge> [response]       somebody who never holds the ceremony
//     snarkjs powersoftau import response <old.ptau> <response> <new.ptau>        file)
// Same three file arguments (the words `zkey new` / `groth16 setup` are accepted and ignored, so the command line
// can be kept as it is with the executable swapped). The .ptau must be prepared for phase 2, as snarkjs requires too:
// `zkpoa-setup powersoftau prepare phase2` does that here. Exit status 0 / non-zero + message on stderr.
// The phase-2 transcript (section 10: circuit hash, contribution records; DESIGN.md "Phase-2 transcript") is opt-in:
// `zkey new ... --transcript` fills in the circuit hash; on such a key `zkey contribute` appends a record (--name= / -n=
// is kept in it), `zkey beacon` works, and `zkey verify` checks the hash and every record. Without the option every
// command writes and accepts what it did before. Acceptance of these keys by `snarkjs zkey verify` is not exercised.
// The phase-1 transcript (a .ptau's section 7; DESIGN.md "Phase-1 transcript") is written by `powersoftau contribute` and
// `powersoftau beacon` and checked by `powersoftau verify`. Acceptance of these files by `snarkjs powersoftau verify`
// is not exercised.
#include "../../include/zkpoa_prover.h"

#include "host_files.hpp"
#include "host_text.hpp"
#include "worker_exit.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

// the record lines of a .ptau's section 7 ("<type> <name> <response hash>\n" each), sized from the record count: a
// public ceremony's file holds scores of records with long names. Empty when the section cannot be read.
#include <string>
static std::string ptau_record_lines(const char* path, uint32_t* count) {
  *count = 0;
  if (zkpoa_ptau_contributions(path, count, nullptr, 0) != PROVER_OK || !*count) return std::string();
  std::string text((size_t)*count * (13 + 255 + 1 + 128 + 1) + 1, '\0');
  if (zkpoa_ptau_contributions(path, count, &text[0], (unsigned long)text.size()) != PROVER_OK) return std::string();
  text.resize(strlen(text.c_str()));
  return text;
}

// `zkey verify`: true when the key's delta2 equals its gamma2 (the generator, which the HEADER check holds it to): no
// contribution has been made, and whoever has the key can forge proofs with it
static bool delta2_is_gamma2(const char* zkey_path) {
  FILE* f = fopen(zkey_path, "rb");
  if (!f) return false;
  bool same = false;
  unsigned char hd[12];
  if (fread(hd, 1, 12, f) == 12) {
    uint32_t ns;
    memcpy(&ns, hd + 8, 4);
    for (uint32_t i = 0; i < ns; i++) {
      unsigned char sh[12];
      if (fread(sh, 1, 12, f) != 12) break;
      uint32_t type;
      uint64_t len;
      memcpy(&type, sh, 4);
      memcpy(&len, sh + 4, 8);
      if (type == 2) {
        unsigned char h[660];
        same = len == sizeof h && fread(h, 1, sizeof h, f) == sizeof h && !memcmp(h + 340, h + 532, 128);
        break;
      }
      if (fseeko(f, (off_t)len, SEEK_CUR) != 0) break;
    }
  }
  fclose(f);
  return same;
}

// The commands: the words that select one (a row with no words left over: the three file arguments alone are `zkey new`),
// its positional arguments, which of them names the file it writes (-1: none), whether it runs in a worker process
// (csrc/worker_exit.hpp), whether its last two positionals are a beacon's hex bytes and exponent, and the default of a
// last positional that may be left out.
enum Cmd { kZkeyNew, kZkeyContribute, kZkeyBeacon, kZkeyVerify, kWtnsCheck, kPtauVerify, kPtauPrepare, kPtauNew, kPtauContribute, kPtauBeacon,
           kPtauExport, kPtauChallengeContribute, kPtauImport };
struct Command {
  Cmd cmd;
  const char* words[3];
  int npos, out_pos;
  bool worker, beacon;
  const char* last_default = nullptr;
};
static const Command kCommands[] = {
    {kZkeyBeacon, {"zkey", "beacon"}, 4, 1, true, true},
    {kZkeyContribute, {"zkey", "contribute"}, 2, 1, true, false},
    {kZkeyVerify, {"zkey", "verify"}, 3, -1, false, false},
    {kPtauVerify, {"powersoftau", "verify"}, 1, -1, false, false},
    {kPtauPrepare, {"powersoftau", "prepare", "phase2"}, 2, 1, false, false},
    {kPtauNew, {"powersoftau", "new"}, 3, 2, false, false},
    {kPtauContribute, {"powersoftau", "contribute"}, 2, 1, false, false},
    {kPtauBeacon, {"powersoftau", "beacon"}, 4, 1, false, true},   // the same beacon arguments as `zkey beacon`
    {kPtauExport, {"powersoftau", "export", "challenge"}, 2, 1, false, false, "challenge"},
    {kPtauChallengeContribute, {"powersoftau", "challenge", "contribute"}, 3, 2, false, false, "response"},
    {kPtauImport, {"powersoftau", "import", "response"}, 3, 2, false, false},
    {kWtnsCheck, {"wtns", "check"}, 2, -1, false, false},
    {kZkeyNew, {"zkey", "new"}, 3, 2, true, false},
    {kZkeyNew, {"groth16", "setup"}, 3, 2, true, false},
    {kZkeyNew, {}, 3, 2, true, false}};

int main(int argc, char** argv) {
  int a = 1;
  const Command* c = kCommands;
  for (;; c++) {
    int w = 0;
    while (w < 3 && c->words[w] && a + w < argc && !strcmp(argv[a + w], c->words[w])) w++;
    if (w == 3 || !c->words[w]) {   // every word of the row matched
      a += w;
      break;
    }
  }
  const Cmd cmd = c->cmd;
  // snarkjs' options: --name=... / -n=... goes into the contribution record when the key carries a transcript; the
  // others (-e=..., -v) are accepted and ignored: the entropy text only feeds snarkjs' own random generator, the secret
  // here comes from /dev/urandom (or ZKPOA_DELTA). --transcript (`zkey new`) is this tool's own.
  const char* pos[4] = {nullptr, nullptr, nullptr, nullptr};
  const char* name = nullptr;
  bool transcript = false;
  int npos = 0;
  for (int i = a; i < argc; i++) {
    if (argv[i][0] == '-' && argv[i][1]) {
      if (!strncmp(argv[i], "--name=", 7)) name = argv[i] + 7;
      else if (!strncmp(argv[i], "-n=", 3)) name = argv[i] + 3;
      else if (!strcmp(argv[i], "--transcript")) transcript = true;
      continue;
    }
    if (npos < 4) pos[npos] = argv[i];
    npos++;
  }
  if (c->last_default && npos == c->npos - 1) pos[npos++] = c->last_default;
  if (npos != c->npos) {
    fprintf(stderr, "usage: zkpoa-setup [zkey new | groth16 setup] <circuit.r1cs> <pot.ptau> <circuit_0.zkey>\n"
                    "         [--transcript]   fill in section 10's circuit hash (needs the ptau's section 2)\n"
                    "       zkpoa-setup zkey contribute <in.zkey> <out.zkey> [--name=...] [-e=...]\n"
                    "       zkpoa-setup zkey beacon <in.zkey> <out.zkey> <beaconHash(hex)> <numIterationsExp> [-n=...]\n"
                    "       zkpoa-setup wtns check <circuit.r1cs> <witness.wtns>\n"
                    "       zkpoa-setup zkey verify <circuit.r1cs> <pot.ptau> <circuit.zkey>\n"
                    "       zkpoa-setup powersoftau verify <pot.ptau>\n"
                    "       zkpoa-setup powersoftau prepare phase2 <in.ptau> <out.ptau>\n"
                    "       zkpoa-setup powersoftau new bn128 <power> <out.ptau>\n"
                    "       zkpoa-setup powersoftau contribute <in.ptau> <out.ptau> [--name=...]\n"
                    "         (-e=<entropy> is accepted and ignored: the secrets come from /dev/urandom)\n"
                    "       zkpoa-setup powersoftau beacon <in.ptau> <out.ptau> <beaconHash(hex)> <numIterationsExp> [--name=...]\n"
                    "       zkpoa-setup powersoftau export challenge <in.ptau> [challenge]\n"
                    "       zkpoa-setup powersoftau challenge contribute bn128 <challenge> [response]\n"
                    "         (--name=... and -e=... are accepted and ignored)\n"
                    "       zkpoa-setup powersoftau import response <old.ptau> <response> <new.ptau> [--name=...]\n");
    return 2;
  }
  if (cmd == kPtauChallengeContribute && strcmp(pos[0], "bn128") && strcmp(pos[0], "bn254")) {
    fprintf(stderr, "zkpoa-setup: powersoftau challenge contribute: the curve must be bn128\n");
    return 2;
  }
  unsigned new_power = 0;
  if (cmd == kPtauNew) {
    char* end = nullptr;
    const long v = strtol(pos[1], &end, 10);
    if ((strcmp(pos[0], "bn128") && strcmp(pos[0], "bn254")) || end == pos[1] || *end || v < 1 || v > 28) {
      fprintf(stderr, "zkpoa-setup: powersoftau new: the curve must be bn128 and the power in [1, 28]\n");
      return 2;
    }
    new_power = (unsigned)v;
  }
  uint8_t delta[32];
  const uint8_t* delta_p = nullptr;
  if (const char* e = cmd == kZkeyContribute ? zkpoa::opt_text(zkpoa::O_DELTA) : nullptr) {   // tests / reproducible keys only: the secret must not be kept
    zkpoa::U256 d;
    if (!d.parse_number(e, e + strlen(e))) {
      fprintf(stderr, "zkpoa-setup: ZKPOA_DELTA is not a number below 2^256\n");
      return 2;
    }
    fprintf(stderr, "zkpoa-setup: WARNING: delta taken from ZKPOA_DELTA -- whoever knows it can forge proofs for this key\n");
    d.to_le(delta);
    delta_p = delta;
  }
  // `zkey new` / `zkey contribute` run in a worker process and this one leaves as soon as the key is renamed into place
  // (csrc/worker_exit.hpp: a worker that has held ~100 GB of host arrays takes seconds to be dismantled).
  // (`wtns check`, `zkey verify` and `powersoftau verify` write nothing and use no worker; `powersoftau prepare phase2`
  // runs in this process too)
  // beacon: hex bytes and the exponent (at most 30: 2^30 hashes take minutes, more would not finish)
  uint8_t beacon_bytes[255];
  unsigned long beacon_len = 0;
  unsigned beacon_exp = 0;
  if (c->beacon) {
    const char* h = pos[2];
    if (h[0] == '0' && (h[1] == 'x' || h[1] == 'X')) h += 2;
    const size_t hl = strlen(h);
    bool ok = hl > 0 && hl % 2 == 0 && hl / 2 <= sizeof beacon_bytes;
    for (size_t i = 0; ok && i < hl; i++) {
      const char c = h[i];
      const int v = c >= '0' && c <= '9' ? c - '0' : ((c | 32) >= 'a' && (c | 32) <= 'f' ? (c | 32) - 'a' + 10 : -1);
      if (v < 0) ok = false;
      else beacon_bytes[i / 2] = (uint8_t)(i % 2 ? (beacon_bytes[i / 2] | v) : v << 4);
    }
    char* end = nullptr;
    const long e = strtol(pos[3], &end, 10);
    if (!ok || end == pos[3] || *end || e < 0 || e > 30) {
      fprintf(stderr, "zkpoa-setup: %s beacon: the beacon must be 1-255 bytes of hex and numIterationsExp in [0, 30]\n", cmd == kPtauBeacon ? "powersoftau" : "zkey");
      return 2;
    }
    beacon_len = hl / 2;
    beacon_exp = (unsigned)e;
  }
  // does the input of `zkey contribute` carry a transcript? (host only; an unreadable file is reported by the command)
  bool in_transcript = false;
  if (cmd == kZkeyContribute) {
    int has = 0;
    uint32_t cnt = 0;
    if (zkpoa_zkey_contributions(pos[0], &has, &cnt, nullptr, 0) == PROVER_OK) in_transcript = has != 0;
  }
  zkpoa::WorkerExit we = zkpoa::WorkerExit::start(c->worker, "zkpoa-setup");
  if (we.is_worker()) zkpoa_setup_defer_host_frees(1);
  auto leave = [&](int code) -> int {
    if (we.is_worker()) we.leave(code);
    return code;
  };
  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  zkpoa_context* ctx = nullptr;
  char err[512] = {0};
  int rc = PROVER_ERROR;
  try {
    rc = zkpoa_context_create(zkpoa::device_from_env(), &ctx, err, sizeof err);
  } catch (const zkpoa::OptionError& e) {
    snprintf(err, sizeof err, "%s", e.what());
  }
  if (rc != PROVER_OK) {
    fprintf(stderr, "zkpoa-setup: %s\n", err);
    return leave(1);
  }
  if (cmd == kWtnsCheck) {   // snarkjs prints "WITNESS IS CORRECT" and exits 0, or names the failure and exits 1
    uint64_t bad = 0, first = 0;
    rc = zkpoa_wtns_check(ctx, pos[0], pos[1], &bad, &first);
    if (rc == PROVER_OK && bad == 0) printf("[INFO]  zkpoa: WITNESS IS CORRECT\n");
    if (rc == PROVER_OK && bad) {
      fprintf(stderr, "[ERROR] zkpoa: WITNESS CHECK FAILED: %llu constraint(s) do not hold, the first is #%llu\n",
              (unsigned long long)bad, (unsigned long long)first);
      zkpoa_context_destroy(ctx);
      return 1;
    }
  } else if (cmd == kZkeyVerify) {   // snarkjs prints "ZKey Ok!" and exits 0, or names what does not match and exits 1
    uint32_t failed = 0;
    rc = zkpoa_zkey_verify(ctx, pos[0], pos[1], pos[2], &failed);
    if (rc == PROVER_OK) {
      static const char* const kWhat[10] = {
          "HEADER: protocol, moduli, alpha1 / beta1 / beta2 (against the ptau) or gamma2 (the G2 generator) do not match",
          "POINTS: a point is off its curve, a G2 point (B2, beta2, gamma2, delta2) is outside G2, or delta1 is zero",
          "DELTA: e(delta1, G2) != e(G1, delta2)",
          "COEFFS: section 4 (coefficients) does not match the r1cs",
          "A: section 5 (A) does not match the r1cs and the ptau",
          "B1: section 6 (B in G1) does not match the r1cs and the ptau",
          "B2: section 7 (B in G2) does not match the r1cs and the ptau",
          "ICCH: sections 3, 8 or 9 (IC, C, H) do not match the r1cs, the ptau and delta",
          "CSHASH: section 10's circuit hash does not match the r1cs, the ptau and the key's A, B1, B2, IC",
          "CONTRIBUTIONS: a contribution record does not verify (transcript hash, pairing checks, beacon) or the "
          "records do not lead to delta1"};
      int has_transcript = 0;
      uint32_t n_records = 0;
      static char records[1 << 16];
      records[0] = 0;
      (void)zkpoa_zkey_contributions(pos[2], &has_transcript, &n_records, records, sizeof records);
      if (!has_transcript) fprintf(stderr, "[WARN]  zkpoa: section 10 (circuit hash, contribution records) is not checked: the key carries no transcript\n");
      for (int b = 0; b < 10; b++)
        if (failed & (1u << b)) fprintf(stderr, "[ERROR] zkpoa: %s\n", kWhat[b]);
      if (failed) {
        zkpoa_context_destroy(ctx);
        return 1;
      }
      if (delta2_is_gamma2(pos[2]))
        fprintf(stderr, "[WARN]  zkpoa: delta2 is the generator: the key has had no contribution, anyone can forge proofs with it\n");
      if (has_transcript) {
        printf("[INFO]  zkpoa: circuit hash and %u contribution(s) verified\n", n_records);
        unsigned k = 1;
        for (char* line = strtok(records, "\n"); line; line = strtok(nullptr, "\n"), k++)
          printf("[INFO]  zkpoa: contribution #%u: %s\n", k, line);
      }
      printf("[INFO]  zkpoa: ZKey Ok!\n");
    }
  } else if (cmd == kPtauVerify) {   // snarkjs prints "Powers of Tau Ok!" and exits 0, or names what does not hold and exits 1
    uint32_t failed = 0, info[4] = {0, 0, 0, 0};
    rc = zkpoa_ptau_verify(ctx, pos[0], 0, &failed, info);
    if (rc == PROVER_OK) {
      static const char* const kWhat[10] = {
          "POINTS: a point is off its curve, a G2 point (section 3, beta2, section 13) is outside G2, T_0 or U_0 is not "
          "the generator, or T_1, A_0, B_0 or beta2 is zero",
          "TAU_G1: section 2 (tau^i G1) is not one chain of powers of the tau of U_1",
          "TAU_G2: section 3 (tau^i G2) is not one chain of powers of the tau of T_1",
          "ALPHA: section 4 (alpha tau^i G1) is not one chain of powers of tau",
          "BETA: section 5 (beta tau^i G1) is not one chain of powers of tau, or beta2 does not match it",
          "LAGRANGE_TAU_G1: section 12 (Lagrange form of tau G1) does not agree with section 2",
          "LAGRANGE_TAU_G2: section 13 (Lagrange form of tau G2) does not agree with section 3",
          "LAGRANGE_ALPHA: section 14 (Lagrange form of alpha tau G1) does not agree with section 4",
          "LAGRANGE_BETA: section 15 (Lagrange form of beta tau G1) does not agree with section 5",
          "CONTRIBUTIONS: a record of section 7 does not verify (key, ratios, beacon) or the records do not lead to this "
          "file's points and challenge"};
      uint32_t n_records = 0;
      std::string records = ptau_record_lines(pos[0], &n_records);
      if (!info[3])
        fprintf(stderr, "[WARN]  zkpoa: section 7 holds no contribution record: the powers carry no trail of who made them\n");
      if (!info[2])
        fprintf(stderr, "[WARN]  zkpoa: the file is not prepared for phase 2 (no sections 12-15): only the powers were checked\n");
      for (int b = 0; b < 10; b++)
        if (failed & (1u << b)) fprintf(stderr, "[ERROR] zkpoa: %s\n", kWhat[b]);
      if (failed) {
        zkpoa_context_destroy(ctx);
        return 1;
      }
      unsigned k = 1;   // one line per record: "contribution <name> <response hash>" or "beacon <name> <response hash>"
      for (char* line = strtok(&records[0], "\n"); line; line = strtok(nullptr, "\n"), k++)
        printf("[INFO]  zkpoa: contribution #%u: %s\n", k, line);
      printf("[INFO]  zkpoa: Powers of Tau Ok!\n");
    }
  } else if (cmd == kPtauPrepare) {   // snarkjs logs its progress and exits 0, or names what is wrong with the file and exits 1
    uint32_t info[4] = {0, 0, 0, 0};
    rc = zkpoa_ptau_prepare_phase2(ctx, pos[0], pos[1], info);
    if (rc == PROVER_OK) printf("[INFO]  zkpoa: Prepared phase 2\n");
  } else if (cmd == kPtauNew) {
    rc = zkpoa_ptau_new(ctx, new_power, pos[2]);
    if (rc == PROVER_OK) printf("[INFO]  zkpoa: new ceremony file of power %u\n", new_power);
  } else if (cmd == kPtauExport || cmd == kPtauChallengeContribute) {   // snarkjs logs the hash of the file it wrote
    uint8_t h[64];
    if (cmd == kPtauExport) rc = zkpoa_ptau_export_challenge(ctx, pos[0], pos[1], h);
    else rc = zkpoa_ptau_challenge_contribute(ctx, pos[1], pos[2], nullptr, h);
    if (rc == PROVER_OK) {
      char hex[129];
      for (int i = 0; i < 64; i++) snprintf(hex + 2 * i, 3, "%02x", h[i]);
      printf("[INFO]  zkpoa: %s hash: %s\n", cmd == kPtauExport ? "challenge" : "response", hex);
    }
  } else if (cmd == kPtauContribute || cmd == kPtauBeacon || cmd == kPtauImport) {
    if (cmd == kPtauBeacon) rc = zkpoa_ptau_beacon(ctx, pos[0], pos[1], beacon_bytes, beacon_len, beacon_exp, name);
    else if (cmd == kPtauImport) rc = zkpoa_ptau_import_response(ctx, pos[0], pos[1], pos[2], name);
    else rc = zkpoa_ptau_contribute(ctx, pos[0], pos[1], nullptr, name);
    if (rc == PROVER_OK) {
      uint32_t n_records = 0;
      const std::string records = ptau_record_lines(pos[c->out_pos], &n_records);
      size_t last = records.size() > 1 ? records.rfind('\n', records.size() - 2) : std::string::npos;   // the record just written
      last = last == std::string::npos ? 0 : last + 1;
      printf("[INFO]  zkpoa: contribution #%u: %s", n_records, records.empty() ? "\n" : records.c_str() + last);
    }
  } else {
    if (cmd == kZkeyBeacon) rc = zkpoa_zkey_beacon(ctx, pos[0], pos[1], beacon_bytes, beacon_len, beacon_exp, name);
    else if (cmd == kZkeyContribute && in_transcript) rc = zkpoa_zkey_contribute_ex(ctx, pos[0], pos[1], delta_p, name);
    else if (cmd == kZkeyContribute) rc = zkpoa_zkey_contribute(ctx, pos[0], pos[1], delta_p);
    else rc = zkpoa_zkey_new_ex(ctx, pos[0], pos[1], pos[2], transcript ? ZKPOA_SETUP_TRANSCRIPT : 0u);
  }
  if (rc != PROVER_OK) fprintf(stderr, "zkpoa-setup: %s\n", zkpoa_last_error(ctx));
  if (!we.is_worker()) zkpoa_context_destroy(ctx);
  clock_gettime(CLOCK_MONOTONIC, &t1);
  if (rc == PROVER_OK && c->out_pos >= 0)
    zkpoa::vlog("zkpoa-setup: %s written in %.2f s\n", pos[c->out_pos], (t1.tv_sec - t0.tv_sec) + (t1.tv_nsec - t0.tv_nsec) / 1e9);
  return leave(rc == PROVER_OK ? 0 : 1);
}
