"""Wall time of `ecdsa-sigs-parser layer-two-input` for one batch out of a large run (host only, no GPU):
a synthetic parsed-signatures file and merkle_proofs.json of 2^16 entries in the shapes the two commands before it write
(every field of an attestation present, sibling paths of 16 hashes), batch [1024, 1536). One warm run, then three;
prints each wall time, the median and the phases ZKPOA_VERBOSE reports for the median run.

    python tools/layer_two_time.py [log2 entries] [batch size] > profiles/layer_two_input_time.txt
"""
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "zk-proof-of-assets_amd", "ecdsa-sigs-parser")
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def big(v, indent):
    return '{\n%s  "__bigint__": "%d"\n%s}' % (indent, v, indent)


def main():
    log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    batch = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    n, depth, rng = 1 << log_n, 16, random.Random(1)
    with tempfile.TemporaryDirectory() as d:
        parsed, proofs, root = (os.path.join(d, f) for f in ("parsed.json", "merkle_proofs.json", "merkle_root.json"))
        with open(parsed, "w") as f:
            f.write('{\n  "accountAttestations": [\n')
            for i in range(n):
                sig = ",\n".join('        "%s": %s' % (k, big(rng.getrandbits(256), "        ")) for k in ("r", "s", "r_prime"))
                key = ",\n".join('          "%s": %s' % (k, big(rng.getrandbits(256), "          ")) for k in ("x", "y"))
                msg = ",\n".join("            %d" % rng.randrange(256) for _ in range(32))
                f.write('    {\n      "signature": {\n%s,\n        "pubkey": {\n%s\n        },\n        "msghash": {\n'
                        '          "__uint8array__": [\n%s\n          ]\n        }\n      },\n      "accountData": {\n'
                        '        "address": %s,\n        "balance": %s\n      }\n    }%s\n'
                        % (sig, key, msg, big((i + 1) << 100, "        "), big(rng.randrange(10 ** 6), "        "), "," if i + 1 < n else ""))
            f.write("  ]\n}")
        with open(proofs, "w") as f:
            f.write('{\n  "leaves": [\n' + ",\n".join(
                '    {\n      "address": %s,\n      "balance": %s,\n      "hash": %s\n    }'
                % (big((i + 1) << 100, "      "), big(1, "      "), big(rng.randrange(R), "      ")) for i in range(n)))
            f.write('\n  ],\n  "path_elements": [\n' + ",\n".join(
                "    [\n" + ",\n".join("      " + big(rng.randrange(R), "      ") for _ in range(depth)) + "\n    ]" for _ in range(n)))
            f.write('\n  ],\n  "path_indices": [\n' + ",\n".join(
                "    [\n" + ",\n".join("      %d" % rng.randrange(2) for _ in range(depth)) + "\n    ]" for _ in range(n)))
            f.write("\n  ]\n}")
        with open(root, "w") as f:
            f.write(big(12345, ""))
        proof = os.path.join(ROOT, "tests", "golden", "ref", "1_sigs_1_batches_5_height__layer_one__batch_0", "sanitized_proof.json")
        argv = [BIN, "layer-two-input", "-i", parsed, "-t", root, "-p", proofs, "-h", os.path.join(d, "hash.txt"), "-d", proof,
                "-o", os.path.join(d, "out.json"), "-s", "1024", "-e", str(1024 + batch)]
        print("layer-two-input, batch [1024, %d) of 2^%d entries: parsed file %.1f MB, merkle_proofs.json %.1f MB (tmpfs or page cache)"
              % (1024 + batch, log_n, os.path.getsize(parsed) / 1e6, os.path.getsize(proofs) / 1e6))
        runs = []
        for k in range(4):
            t0 = time.perf_counter()
            rc = subprocess.run(argv, env=dict(os.environ, ZKPOA_VERBOSE="1"), capture_output=True, text=True)
            dt = time.perf_counter() - t0
            assert rc.returncode == 0, rc.stderr
            if k:
                runs.append((dt, rc.stderr))
                print("run %d: %.3f s" % (k, dt))
        runs.sort()
        print("median %.3f s; its phases:" % runs[1][0])
        print(runs[1][1].rstrip())


if __name__ == "__main__":
    main()
