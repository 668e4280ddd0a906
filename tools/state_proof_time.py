"""Time the state-proof check (include/zkpoa_state_proof.h) on the GPU. A measurement input only: the trie is built level
by level with the device's own batched zkpoa_keccak256, which no test does.

The trie is the complete 16-ary one over 2^20 raw keys, one per 5-nibble prefix: every branch is 532 bytes, a proof is
five branches and a leaf. Timed, as the median of three runs after a warm one:
  kernels   zkpoa_mpt_verify over --proofs proofs: zkpoa_last_ms id 8 (the hash, walk kernels), and the wall clock
  hashing   the byte-wise zkpoa_keccak256 over as many 532-byte messages as those proofs hold branches, wall clock; the two
            kernels alone are compared under `rocprofv3 --kernel-trace --stats -- python tools/state_proof_time.py --compare`,
            whose table lists keccak256_kernel and mpt_hash_kernel side by side
  command   zkpoa-audit --state-proofs over a file of --file-proofs proofs (rows = those addresses), ZKPOA_VERBOSE's split

    python tools/state_proof_time.py [--proofs 131072] [--file-proofs 32768] [--compare] [--out profiles/state_proof_time.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

LEVELS = 5


def build_trie(ctx, rng):
    """-> (levels: [branch arrays (16^d, 532) for d = 0..4], leaves (2^20, L), keys (2^20, 32), root)"""
    n = 16 ** LEVELS
    keys = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    idx = np.arange(n, dtype=np.uint32)
    keys[:, 0] = idx >> 12
    keys[:, 1] = (idx >> 4) & 0xff
    keys[:, 2] = ((idx & 15) << 4) | (keys[:, 2] & 15)
    # leaf: list [hex-prefix of the remaining 59 nibbles (odd: flag 3), a 44-byte value]
    path = np.empty((n, 30), dtype=np.uint8)
    path[:, 0] = 0x30 | (keys[:, 2] & 15)
    path[:, 1:] = keys[:, 3:]
    value = np.full((n, 44), 0x76, dtype=np.uint8)
    value[:, :4] = idx.view(np.uint8).reshape(n, 4)
    leaf = np.concatenate([np.full((n, 1), 0xf8, np.uint8), np.full((n, 1), 31 + 45, np.uint8), np.full((n, 1), 0x80 + 30, np.uint8), path,
                           np.full((n, 1), 0x80 + 44, np.uint8), value], axis=1)
    digests = np.frombuffer(ctx.keccak256(leaf.tobytes(), leaf.shape[1]), dtype=np.uint8).reshape(n, 32)
    levels = []
    for d in range(LEVELS - 1, -1, -1):
        nb = 16 ** d
        node = np.empty((nb, 532), dtype=np.uint8)
        node[:, 0:3] = (0xf9, 0x02, 0x11)
        body = node[:, 3:531].reshape(nb, 16, 33)
        body[:, :, 0] = 0xa0
        body[:, :, 1:] = digests.reshape(nb, 16, 32)
        node[:, 531] = 0x80
        digests = np.frombuffer(ctx.keccak256(node.tobytes(), 532), dtype=np.uint8).reshape(nb, 32)
        levels.insert(0, node)
    return levels, leaf, keys, digests[0].tobytes()


def proofs_of(levels, leaf, m):
    """The first m keys' proofs in the C ABI's layout (every node copied per proof, as a file of proofs holds them)"""
    per = LEVELS * 536 + ((leaf.shape[1] + 7) & ~7)
    blob = np.zeros((m, per), dtype=np.uint8)
    idx = np.arange(m)
    for d in range(LEVELS):
        blob[:, 536 * d:536 * d + 532] = levels[d][idx >> (4 * (LEVELS - d))]
    blob[:, 536 * LEVELS:536 * LEVELS + leaf.shape[1]] = leaf[:m]
    offsets = (idx[:, None] * per + np.arange(LEVELS + 1)[None, :] * 536).astype(np.uint64).reshape(-1)
    lengths = np.tile(np.array([532] * LEVELS + [leaf.shape[1]], dtype=np.uint32), m)
    first = (np.arange(m + 1) * (LEVELS + 1)).astype(np.uint64)
    return blob.reshape(-1), offsets, lengths, first


def median3(fn):
    fn()
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        extra = fn()
        runs.append((time.perf_counter() - t0, extra))
    return statistics.median(r[0] for r in runs), statistics.median(r[1] for r in runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proofs", type=int, default=1 << 17)
    ap.add_argument("--file-proofs", type=int, default=1 << 15)
    ap.add_argument("--compare", action="store_true", help="only the two hashing runs (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    zk = entry.load_package()
    ctx = zk.Context(0)
    rng = np.random.default_rng(20)
    t0 = time.perf_counter()
    levels, leaf, keys, root = build_trie(ctx, rng)
    lines = ["state proof timing (builder-run): complete 16-ary trie over 2^20 keys built in %.1f s; a proof = %d branches of 532 B + a "
             "leaf of %d B" % (time.perf_counter() - t0, LEVELS, leaf.shape[1])]
    m = args.proofs
    blob, offsets, lengths, first = proofs_of(levels, leaf, m)
    blob_bytes, key_bytes = blob.tobytes(), keys[:m].tobytes()
    perms = m * (LEVELS * 4 + 1)

    def verify():
        status, _, _ = ctx.mpt_verify(key_bytes, root, blob_bytes, offsets, lengths, first)
        assert status == bytes(m), "a proof of the timing trie did not verify"
        return ctx.last_ms(8)
    wall, kernel_ms = median3(verify)
    lines.append("kernels: zkpoa_mpt_verify, %d proofs (%d nodes, %.0f MB, %d permutations): kernels %.2f ms (%.2f G permutations/s, hash "
                 "and walk together), call %.0f ms with the upload" % (m, m * (LEVELS + 1), len(blob_bytes) / 1e6, perms, kernel_ms,
                                                                      perms / kernel_ms / 1e6, wall * 1e3))
    msgs = np.ascontiguousarray(blob.reshape(m, -1)[:, :536 * LEVELS].reshape(m * LEVELS, 536)[:, :532]).tobytes()
    wall_b, _ = median3(lambda: len(ctx.keccak256(msgs, 532)))
    lines.append("hashing: byte-wise zkpoa_keccak256, %d messages of 532 B (%d permutations): call %.0f ms with the upload (no kernel slot: "
                 "compare the kernels under a kernel trace, --compare)" % (m * LEVELS, m * LEVELS * 4, wall_b * 1e3))
    if not args.compare:
        fm = min(args.file_proofs, m)
        with tempfile.TemporaryDirectory() as tmp:
            proofs_path, csv_path = os.path.join(tmp, "proofs.jsonl"), os.path.join(tmp, "set.csv")
            per = blob.size // m
            rows = blob.reshape(m, per)
            with open(proofs_path, "w") as f, open(csv_path, "w") as c:
                c.write("address,eth_balance\n")
                for i in range(fm):
                    address = keys[i, :20].tobytes().hex()
                    nodes = ['"0x%s"' % rows[i, 536 * d:536 * d + 532].tobytes().hex() for d in range(LEVELS)]
                    nodes.append('"0x%s"' % rows[i, 536 * LEVELS:536 * LEVELS + leaf.shape[1]].tobytes().hex())
                    f.write('{"address":"0x%s","balance":"0x0","accountProof":[%s],"storageProof":[]}\n' % (address, ",".join(nodes)))
                    c.write("0x%s,0\n" % address)
            size = os.path.getsize(proofs_path)
            golden = os.path.join(ROOT, "tests", "golden", "ref")
            run_dir = os.path.join(golden, "1_sigs_1_batches_5_height__layer_three")
            argv = [zk.AUDIT_BIN, "--anon-set", csv_path, "--vkey", os.path.join(golden, "layer_three_vkey.json"), "--public",
                    os.path.join(run_dir, "public.json"), "--proof", os.path.join(run_dir, "proof.json"), "--state-proofs", proofs_path,
                    "--state-root", "0x" + root.hex()]
            # The command hashes each address into its key, and these keys have no known preimages: the walks leave the
            # proofs at node 1 and the state check reports failed proofs. Reading, upload and the hashing of every node,
            # which is nearly all of the device work, are those of a file of good proofs.
            runs = []
            for _ in range(4):
                t0 = time.perf_counter()
                rc = subprocess.run(argv, capture_output=True, text=True, env=dict(os.environ, ZKPOA_VERBOSE="1"))
                runs.append((time.perf_counter() - t0, rc))
            wall_c = statistics.median(r[0] for r in runs[1:])
            split = [l for l in runs[-1][1].stderr.splitlines() if "state check" in l]
            state = [l for l in runs[-1][1].stdout.splitlines() if l.startswith("state:")]
            lines.append("command: zkpoa-audit --state-proofs, %d proofs in %.0f MB of JSON Lines: file to verdict %.2f s" % (fm, size / 1e6, wall_c))
            lines += ["  " + l for l in split + state]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
