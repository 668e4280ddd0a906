"""File-to-verdict time of the `zkpoa-audit` executable on a 10 M-line anonymity set, `merkle-tree` on the same file beside
it, and the index kernels alone (zkpoa_last_ms id 9) on four key shapes -- random, all equal, 31 shared bytes, real-shaped
160-bit -- against the device-to-device copy bandwidth measured in the same run.
  python tools/audit_time.py [--rows 10000000] [--dir /dev/shm]
The proof files are the reference's committed 4_sigs layer-three run: its root is not this set's, so the verdict is
"AUDIT FAILED: root" (exit 1) with every check run -- the time is that of a passing audit."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# Bytes one pass moves per row, by count (csrc/anon_set_sort.hip.h). The count kernel reads the row number (4 B) and one
# byte of the key; the scatter kernel reads both again and writes the row number (4 B). The (digit, tile) table is 256
# words per tile of 2048 rows, written once, read twice and written once by the three scan kernels, read once by the scatter:
# 5 x 4 x 256 / 2048 = 2.5 B per row.
NEEDED_PER_ROW = 4 + 1 + 4 + 1 + 4 + 2.5
# what the memory system has to fetch when every gathered key byte costs a 32-byte sector of its own
SECTOR_PER_ROW = 4 + 32 + 4 + 32 + 4 + 2.5


def write_csv(path, rows):
    import numpy as np
    nr = np.random.default_rng(7)
    owned = {}
    with open(path, "w") as f:
        f.write("address,eth_balance\n")
        step = 1 << 18
        for lo in range(0, rows, step):
            cnt = min(step, rows - lo)
            hi64 = nr.integers(0, 1 << 63, size=(cnt, 3), dtype=np.uint64)
            bal = nr.integers(0, 1 << 62, size=cnt, dtype=np.uint64)
            out = []
            for i in range(cnt):
                a = ((int(hi64[i, 0]) << 96) | (int(hi64[i, 1]) << 33) | int(hi64[i, 2] >> 30)) & ((1 << 160) - 1)
                out.append("0x%040x,%d\n" % (a, int(bal[i])))
                if (lo + i) in (5, rows // 2, rows - 1):
                    owned[lo + i] = (a, int(bal[i]))
            f.write("".join(out))
    return {"accountAttestations": [{"accountData": {"address": {"__bigint__": str(a)}, "balance": {"__bigint__": str(b)}}}
                                    for _, (a, b) in sorted(owned.items())]}


def copy_bandwidth(torch):
    """Device-to-device copy of 1 GiB, read + written bytes over the best of five event-timed copies, in GB/s."""
    x = torch.empty(1 << 30, dtype=torch.uint8, device="cuda").random_(0, 255)
    y = torch.empty_like(x)
    y.copy_(x)
    best = None
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        y.copy_(x)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None else min(best, ms)
    return 2 * (1 << 30) / (best * 1e-3) / 1e9


def index_kernels(z, torch, rows):
    ctx = z.Context(0)
    gbs = copy_bandwidth(torch)
    print("device-to-device copy, 1 GiB, best of 5: %.0f GB/s (read + written bytes)" % gbs, flush=True)
    g = torch.Generator(device="cuda").manual_seed(11)

    def rand_bytes(width):
        k = torch.zeros((rows, 32), dtype=torch.uint8, device="cuda")
        k[:, :width] = torch.randint(0, 256, (rows, width), dtype=torch.uint8, device="cuda", generator=g)
        return k
    base = torch.arange(1, 33, dtype=torch.uint8, device="cuda").repeat(rows, 1)
    shared31 = base.clone()
    shared31[:, 0] = torch.randint(0, 256, (rows,), dtype=torch.uint8, device="cuda", generator=g)
    rnd = rand_bytes(32)
    rnd[:, 31] &= 0x1f                                                   # below r
    shapes = [("random below 2^253 (32 passes)", rnd), ("all equal (0 passes)", base), ("31 shared bytes (1 pass)", shared31),
              ("real-shaped 160-bit (20 passes)", rand_bytes(20))]
    perm = torch.empty(rows, dtype=torch.int32, device="cuda")
    for name, keys in shapes:
        torch.cuda.synchronize()
        ms = []
        for _ in range(4):
            ctx.anon_set_index(keys.data_ptr(), rows, perm.data_ptr())
            ms.append(ctx.last_ms(9))
        passes = int(name.split("(")[1].split()[0])
        best = min(ms[1:])
        line = "index kernels (id 9), %d rows, %s: %s ms -> best after warm-up %.2f ms" % (
            rows, name, " ".join("%.2f" % m for m in ms), best)
        if passes:
            line += "; %.2f ms per pass; by count %.1f B per row and pass needed = %.0f GB/s, %.1f B with a 32-B sector per " \
                    "gathered digit = %.0f GB/s = %.0f%% of the copy bandwidth" % (
                        best / passes, NEEDED_PER_ROW, passes * rows * NEEDED_PER_ROW / best / 1e6, SECTOR_PER_ROW,
                        passes * rows * SECTOR_PER_ROW / best / 1e6, 100 * passes * rows * SECTOR_PER_ROW / best / 1e6 / gbs)
        print(line, flush=True)
    a = rnd.cpu().numpy().tobytes()
    t0 = time.perf_counter()
    res = ctx.anon_set_audit(a)
    print("anon_set_audit from a host buffer (upload, index, compare), random keys: %.0f ms, kernels %.2f ms -> %r" % (
        (time.perf_counter() - t0) * 1e3, ctx.last_ms(9), res), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dir", default="/dev/shm")
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    z = load_package()
    d = os.path.join(args.dir, "zkpoa_audit_time")
    os.makedirs(d, exist_ok=True)
    csv = os.path.join(d, "anonymity_set.csv")
    run = os.path.join(ROOT, "tests", "golden", "ref", "4_sigs_2_batches_12_height__layer_three")
    vkey = os.path.join(ROOT, "tests", "golden", "ref", "layer_three_vkey.json")
    t0 = time.perf_counter()
    json.dump(write_csv(csv, args.rows), open(os.path.join(d, "poa.json"), "w"))
    print("wrote %d rows, %.0f MB in %.0f s" % (args.rows, os.path.getsize(csv) / 1e6, time.perf_counter() - t0), flush=True)
    env = dict(os.environ, ZKPOA_VERBOSE="1")
    try:
        for i in range(3):
            t0 = time.perf_counter()
            rc = subprocess.run([z.AUDIT_BIN, "--anon-set", csv, "--vkey", vkey, "--public", os.path.join(run, "public.json"),
                                 "--proof", os.path.join(run, "proof.json")], env=env, capture_output=True, text=True)
            dt = time.perf_counter() - t0
            assert rc.returncode == 1 and rc.stdout.splitlines()[-1] == "AUDIT FAILED: root", rc.stdout + rc.stderr
            print("zkpoa-audit, %d rows: %.2f s  (%s)" % (args.rows, dt, " | ".join(rc.stdout.splitlines()[:2])), flush=True)
            for l in rc.stderr.splitlines():
                if l.startswith("zkpoa"):
                    print("    " + l, flush=True)
        for i in range(2):
            t0 = time.perf_counter()
            rc = subprocess.run([z.MERKLE_BIN, "-a", csv, "-p", os.path.join(d, "poa.json"), "-o", d], env=env,
                                capture_output=True, text=True)
            dt = time.perf_counter() - t0
            assert rc.returncode == 0, rc.stderr
            print("merkle-tree, same file: %.2f s" % dt, flush=True)
            for l in rc.stderr.splitlines():
                if l.startswith("merkle-tree:"):
                    print("    " + l, flush=True)
    finally:
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
        os.rmdir(d)
    index_kernels(z, torch, args.rows)


if __name__ == "__main__":
    main()
