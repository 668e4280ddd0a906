"""Time of signing on 2^20 derived keys: the kernels of zkpoa_ecdsa_sign (signatures / s) next to those of
zkpoa_ecdsa_star on the same 2^20 signatures in the same process, and the whole `ecdsa-sigs-parser sign` and `anon-set`
commands split into keys, device, sort and write (their ZKPOA_VERBOSE lines). Medians of three after a warm run. Every
signature goes back through the recovery (all statuses 0, every recovered key the signer's), and the first entries are
compared with tests/sign_ref.py.
  python tools/sign_time.py [--log 20] [--anon 10000000] [--dir /dev/shm] [--cpu 64]"""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sign_ref as sg  # noqa: E402


def laps_of(stderr, command):
    return {l.split()[3]: float(l.split()[-2]) for l in stderr.splitlines() if l.startswith("zkpoa: %s:" % command)}


def timed(argv, command, names):
    walls, laps = [], []
    for rep in range(4):
        t0 = time.perf_counter()
        rc = subprocess.run(argv, env=dict(os.environ, ZKPOA_VERBOSE="1"), capture_output=True, text=True)
        dt = time.perf_counter() - t0
        assert rc.returncode == 0, rc.stderr
        lap = laps_of(rc.stderr, command)
        print("  run %d: %.2f s wall; %s" % (rep, dt, ", ".join("%s %.0f ms" % (k, lap[k]) for k in names)), flush=True)
        if rep:
            walls.append(dt)
            laps.append(lap)
    return statistics.median(walls), {k: statistics.median(l[k] for l in laps) / 1e3 for k in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, default=20)
    ap.add_argument("--anon", type=int, default=10_000_000)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--cpu", type=int, default=64, help="entries to compare with the pure-Python restatement")
    args = ap.parse_args()
    from __graft_entry__ import load_package
    z = load_package()
    n = 1 << args.log
    seed, message = b"sign_time", b"my message to sign"
    ctx = z.Context(0)
    keys = ctx.secp256k1_derive_keys(seed, 0, n)
    h = hashlib.sha256(message).digest()
    ms = []
    for rep in range(4):
        r, s, v, pk, ad, st = ctx.ecdsa_sign(keys, h, 0)
        assert st == bytes(n)
        if rep:
            ms.append(ctx.last_ms(8))
    med = statistics.median(ms)
    print("zkpoa_ecdsa_sign kernels, %d keys: %s ms, median %.1f ms -> %.3f M signatures/s"
          % (n, " ".join("%.1f" % m for m in ms), med, n / med / 1e3), flush=True)
    ms_star = []
    for rep in range(4):
        rp, pk2, ad2, st2 = ctx.ecdsa_star(r, s, h * n, v, ad)
        assert st2 == bytes(n) and pk2 == pk and ad2 == ad, "the recovery disagrees with the signer"
        if rep:
            ms_star.append(ctx.last_ms(8))
    med_star = statistics.median(ms_star)
    print("zkpoa_ecdsa_star kernels on those %d signatures, same process: %s ms, median %.1f ms -> %.3f M signatures/s; signing / recovery "
          "rate %.2f" % (n, " ".join("%.1f" % m for m in ms_star), med_star, n / med_star / 1e3, med_star / med), flush=True)
    zi = int.from_bytes(h, "big")
    t0 = time.perf_counter()
    for i in range(args.cpu):
        d = int.from_bytes(keys[32 * i:32 * i + 32], "big")
        assert d == sg.derive_key(seed, i)
        g = sg.sign(d, zi)
        assert (g["r"].to_bytes(32, "big"), g["s"].to_bytes(32, "big"), g["v"], g["address"]) == \
            (r[32 * i:32 * i + 32], s[32 * i:32 * i + 32], v[i], ad[20 * i:20 * i + 20]), i
    if args.cpu:
        dt = time.perf_counter() - t0
        print("for scale only: tests/sign_ref.py (pure Python, one thread), %d entries: %.2f s -> %.0f signatures/s"
              % (args.cpu, dt, args.cpu / dt), flush=True)
    ctx.close()
    d = os.path.join(args.dir, "zkpoa_sign_time")
    os.makedirs(d, exist_ok=True)
    out, csv = os.path.join(d, "signatures.json"), os.path.join(d, "anonymity_set.csv")
    try:
        source = ["--generate-keys", str(n), "--seed", seed.decode()]
        names = ("keys", "device", "sort", "write")
        wall, lap = timed([z.SIGS_BIN, "sign"] + source + ["--message", message.decode(), "--output-path", out], "ecdsa-sigs-parser sign", names)
        print("ecdsa-sigs-parser sign, %d derived keys, output %.0f MB: median %.2f s wall (%s)"
              % (n, os.path.getsize(out) / 1e6, wall, ", ".join("%s %.2f s" % (k, lap[k]) for k in names)), flush=True)
        names = ("device", "sort", "write")
        wall, lap = timed([z.SIGS_BIN, "anon-set"] + source + ["--num-addresses", str(args.anon), "--output-path", csv],
                          "ecdsa-sigs-parser anon-set", names)
        print("ecdsa-sigs-parser anon-set, %d addresses (%d of them from keys), output %.0f MB: median %.2f s wall (%s)"
              % (args.anon, min(n, args.anon), os.path.getsize(csv) / 1e6, wall, ", ".join("%s %.2f s" % (k, lap[k]) for k in names)), flush=True)
    finally:
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
        os.rmdir(d)


if __name__ == "__main__":
    main()
