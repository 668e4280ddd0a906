"""Time of the ECDSA -> ECDSA* step on 2^20 signatures: the kernels of zkpoa_ecdsa_star (signatures / s) and the whole
`ecdsa-sigs-parser` command on the corresponding JSON file, split into read, device and write (its ZKPOA_VERBOSE lines).
Medians of three after a warm run. The signatures come from the generator of tests/secp_ref.py (nonce points and keys
walked by additions, answers known by construction), here with the additions batched: R_i = A_(i // 1024) + B_(i % 1024)
with one shared inversion per 2^16 sums. The addresses are taken from zkpoa_eth_address (which the GPU tests pin
against the restatement): Keccak in pure Python would take ten minutes for them.
  python tools/sigs_parser_time.py [--log 20] [--dir /dev/shm] [--cpu 256]"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import secp_ref as sr  # noqa: E402

P, N = sr.P, sr.N


def batch_inverse(vals, mod):
    pre, acc = [], 1
    for v in vals:
        pre.append(acc)
        acc = acc * v % mod
    inv = pow(acc, -1, mod)
    out = [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = pre[i] * inv % mod
        inv = inv * vals[i] % mod
    return out


def walk(start_scalar, count):
    """[(start + i) G for i < count] as affine points, 2^16 independent additions per inversion."""
    step = 1024
    rows = (count + step - 1) // step
    a = [sr.mul(start_scalar + j * step, sr.G) for j in range(rows)]
    b = [None] + [sr.mul(l, sr.G) for l in range(1, step)]
    out = []
    for j0 in range(0, rows, 64):
        pairs = [(a[j], b[l]) for j in range(j0, min(rows, j0 + 64)) for l in range(1, step)]
        inv = batch_inverse([(q[0] - p[0]) % P for p, q in pairs], P)   # distinct x: start + i never meets +-l here
        sums = iter(zip(pairs, inv))
        for j in range(j0, min(rows, j0 + 64)):
            out.append(a[j])
            for _ in range(1, step):
                (p, q), iv = next(sums)
                lam = (q[1] - p[1]) * iv % P
                x = (lam * lam - p[0] - q[0]) % P
                out.append((x, (lam * (p[0] - x) - p[1]) % P))
    return out[:count]


def generate(count, seed):
    rng = random.Random(seed)
    k0, d0 = rng.randrange(1 << 200, N - count), rng.randrange(1 << 200, N - count)
    rs, qs = walk(k0, count), walk(d0, count)
    kinv = batch_inverse([k0 + i for i in range(count)], N)
    out = []
    for i in range(count):
        big_r, r = rs[i], rs[i][0]
        z = rng.getrandbits(256)
        s = kinv[i] * (z + r * (d0 + i)) % N
        v, rprime = 27 + (big_r[1] & 1), big_r[1]
        if s >= 1 << 255:
            s, v, rprime = N - s, 55 - v, P - rprime
        out.append((r, s, v, z, rprime, qs[i]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, default=20)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--cpu", type=int, default=256, help="entries of the pure-Python restatement to time (0: none)")
    args = ap.parse_args()
    from __graft_entry__ import load_package
    z = load_package()
    n = 1 << args.log
    t0 = time.perf_counter()
    sigs = generate(n, 5)
    print("generated %d signatures on the host in %.0f s (not timed below)" % (n, time.perf_counter() - t0), flush=True)
    be = lambda v: v.to_bytes(32, "big")
    r = b"".join(be(e[0]) for e in sigs)
    s = b"".join(be(e[1]) for e in sigs)
    v = bytes(e[2] for e in sigs)
    zz = b"".join(be(e[3]) for e in sigs)
    want_rp = b"".join(be(e[4]) for e in sigs)
    want_pk = b"".join(be(e[5][0]) + be(e[5][1]) for e in sigs)
    ctx = z.Context(0)
    addr, text = ctx.eth_address(want_pk)
    ms = []
    for rep in range(4):
        rp, pk, ad, st = ctx.ecdsa_star(r, s, zz, v, addr)
        assert (rp, pk, ad, st) == (want_rp, want_pk, addr, bytes(n)), "the device disagrees with the generator"
        if rep:
            ms.append(ctx.last_ms(8))
    med = statistics.median(ms)
    print("zkpoa_ecdsa_star kernels, %d signatures: %s ms, median %.1f ms -> %.3f M signatures/s"
          % (n, " ".join("%.1f" % m for m in ms), med, n / med / 1e3), flush=True)
    ctx.close()
    if args.cpu:
        t0 = time.perf_counter()
        for e, a in zip(sigs[:args.cpu], (addr[20 * i:20 * i + 20] for i in range(args.cpu))):
            assert sr.recover(e[0], e[1], e[2], e[3], a)[0] == sr.OK
        dt = time.perf_counter() - t0
        print("for scale only: tests/secp_ref.py (pure Python, one thread, one recovery per entry where the reference does "
              "two and two more multiplications), %d entries: %.2f s -> %.0f signatures/s" % (args.cpu, dt, args.cpu / dt), flush=True)
    d = os.path.join(args.dir, "zkpoa_sigs_time")
    os.makedirs(d, exist_ok=True)
    src, out = os.path.join(d, "signatures.json"), os.path.join(d, "parsed.json")
    try:
        with open(src, "w") as f:
            f.write("[")
            for i, e in enumerate(sigs):
                f.write(("," if i else "") + json.dumps({"signature": {"r": sr.hex32(e[0]), "s": sr.hex32(e[1]), "v": e[2], "msghash": sr.hex32(e[3])},
                                                         "address": text[i], "balance": "%dn" % (i + 1)}, separators=(",", ":")))
            f.write("]")
        print("input %.0f MB" % (os.path.getsize(src) / 1e6), flush=True)
        walls, laps = [], []
        for rep in range(4):
            t0 = time.perf_counter()
            rc = subprocess.run([z.SIGS_BIN, "-s", src, "-o", out], env=dict(os.environ, ZKPOA_VERBOSE="1"), capture_output=True, text=True)
            dt = time.perf_counter() - t0
            assert rc.returncode == 0, rc.stderr
            lap = {l.split()[2]: float(l.split()[-2]) for l in rc.stderr.splitlines() if l.startswith("zkpoa: ecdsa-sigs-parser:")}
            print("  run %d: %.2f s wall; read %.0f ms, device %.0f ms, write %.0f ms" % (rep, dt, lap["read"], lap["device"], lap["write"]), flush=True)
            if rep:
                walls.append(dt)
                laps.append(lap)
        print("ecdsa-sigs-parser, %d signatures, output %.0f MB: median %.2f s wall (read %.2f s, device with both copies %.2f s, write %.2f s)"
              % (n, os.path.getsize(out) / 1e6, statistics.median(walls), statistics.median(l["read"] for l in laps) / 1e3,
                 statistics.median(l["device"] for l in laps) / 1e3, statistics.median(l["write"] for l in laps) / 1e3), flush=True)
    finally:
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
        os.rmdir(d)


if __name__ == "__main__":
    main()
