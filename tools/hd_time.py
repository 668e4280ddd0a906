"""Time of BIP-32 derivation on the device: 2^20 children of one parent, private and public (zkpoa_bip32_children: the HMAC
kernel and the tweak kernel), the tweak kernel alone (zkpoa_bip32_tweak), and in the same process zkpoa_secp256k1_pubkey
on 2^20 keys, the kernel the tweak kernel is built from. Kernel times are the library's HIP events (zkpoa_last_ms 8);
zkpoa_secp256k1_pubkey reports none, so every call is also timed on the host clock, copies included -- its kernel's own
time comes from a run of this script under a kernel trace. Medians of three after a warm run. The first and last children
are compared with tests/hd_ref.py.
  python tools/hd_time.py [--log 20] [--cpu 8]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hd_ref as hd  # noqa: E402


def timed(what, n, call, kernel_ms):
    """call() four times -> (median kernel ms or None, median wall ms) of the last three."""
    ms, wall = [], []
    for rep in range(4):
        t0 = time.perf_counter()
        out = call()
        dt = (time.perf_counter() - t0) * 1e3
        if rep:
            wall.append(dt)
            ms.append(kernel_ms() if kernel_ms else 0.0)
    k, w = statistics.median(ms), statistics.median(wall)
    if kernel_ms:
        print("%s, %d lanes: kernels %s ms, median %.2f ms -> %.2f M/s; whole call (copies included) median %.1f ms"
              % (what, n, " ".join("%.2f" % m for m in ms), k, n / k / 1e3, w), flush=True)
    else:
        print("%s, %d lanes: whole call (copies included) %s ms, median %.1f ms" % (what, n, " ".join("%.1f" % m for m in wall), w), flush=True)
    return k, w, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, default=20)
    ap.add_argument("--cpu", type=int, default=8, help="children at either end to compare with the pure-Python restatement")
    args = ap.parse_args()
    from __graft_entry__ import load_package
    z = load_package()
    n = 1 << args.log
    key, chain = z.bip32_master(bytes(range(32)))
    pub = hd.neuter(key)
    ctx = z.Context(0)
    ms8 = lambda: ctx.last_ms(8)
    k_priv, _, priv = timed("zkpoa_bip32_children, private parent", n, lambda: ctx.bip32_children(key, chain, 0, n), ms8)
    k_pub, _, pubs = timed("zkpoa_bip32_children, public parent", n, lambda: ctx.bip32_children(pub, chain, 0, n), ms8)
    assert priv[4] == bytes(n) and pubs[4] == bytes(n) and priv[1:4] == pubs[1:4], "the public derivation disagrees with the private one"
    tweaks = priv[1]          # any 2^20 values below the group order serve as IL: the chain codes
    t_priv, _, _ = timed("zkpoa_bip32_tweak (the tweak kernel alone), private parent", n, lambda: ctx.bip32_tweak(key, tweaks), ms8)
    t_pub, _, _ = timed("zkpoa_bip32_tweak (the tweak kernel alone), public parent", n, lambda: ctx.bip32_tweak(pub, tweaks), ms8)
    keys = b"".join(priv[0][33 * i + 1:33 * i + 33] for i in range(n))
    _, w_key, pk = timed("zkpoa_secp256k1_pubkey on the children's keys (the baseline: the parent commit's kernel)", n,
                         lambda: ctx.secp256k1_pubkey(keys), None)
    assert pk[0] == priv[2] and pk[1] == priv[3] and pk[2] == bytes(n), "zkpoa_secp256k1_pubkey disagrees with the derivation"
    print("parts: HMAC kernel = children - tweak: private %.2f ms, public %.2f ms; the public parent's mixed addition = tweak public - "
          "tweak private: %.2f ms" % (k_priv - t_priv, k_pub - t_pub, t_pub - t_priv), flush=True)
    for i in list(range(args.cpu)) + list(range(n - args.cpu, n)):
        c = hd.child(key, chain, i)
        got = dict(status=priv[4][i], key=priv[0][33 * i:33 * i + 33], chain=priv[1][32 * i:32 * i + 32],
                   pub=(int.from_bytes(priv[2][64 * i:64 * i + 32], "big"), int.from_bytes(priv[2][64 * i + 32:64 * i + 64], "big")),
                   address=priv[3][20 * i:20 * i + 20])
        assert got == c, i
    print("children 0..%d and %d..%d agree with tests/hd_ref.py" % (args.cpu - 1, n - args.cpu, n - 1), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
