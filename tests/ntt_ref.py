"""References and input sets for the Fr NTT tests (tests/test_gpu_ntt.py). Test infrastructure, written against
oracle/c_oracle.py and oracle/py only: buffers are 32-byte little-endian Montgomery-form elements as zkpoa_ntt takes
them, and every expected value is the C oracle's transform, moved around by exact identities (a permutation, one
oracle multiplication). tests/test_ntt_ref.py pins these helpers without a GPU."""
import functools

import numpy as np

from oracle import c_oracle as co
from oracle.py import bn254 as bn

R, M = bn.R, bn.MONT_R
_EL = np.dtype("V32")


def pack(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def unpack(buf):
    return [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]


# ---- orderings -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def bitrev_perm(k):
    """rev[i] = the k-bit reversal of i, as a (read-only, cached) numpy index array"""
    i = np.arange(1 << k, dtype=np.int64)
    rev = np.zeros_like(i)
    for b in range(k):
        rev |= ((i >> b) & 1) << (k - 1 - b)
    rev.setflags(write=False)
    return rev


def permute(buf, k):
    """out[i] = buf[bitrev_k(i)] on 32-byte elements: natural order <-> bit-reversed order (an involution)"""
    return np.frombuffer(buf, dtype=_EL, count=1 << k)[bitrev_perm(k)].tobytes()


def negate_index(buf, k):
    """out[i] = buf[-i mod n]. The transform of the index-negated vector is the index-negated transform (either root)."""
    n = 1 << k
    return np.frombuffer(buf, dtype=_EL, count=n)[(-np.arange(n, dtype=np.int64)) % n].tobytes()


def scale(buf, s):
    """every element times the integer s mod r: one oracle Montgomery multiplication by s in Montgomery form"""
    n = len(buf) // 32
    return co.field_op(1, 0, buf, (s * M % R).to_bytes(32, "little") * n)


# ---- the odd coset ---------------------------------------------------------------------------------------
def coset_ref(x, k):
    """Evaluations on the n-point domain -> evaluations on its odd coset inc * <w_n>, inc = w_2n (what the prover's
    ifft, batchApplyKey(1, inc), fft chain computes): the odd coset of the n-point domain is the odd half of the
    2n-point domain, so it is the odd slots of the oracle's 2n-point transform of the zero-padded coefficients."""
    if k == 0:
        return bytes(x[:32])
    n = 1 << k
    coefs = co.ntt(x, k, inverse=True)
    big = co.ntt(coefs + bytes(32 * n), k + 1)
    return np.frombuffer(big, dtype=_EL, count=2 * n)[1::2].tobytes()


# ---- input sets --------------------------------------------------------------------------------------------
def uniform_bytes(n, seed):
    """n elements uniform over the whole of [0, r) (vectorised rejection sampling from [0, 2^254))"""
    nr = np.random.default_rng(seed)
    rl = [np.uint64((R >> (64 * j)) & (2**64 - 1)) for j in range(4)]
    out, have = [], 0
    while have < n:
        limbs = nr.integers(0, 2**64, size=(n - have + (n - have) // 2 + 16, 4), dtype=np.uint64)
        limbs[:, 3] &= np.uint64(2**62 - 1)
        below = np.zeros(len(limbs), dtype=bool)
        equal = np.ones(len(limbs), dtype=bool)
        for j in (3, 2, 1, 0):
            below |= equal & (limbs[:, j] < rl[j])
            equal &= limbs[:, j] == rl[j]
        out.append(limbs[below])
        have += int(below.sum())
    return np.ascontiguousarray(np.concatenate(out)[:n]).tobytes()


def edge_vectors(k, rng, info=None):
    """name -> 2^k canonical elements where a lazy butterfly layer goes wrong without a random band noticing: exact
    zeros out of u - v with u == v, a single non-zero output, the top of the range. `info` (a dict) receives the
    constant c and the odd exponent m, for the closed forms (tests/test_ntt_ref.py)."""
    n = 1 << k
    c = rng.randrange(1, R)
    m = 2 * rng.randrange(n // 2) + 1 if n > 1 else 1
    w = bn.fr_root_of_unity(k)
    if info is not None:
        info.update(c=c, m=m)

    def delta(at):
        return [c if i == at else 0 for i in range(n)]
    geo, g, wm = [], c, pow(w, m, R)
    for _ in range(n):
        geo.append(g)
        g = g * wm % R
    vecs = {
        "zero": [0] * n,
        "constant": [c] * n,
        "all_r_minus_1": [R - 1] * n,
        "delta_0": delta(0),
        "delta_mid": delta(n // 2),
        "delta_last": delta(n - 1),
        "alternating": [c if i % 2 == 0 else R - c for i in range(n)],
        "geometric": geo,                                   # c * w_n^(m i): forward transform n c at slot -m mod n
        "uniform": [rng.randrange(R) for _ in range(n)],
        "near_r": [R - 1 - rng.randrange(1 << 200) for _ in range(n)],
    }
    return {name: pack(v) for name, v in vecs.items()}
