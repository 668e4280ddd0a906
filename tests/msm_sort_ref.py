"""What phase A of the MSM (csrc/msm.hip.h msm_sort_phase) must hand the accumulation, restated with Python integers
and numpy and none of the project's code: sign normalisation, the signed-digit recoding as msm_digits_kernel documents it,
the entries of the classic and the fixed-base (merged) form, and from them the bucket counts, their offsets, the level-0
pieces, the piece-length histogram and the totals; and the digit density of msm_density_kernel.
tests/test_msm_sort_ref.py checks this file itself, tests/test_gpu_msm_sort.py the device against it."""
import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
HALF = (R - 1) // 2
SIGN = 1 << 31


def windows(c):
    return (254 + c - 1) // c


def normalise(s):
    """s > (r - 1) / 2 becomes r - s with the sign flipped -> (magnitude, negated)"""
    return (R - s, 1) if s > HALF else (s, 0)


def recode(s, c):
    """The signed c-bit digits of one scalar, lowest window first -> ([(magnitude, sign)] * windows(c), carry out of the
    top window). d = (s & mask) + carry; carry = d > Nb; mag = carry ? 2^c - d : d; sign = carry xor negated."""
    t, negated = normalise(s)
    nb, mask = 1 << (c - 1), (1 << c) - 1
    carry, out = 0, []
    for _ in range(windows(c)):
        d = (t & mask) + carry
        t >>= c
        carry = 1 if d > nb else 0
        mag = (1 << c) - d if carry else d
        out.append((mag, (carry ^ negated) if mag else 0))
    return out, carry


def digits_value(digits, c):
    """the integer the signed digits stand for"""
    return sum((-mag if sign else mag) << (c * w) for w, (mag, sign) in enumerate(digits))


def edge_scalars(c):
    """The scalars at which a recoding goes wrong: the ends of the range and of the normalisation, every power of two
    and its predecessor (2^(3c) - 1 gives a zero digit that carries), and the scalars whose digits are all Nb (the
    largest magnitude that does not carry) or all Nb + 1 (the smallest that does), as long as they stay below r and as
    long as they stay below (r - 1) / 2, where the normalisation leaves them alone."""
    out = [0, 1, 2, R - 1, R - 2, HALF, HALF + 1, HALF - 1, (R + 1) // 2]
    for k in range(254):
        out += [v for v in (1 << k, (1 << k) - 1) if v < R]
    nb = 1 << (c - 1)
    for digit in (nb, nb + 1):
        v, below_half = 0, None
        for w in range(windows(c)):
            nxt = v + (digit << (c * w))
            if nxt >= R:
                break
            v = nxt
            if v <= HALF:
                below_half = v
        out += [v, below_half]
    return sorted(set(out))


def entries(scalars, c, merged):
    """One entry per non-zero digit -> (bucket, payload) as numpy arrays. Classic form: bucket w * Nb + mag - 1, payload
    i | sign << 31; merged form: one bucket set, bucket mag - 1, payload (w * n + i) | sign << 31."""
    n, nb, mask = len(scalars), 1 << (c - 1), (1 << c) - 1
    W = windows(c)
    bucket, payload = [], []
    for i, s in enumerate(scalars):
        t, negated = normalise(s)
        carry = 0
        for w in range(W):
            if not t and not carry:
                break                       # every further digit is zero
            d = (t & mask) + carry
            t >>= c
            carry = 1 if d > nb else 0
            mag = (1 << c) - d if carry else d
            if mag:
                sign = SIGN if carry ^ negated else 0
                bucket.append(mag - 1 if merged else w * nb + mag - 1)
                payload.append(((w * n + i) if merged else i) | sign)
        assert not carry
    return np.array(bucket, dtype=np.int64), np.array(payload, dtype=np.uint32)


def keys(bucket, payload):
    """sorted (bucket << 32 | payload): the multiset of payloads of every bucket, order inside a bucket set aside"""
    return np.sort((bucket.astype(np.uint64) << np.uint64(32)) | payload.astype(np.uint64))


def excl(v):
    out = np.zeros(len(v) + 1, dtype=np.int64)
    np.cumsum(v, out=out[1:])
    return out


def sort_result(scalars, c, merged, k0):
    """Everything phase A hands on, for piece length k0, as a dict of integers and numpy arrays."""
    W, nb = windows(c), 1 << (c - 1)
    tb = nb if merged else W * nb
    bucket, payload = entries(scalars, c, merged)
    counts = np.bincount(bucket, minlength=tb).astype(np.int64)
    pieces = -(-counts // k0)
    po_a = excl(pieces)
    total1 = int(po_a[-1])
    pbkt = np.repeat(np.arange(tb, dtype=np.int64), pieces)
    j = np.arange(total1, dtype=np.int64) - po_a[pbkt]
    piece_len = np.minimum(k0, counts[pbkt] - j * k0)
    return {"W": W, "TB": tb, "counts": counts, "off0": excl(counts), "po_a": po_a, "total_entries": int(counts.sum()),
            "max_count": int(counts.max()) if tb else 0, "total1": total1, "pbkt": pbkt, "piece_len": piece_len,
            "len_hist": np.bincount(piece_len, minlength=k0 + 1).astype(np.int64), "keys": keys(bucket, payload)}


def density(scalars):
    """32 doubles indexed by the window width: sum(ceil(bitlen(normalised s) / c)) / n for c = 4..25, the uniform default
    ceil(254 / max(c, 4)) elsewhere and for no scalars at all"""
    out = [float(windows(max(c, 4))) for c in range(32)]
    n = len(scalars)
    if n:
        lengths = [normalise(s)[0].bit_length() for s in scalars]
        for c in range(4, 26):
            out[c] = sum(-(-L // c) for L in lengths) / n
    return out
