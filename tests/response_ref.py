"""Big-integer restatement of DESIGN.md "Phase-1 transcript", part "Challenge and response files" (test infrastructure): the
square roots in Fq and Fq2 with the sign rule, the way back from the compressed form and from the hash form, and the
layout of the two files. Written from that text, not from csrc/ptau_response.hip. The forward forms, Blake2b with its
saved state, the key and the records come from tests/phase1_ref.py and tests/phase2_ref.py."""
import phase1_ref as p1
import phase2_ref as p2
from oracle.py import bn254 as bn

Q, R = bn.Q, bn.R
F2 = bn.FQ2
KEY_BYTES = 6 * 64 + 3 * 128
GROUPS = ((2, 1), (3, 2), (4, 1), (5, 1), (6, 2))                    # section, group, in file order


class FormError(ValueError):
    """kind: 'range' (not below q), 'bit7', 'flags' (both flag bits), 'infinity' (0x40, then not zeros), 'curve'."""

    def __init__(self, kind):
        ValueError.__init__(self, kind)
        self.kind = kind


# ---- roots: the one that is not negative, None for a non-square -------------------------------------------------------
def fq_sqrt(a):
    a %= Q
    r = pow(a, (Q + 1) // 4, Q)                                      # q = 3 mod 4
    if r * r % Q != a:
        return None
    return Q - r if p2.fq_negative(r) else r


def fq2_sqrt(a):
    """a0 + a1 u, u^2 = -1. With n = a0^2 + a1^2 a square in Fq (else a is none in Fq2) and d its root, one of
    (a0 + d) / 2, (a0 - d) / 2 is a square c0^2 in Fq, and c1 = a1 / (2 c0). a1 = 0: a real root of a0, or u times a real
    root of -a0."""
    a0, a1 = a[0] % Q, a[1] % Q
    if a1 == 0:
        r = fq_sqrt(a0)
        if r is not None:
            root = (r, 0)
        else:
            root = (0, fq_sqrt(Q - a0))                              # -1 is a non-residue: one of the two is a square
    else:
        d = fq_sqrt((a0 * a0 + a1 * a1) % Q)
        if d is None:
            return None
        inv2 = (Q + 1) // 2
        c0 = fq_sqrt((a0 + d) * inv2 % Q)
        if c0 is None:
            c0 = fq_sqrt((a0 - d) * inv2 % Q)
        root = (c0, a1 * pow(2 * c0, -1, Q) % Q)
    assert F2.eq(F2.sqr(root), (a0, a1))
    return F2.neg(root) if p2.fq2_negative(root) else root


# ---- compressed form -> point -------------------------------------------------------------------------------------------
def _be(b):
    return int.from_bytes(b, "big")


def _flags(b):
    """(negative, infinity) of the first byte, and the bytes with both bits taken off"""
    if b[0] & 0xc0 == 0xc0:
        raise FormError("flags")
    rest = bytes([b[0] & 0x3f]) + bytes(b[1:])
    if b[0] & 0x40 and any(rest):
        raise FormError("infinity")
    return bool(b[0] & 0x80), bool(b[0] & 0x40), rest


def decompress_g1(b):
    assert len(b) == 32
    neg, inf, rest = _flags(b)
    if inf:
        return None
    x = _be(rest)
    if x >= Q:
        raise FormError("range")
    y = fq_sqrt((x * x * x + bn.B1) % Q)
    if y is None:
        raise FormError("curve")
    return (x, Q - y if neg and y else y)


def decompress_g2(b):
    assert len(b) == 64
    neg, inf, rest = _flags(b)
    if inf:
        return None
    x = (_be(rest[32:]), _be(rest[:32]))                              # c1 then c0
    if x[0] >= Q or x[1] >= Q:
        raise FormError("range")
    y = fq2_sqrt(F2.add(F2.mul(F2.sqr(x), x), bn.B2))
    if y is None:
        raise FormError("curve")
    return (x, F2.neg(y) if neg else y)


# ---- hash form -> point -----------------------------------------------------------------------------------------------
def _unhash(b, coords):
    if b[0] & 0x80:
        raise FormError("bit7")
    if b[0] == 0x40:
        if any(b[1:]):
            raise FormError("infinity")
        return None
    v = [_be(b[32 * i:32 * i + 32]) for i in range(coords)]
    if any(c >= Q for c in v):
        raise FormError("range")
    return v


def unhash_g1(b):
    v = _unhash(b, 2)
    return None if v is None else (v[0], v[1])


def unhash_g2(b):
    v = _unhash(b, 4)
    return None if v is None else ((v[1], v[0]), (v[3], v[2]))


# ---- the two files ------------------------------------------------------------------------------------------------------
def challenge_size(power):
    n = 1 << power
    return 64 + 64 * (2 * n - 1) + 128 * n + 64 * n + 64 * n + 128


def response_size(power):
    n = 1 << power
    return 64 + 32 * (2 * n - 1) + 64 * n + 32 * n + 32 * n + 64 + KEY_BYTES


def power_of(size, size_of):
    """The power in [1, 28] whose file has `size` bytes; None for any other size."""
    for power in range(1, 29):
        if size_of(power) == size:
            return power
    return None


def challenge_file(last_response, secs):
    """last_response: the response hash of the last record, Blake2b-512 of the empty string without records."""
    return last_response + p1.hash_form(secs)


def key_form(key_g1, key_g2):
    return b"".join(p2.hash_g1(P) for P in key_g1) + b"".join(p2.hash_g2(P) for P in key_g2)


def response_file(challenge, new_secs, key_g1, key_g2):
    return challenge + p1.compressed_form(new_secs) + key_form(key_g1, key_g2)


def response_offset(power, section, index):
    """byte offset of point `index` of `section` in a response file"""
    n = 1 << power
    counts = {2: 2 * n - 1, 3: n, 4: n, 5: n, 6: 1}
    at = 64
    for t, grp in GROUPS:
        if t == section:
            return at + 32 * grp * index
        at += 32 * grp * counts[t]
    raise KeyError(section)


def g1_x_off_curve(start):
    """the first x >= start for which x^3 + 3 is no square"""
    x = start
    while fq_sqrt((x * x * x + bn.B1) % Q) is not None:
        x += 1
    return x


def g2_x_off_curve(start):
    x = (start, 1)
    while fq2_sqrt(F2.add(F2.mul(F2.sqr(x), x), bn.B2)) is not None:
        x = (x[0] + 1, 1)
    return x


def twist_point_outside_g2(start):
    """A point of the twist that is not in G2 (the twist's order is r (2q - r): nearly every point is outside)."""
    x = (start, 1)
    while True:
        y = fq2_sqrt(F2.add(F2.mul(F2.sqr(x), x), bn.B2))
        if y is not None and bn.ec_mul((x, y), R, F2, order=1 << 300) is not None:
            return (x, y)
        x = (x[0] + 1, 1)
