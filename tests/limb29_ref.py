"""Big-int reference and operand sets for the 9 x 29-bit-limb field (zk-proof-of-assets_amd/csrc/fq29.hip.h), shared by
tests/test_limb29_host.py (the header compiled by g++) and tests/test_gpu_limb29.py (zkpoa_fq29_prim). Test
infrastructure, written against oracle/py/bn254.py only. The operand classes, their bounds and the rules for combining
them are the ones stated at the top of the header:
  N  limbs 0..7 < 2^29, value < 3q          X  normalised, value < 13q          W  normalised, value < 2^256
  P  normalised, value < 17q (a normalised difference)
  D  limbs < 3 * 2^29, value < 17q          Y  limbs < 2^30, value < 6q (a negated coordinate: C4 - N or C6 - W)
A product takes at most one un-normalised operand and va * vb <= 338 q^2 (dot2: the sum of both products)."""
import random
import struct

from oracle.py import bn254 as bn

Q = bn.Q
M29 = (1 << 29) - 1
RINV = pow(1 << 261, -1, Q)
OP_MUL, OP_SQR, OP_DOT2, OP_SUB4, OP_RELIMB, OP_MADD, OP_ADD, OP_SUB14, OP_PIECE = range(9)

# class -> (limb bound (exclusive) of limbs 0..7, value bound (exclusive))
CLASSES = {"N": (1 << 29, 3 * Q), "X": (1 << 29, 13 * Q), "W": (1 << 29, 1 << 256), "P": (1 << 29, 17 * Q),
           "D": (3 << 29, 17 * Q), "Y": (1 << 30, 6 * Q)}


def limbs(v):
    """the normalised limb vector of v"""
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def value(l):
    return sum(x << (29 * i) for i, x in enumerate(l))


def is_normalised(l):
    return all(0 <= x <= M29 for x in l[:8]) and 0 <= l[8] < (1 << 32)


def rand_elem(rng, cls):
    """a random member of the class: a value below its bound, spread over limbs up to the class's limb bound"""
    lb, vb = CLASSES[cls]
    v = rng.randrange(vb)
    l = limbs(v)
    if lb > (1 << 29):           # un-normalise: move multiples of 2^29 from limb i + 1 down into limb i
        for i in range(7, -1, -1):
            k = min(l[i + 1], (lb - 1 - l[i]) >> 29)
            k = rng.randrange(k + 1)
            l[i + 1] -= k
            l[i] += k << 29
    assert value(l) == v and all(x < lb for x in l[:8])
    return l


def max_elem(cls):
    """every limb at the largest value the class allows: limbs 0..7 at the limb bound, limb 8 as large as the value
    bound leaves room for"""
    lb, vb = CLASSES[cls]
    low = [lb - 1] * 8
    top = (vb - 1 - value(low + [0])) >> 232
    l = low + [top]
    assert value(l) < vb and value(low + [top + 1]) >= vb
    return l


def special_values(cls):
    """0, 1, q - 1, q, 2q - 1 and the largest multiple of q the class holds, normalised"""
    vb = CLASSES[cls][1]
    vals = [0, 1, Q - 1, Q, 2 * Q - 1, ((vb - 1) // Q) * Q, vb - 1]
    return [limbs(v) for v in vals if v < vb]


def pack(records):
    return b"".join(struct.pack("<%dI" % len(r), *r) for r in records)


def unpack(data, words):
    n = len(data) // (4 * words)
    return [list(struct.unpack_from("<%dI" % words, data, 4 * words * i)) for i in range(n)]


# the operand class combinations each product is used with, value products within 338 q^2
MUL_CLASSES = [("N", "N"), ("W", "N"), ("Y", "N"), ("X", "N"), ("P", "N"), ("D", "N"), ("P", "P")]
DOT2_CLASSES = [("P", "D", "Y", "N"), ("N", "N", "N", "N")]     # 17 * 17 + 6 * 3 = 307
# two un-normalised operands with every limb at 3 * 2^29 - 1: the fullest column the header allows (63 * 2^58)
DOT2_FULLEST = ("N", "D", "D", "N")                              # 3 * 17 + 17 * 3 = 102


def product_cases(rng, n_random):
    """(op, records, check) for mul, sqr and dot2: random operands of every class combination, all-limbs-at-maximum
    operands and the special values"""
    out = {}
    recs = []
    for ca, cb in MUL_CLASSES:
        recs += [rand_elem(rng, ca) + rand_elem(rng, cb) for _ in range(n_random // len(MUL_CLASSES))]
        recs.append(max_elem(ca) + max_elem(cb))
        recs += [a + b for a in special_values(ca) for b in special_values(cb)]
    out[OP_MUL] = recs
    recs = [rand_elem(rng, "P") for _ in range(n_random)] + [max_elem("P"), max_elem("N")] + special_values("P")
    out[OP_SQR] = recs
    recs = []
    for cs in DOT2_CLASSES + [DOT2_FULLEST]:
        recs += [sum((rand_elem(rng, c) for c in cs), []) for _ in range(n_random // 3)]
        recs.append(sum((max_elem(c) for c in cs), []))
    sp = special_values("N")
    recs += [a + b + b + a for a in sp for b in sp]
    out[OP_DOT2] = recs
    return out


def product_expected(op, rec):
    v = [value(rec[9 * i:9 * i + 9]) for i in range(len(rec) // 9)]
    if op == OP_MUL:
        return v[0] * v[1] * RINV % Q
    if op == OP_SQR:
        return v[0] * v[0] * RINV % Q
    return (v[0] * v[1] + v[2] * v[3]) * RINV % Q


def check_product(op, rec, got):
    assert is_normalised(got), (op, rec, got)
    assert value(got) < 3 * Q, (op, rec, got)
    assert value(got) % Q == product_expected(op, rec), (op, rec, got)


def sub_cases(rng, n_random):
    """op 3: norm(a + (4q - b)), a, b of class N; op 7: norm(a + (14q - b)), a of class N, b of class X"""
    out = {}
    for op, cb in ((OP_SUB4, "N"), (OP_SUB14, "X")):
        recs = [rand_elem(rng, "N") + rand_elem(rng, cb) for _ in range(n_random)]
        recs += [max_elem("N") + max_elem(cb), limbs(0) + max_elem(cb), max_elem("N") + limbs(0)]
        recs += [a + b for a in special_values("N") for b in special_values(cb)]
        out[op] = recs
    return out


def check_sub(op, rec, got):
    a, b = value(rec[:9]), value(rec[9:])
    k = 4 if op == OP_SUB4 else 14
    assert is_normalised(got), (op, rec, got)
    assert value(got) == a + k * Q - b, (op, rec, got)      # exactly: nothing is reduced, nothing goes negative


def relimb_cases(rng, n_random):
    vals = [rng.randrange(1 << 256) for _ in range(n_random)]
    vals += [0, 1, Q - 1, Q, 2 * Q - 1, (1 << 256) - 1, 1 << 255, M29, 1 << 29, (1 << 232) - 1, 1 << 232]
    return [list(struct.unpack("<8I", v.to_bytes(32, "little"))) for v in vals]


def check_relimb(rec, got):
    v = int.from_bytes(struct.pack("<8I", *rec), "little")
    assert got[:9] == limbs(v), (rec, got)
    assert got[9:] == rec, (rec, got)


# ---- G1 --------------------------------------------------------------------------------------------------------
def wire(v):
    """field element -> the 8 words of its wire form (Montgomery, radix 2^256)"""
    return list(struct.unpack("<8I", (v * bn.MONT_R % Q).to_bytes(32, "little")))


def affine_words(P):
    return [0] * 16 if P is None else wire(P[0]) + wire(P[1])


def xyzz_words(P, rng=None):
    """a wire XYZZ representative of P: (x zz, y zzz, zz, zzz) with zz = t^2, zzz = t^3 for a random t (1 without rng)"""
    if P is None:
        return [0] * 32
    t = rng.randrange(1, Q) if rng else 1
    zz, zzz = t * t % Q, t * t * t % Q
    return wire(P[0] * zz % Q) + wire(P[1] * zzz % Q) + wire(zz) + wire(zzz)


def xyzz_point(words):
    """wire XYZZ words (any representative below 2^256) -> affine point or None"""
    inv = pow(bn.MONT_R, -1, Q)
    x, y, zz, zzz = (int.from_bytes(struct.pack("<8I", *words[8 * i:8 * i + 8]), "little") * inv % Q for i in range(4))
    if zz == 0:
        return None
    assert pow(zz, 3, Q) == zzz * zzz % Q
    return (x * pow(zz, -1, Q) % Q, y * pow(zzz, -1, Q) % Q)


def signed(P, neg):
    return bn.ec_neg(P, bn.FQ) if (neg and P is not None) else P


def g1_points(rng, n):
    """n distinct random multiples of the generator, by a chain of additions"""
    step = bn.g1_mul(bn.G1_GEN, rng.randrange(1, bn.R))
    P = bn.g1_mul(bn.G1_GEN, rng.randrange(1, bn.R))
    out = []
    for _ in range(n):
        out.append(P)
        P = bn.g1_add(P, step)
    return out
