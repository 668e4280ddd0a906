"""zk-proof-of-assets_amd/csrc/fq29.hip.h on the CPU (tools/limb29_check.cpp, g++ -DZKPOA_LIMB29_CHECK: every column
addition checked for leaving 64 bits), for the two things the header's QUOTIENT LIMBS paragraph and its piece ends rest on:
  * fq29_mul and fq29_sqr keep the quotient limbs m_0..m_7 as 32-bit values. The operands here have every limb within
    2^12 of the most its class allows AND are searched, column by column, so that lo32(acc) * INV has its top three bits
    set in each of the columns 0..7: the largest m the code can meet on the largest products. Plus 10^5 random operands.
    The result has to be the exact integer (a b + Mt q) / 2^261 of a Python restatement, normalised and below 3q.
  * a piece opens by fq29_times32 and closes by fq29_div32 instead of Montgomery products: bounds and classes as the
    header states them, and what a poisoned ZZ (0, q, 2q) closes to.
The overflow counter must stay 0 throughout."""
import os
import random
import struct
import subprocess

import pytest

from conftest import ROOT
from oracle.py import bn254 as bn
import limb29_ref as lr
import limb29_packed_ref as pr

Q = lr.Q
M29 = lr.M29
INV = 0x04866389                      # -1/q mod 2^29
QL = lr.limbs(Q)
OP_TIMES32, OP_DIV32 = 15, 16
SEARCH = 1 << 12                      # a crafted limb lies within this of its class's largest limb
N_OPERANDS = 100000
# 6q in the borrowed form the kernels negate a wire word with (Fq29C6): limbs 0..7 >= 2^29 - 1, limb 8 >= 2^24 - 1
C6 = [0x32edefaa, 0x261a4447, 0x2aafd3d9, 0x30fed0e4, 0x212318cf, 0x31238483, 0x23e94785, 0x3628e537, 0x012259d5]


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("limb29u") / "limb29_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-DZKPOA_LIMB29_CHECK", "-I",
                    os.path.join(ROOT, "zk-proof-of-assets_amd", "csrc"), os.path.join(ROOT, "tools", "limb29_check.cpp"),
                    "-o", out], check=True, capture_output=True, text=True)
    return out


def run(check_bin, op, records, out_words):
    data = struct.pack("<I", len(records)) + lr.pack(records)
    rc = subprocess.run([check_bin, str(op)], input=data, capture_output=True, timeout=300)
    assert rc.returncode == 0
    assert len(rc.stdout) == 4 * out_words * len(records) + 8
    assert struct.unpack("<Q", rc.stdout[-8:])[0] == 0          # no column left 64 bits
    return lr.unpack(rc.stdout[:-8], out_words)


# ---- the product, restated: columns 0..8 as the header adds them, m_0..m_7 unmasked -------------------------------
def column(a, b, m, k, carry):
    """column k < 9 of a * b before its own m is added: carry + sum a_i b_(k-i) + sum m_i q_(k-i)"""
    acc = carry
    for i in range(k + 1):
        acc += a[i] * b[k - i]
    for i in range(k):
        acc += m[i] * QL[k - i]
    return acc


def quotient(a, b):
    """([mt_0..mt_7, m_8], the largest column sum of columns 0..8)"""
    m, carry, top = [], 0, 0
    for k in range(9):
        acc = column(a, b, m, k, carry)
        mk = ((acc & 0xffffffff) * INV) & 0xffffffff
        if k == 8:
            mk &= M29
        m.append(mk)
        acc += mk * QL[0]
        top = max(top, acc)
        assert acc & M29 == 0
        carry = acc >> 29
    return m, top


def exact_product(a, b):
    m, top = quotient(a, b)
    assert top < (1 << 64)
    total = lr.value(a) * lr.value(b) + lr.value(m) * Q
    assert total % (1 << 261) == 0
    return total >> 261, m


def craft(ca, cb, square=False):
    """operands of the classes with every limb 0..7 within SEARCH of the class's largest, limb 8 the largest the value
    bound leaves, and limb k of a chosen so that column k's unmasked m has its top three bits set (k = 0..7)"""
    a, b = lr.max_elem(ca), (None if square else lr.max_elem(cb))
    m, carry = [], 0
    for k in range(8):
        hi = a[k]
        for d in range(SEARCH):
            a[k] = hi - d
            acc = column(a, a if square else b, m, k, carry)
            mk = ((acc & 0xffffffff) * INV) & 0xffffffff
            if mk >> 29 == 7:
                break
        else:
            raise AssertionError("no limb found for column %d" % k)
        m.append(mk)
        carry = (acc + mk * QL[0]) >> 29
    return a, (a if square else b)


def check_exact(a, b, got):
    want, m = exact_product(a, b)
    assert lr.is_normalised(got), (a, b, got)
    assert lr.value(got) == want, (a, b, got)
    assert want < 3 * Q, (a, b, got)
    assert want % Q == lr.value(a) * lr.value(b) * lr.RINV % Q
    return m


def test_mul_crafted_largest_quotient_limbs(check_bin):
    pairs = [craft(ca, cb) for ca, cb in lr.MUL_CLASSES] + [craft(cb, ca)[::-1] for ca, cb in lr.MUL_CLASSES]
    for (ca, cb), (a, b) in zip(lr.MUL_CLASSES + lr.MUL_CLASSES, pairs):
        for cls, l in ((ca, a), (cb, b)):
            lb, vb = lr.CLASSES[cls]
            assert all(lb - SEARCH <= x < lb for x in l[:8]) and lr.value(l) < vb
        assert lr.value(a) * lr.value(b) <= 338 * Q * Q
    got = run(check_bin, lr.OP_MUL, [a + b for a, b in pairs], 9)
    for (a, b), g in zip(pairs, got):
        m = check_exact(a, b, g)
        assert all(x >> 29 == 7 for x in m[:8]), (a, b, m)      # the search did what it is for


def test_sqr_crafted_largest_quotient_limbs(check_bin):
    ops = [craft(c, c, square=True)[0] for c in ("P", "N", "X", "W")]
    got = run(check_bin, lr.OP_SQR, ops, 9)
    for a, g in zip(ops, got):
        m = check_exact(a, a, g)
        assert all(x >> 29 == 7 for x in m[:8]), (a, m)


def test_column_bound_of_the_header():
    """the header's COLUMNS arithmetic: 2^32 (q_0 + ... + q_8) plus the a b part and a carry stays inside 64 bits"""
    assert sum(QL) == 1616751127
    m_part = (1 << 32) * sum(QL)
    assert m_part < 0.377 * 2 ** 64
    assert m_part + 9 * (1 << 58) + (1 << 35) < 0.52 * 2 ** 64
    assert m_part + 27 * (1 << 58) + (1 << 35) < 0.80 * 2 ** 64
    mt = (1 << 261) + (1 << 32) * ((1 << 232) - 1) // M29
    assert mt * 2 ** 25.9 < (1 << 261) * (2 ** 25.9 + 1)
    assert 338 * Q * Q // (1 << 261) + Q + (Q >> 25) < 3 * Q


def test_products_of_random_operands(check_bin):
    """10^5 random operands through mul (every class pair the rules allow) and 10^5 through sqr"""
    rng = random.Random(229)
    n = N_OPERANDS // (2 * len(lr.MUL_CLASSES)) + 1
    recs = [(lr.rand_elem(rng, ca), lr.rand_elem(rng, cb)) for ca, cb in lr.MUL_CLASSES for _ in range(n)]
    assert 2 * len(recs) >= N_OPERANDS
    for (a, b), g in zip(recs, run(check_bin, lr.OP_MUL, [a + b for a, b in recs], 9)):
        lr.check_product(lr.OP_MUL, a + b, g)
    for a, b in recs[::997]:                                    # the restatement agrees with the definition
        assert exact_product(a, b)[0] % Q == lr.value(a) * lr.value(b) * lr.RINV % Q
    sq = [lr.rand_elem(rng, "P") for _ in range(N_OPERANDS)]
    for a, g in zip(sq, run(check_bin, lr.OP_SQR, sq, 9)):
        lr.check_product(lr.OP_SQR, a, g)
    for a, g in list(zip(sq, run(check_bin, lr.OP_SQR, sq[:64], 9))):
        assert lr.value(g) == exact_product(a, a)[0]


# ---- piece ends -----------------------------------------------------------------------------------------------
def wire_words(rng):
    vals = [0, 1, Q - 1, Q, (1 << 256) - 1, Q + 1, 2 * Q, 5 * Q, 5 * Q + 1, (1 << 255), (1 << 232) - 1, 1 << 232]
    vals += [(k * ((Q >> 232) + 1) << 232) // 32 + e for k in (1, 2, 160, 169) for e in (-1, 0, 1)]   # estimate's edges
    vals += [rng.randrange(1 << 256) for _ in range(4000)] + [rng.randrange(Q) for _ in range(1000)]
    return [v for v in vals if 0 <= v < (1 << 256)]


def test_piece_opens_by_times32(check_bin):
    assert lr.value(C6) == 6 * Q and all(c >= M29 for c in C6[:8]) and C6[8] >= (1 << 24) - 1
    vals = wire_words(random.Random(233))
    recs = [lr.limbs(v) for v in vals]
    negs = [[c - x for c, x in zip(C6, lr.limbs(v))] for v in vals]     # C6 - W: limbs < 2^30, value 6q - w
    assert all(0 <= x < (1 << 30) for l in negs for x in l)
    got = run(check_bin, OP_TIMES32, recs + negs, 9)
    bound = Q + 194 * (1 << 232)
    assert bound < 3 * Q and bound < Q + (Q >> 13)
    for v, g in zip(vals + [6 * Q - v for v in vals], got):
        r = lr.value(g)
        assert lr.is_normalised(g), (v, g)
        assert r < bound, (v, g)                                # class N (Y) and class X at once
        assert r <= 32 * v and (32 * v - r) % Q == 0, (v, g)     # the same element: k q taken off, nothing negative
        assert g[8] < (1 << 26)


def test_piece_closes_by_div32(check_bin):
    rng = random.Random(239)
    vals = [0, Q, 2 * Q, 1, Q - 1, Q + 1, 2 * Q - 1, 2 * Q + 1, 3 * Q - 1, (1 << 266) % Q, 31, 32, 33]
    vals += [rng.randrange(3 * Q) for _ in range(5000)]
    got = run(check_bin, OP_DIV32, [lr.limbs(v) for v in vals] + [lr.max_elem("N")], 9)
    for v, g in zip(vals + [lr.value(lr.max_elem("N"))], got):
        m = (-v * pow(Q, -1, 32)) % 32
        assert lr.is_normalised(g), (v, g)
        assert lr.value(g) == (v + m * Q) >> 5 and (v + m * Q) % 32 == 0, (v, g)
        assert lr.value(g) * 32 % Q == v % Q
        assert 16 * lr.value(g) < 17 * Q                        # below 1.0625 q: class N with room
    for v, g in zip(vals[:3], got[:3]):                         # poison closes to 0 or q, nothing else
        assert lr.value(g) in (0, Q), (v, g)
    assert [lr.value(g) for g in got[:3]] == [0, Q, Q]


def test_pieces_through_both_ends(check_bin):
    """pieces of length 1, 2 and 3 with each sign, infinity first and last, closed into the packed form; acc = +-base
    at position 1 is reported as poisoned with ZZ = 0 or q"""
    rng = random.Random(241)
    P, S, T = (bn.g1_mul(bn.G1_GEN, rng.randrange(1, bn.R)) for _ in range(3))
    seqs = [[(P, s)] for s in (0, 1)]
    seqs += [[(P, s), (S, t)] for s in (0, 1) for t in (0, 1)]
    seqs += [[(P, s), (S, t), (T, u)] for s in (0, 1) for t in (0, 1) for u in (0, 1)]
    seqs += [[(None, 0), (P, 1)], [(P, 1), (None, 1)], [(None, 1), (P, 0), (S, 1), (None, 0)]]
    bad = [[(P, s), (P, t)] for s in (0, 1) for t in (0, 1)] + [[(P, 0), (P, 1), (S, 0)], [(None, 0), (P, 1), (P, 1), (T, 0)]]
    rec = lambda seq: [len(seq)] + sum((lr.affine_words(p) + [s] for p, s in seq), [])
    got = run(check_bin, pr.OP_PIECE_PACKED, [rec(s) for s in seqs + bad], 33)
    for seq, g in zip(seqs, got):
        want = None
        for p, s in seq:
            want = bn.g1_add(want, lr.signed(p, s))
        assert g[32] == 1 and pr.packed_point(g[:32]) == want, seq
        assert pr.word_value(g[16:24]) < Q + Q // 16 and pr.word_value(g[24:32]) < Q + Q // 16
    for g in got[len(seqs):]:
        assert g[32] == 0 and pr.word_value(g[16:24]) in (0, Q)
