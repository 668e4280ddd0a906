"""The 9 x 29-bit-limb field and the G1 sums built on it, on the device (zkpoa_fq29_prim), with the operand sets of
tests/limb29_ref.py -- the ones tests/test_limb29_host.py feeds the same header on the CPU -- and the MSM with piece
lengths, window widths and inputs chosen so that pieces meet repeated bases, opposite pairs and infinity bases at
their first, a middle and their last position."""
import random
import struct

import pytest

from conftest import le
from oracle import c_oracle as co
from oracle.py import bn254 as bn
from oracle.py import groth16 as g16
import limb29_ref as lr

pytestmark = pytest.mark.gpu

N = 4096


def run(ctx, op, records, out_words, raw=True):
    return lr.unpack(ctx.fq29_prim(op, lr.pack(records), len(records), out_words, raw=raw), out_words)


@pytest.mark.parametrize("op", [lr.OP_MUL, lr.OP_SQR, lr.OP_DOT2])
def test_products(ctx, op):
    recs = lr.product_cases(random.Random(29 + op), N)[op]
    assert len(recs) >= N - 8
    for rec, got in zip(recs, run(ctx, op, recs, 9)):
        lr.check_product(op, rec, got)


@pytest.mark.parametrize("op", [lr.OP_SUB4, lr.OP_SUB14])
def test_sub_norm(ctx, op):
    recs = lr.sub_cases(random.Random(31 + op), N)[op]
    for rec, got in zip(recs, run(ctx, op, recs, 9)):
        lr.check_sub(op, rec, got)


def test_relimb_round_trip_and_wire_operands(ctx):
    recs = lr.relimb_cases(random.Random(37), N)
    for rec, got in zip(recs, run(ctx, lr.OP_RELIMB, recs, 17)):
        lr.check_relimb(rec, got)
    # raw = 0: operands are 8-word values, re-limbed on load
    pairs = [recs[i] + recs[i + 1] for i in range(0, 256, 2)]
    for rec, got in zip(pairs, run(ctx, lr.OP_MUL, pairs, 9, raw=False)):
        a, b = (int.from_bytes(struct.pack("<8I", *rec[8 * j:8 * j + 8]), "little") for j in (0, 1))
        lr.check_product(lr.OP_MUL, lr.limbs(a) + lr.limbs(b), got)


def canonical_point(words):
    """canonical wire XYZZ words -> affine point, every coordinate asserted below q"""
    for c in range(4):
        assert int.from_bytes(struct.pack("<8I", *words[8 * c:8 * c + 8]), "little") < lr.Q
    return lr.xyzz_point(words)


def test_mixed_addition(ctx):
    """64 accumulator / base pairs, generic ones and: acc = base (doubling), acc = -base, through the negate flag too,
    an infinity base, an infinity accumulator, both"""
    rng = random.Random(53)
    pts = lr.g1_points(rng, 128)
    cases = []
    for i in range(0, 52, 2):
        cases.append((pts[i], pts[i + 1], rng.randrange(2)))
    P, S = pts[60], pts[61]
    cases += [(P, P, 0), (P, P, 1), (P, bn.ec_neg(P, bn.FQ), 0), (P, bn.ec_neg(P, bn.FQ), 1), (P, None, 0), (P, None, 1),
              (None, S, 0), (None, S, 1), (None, None, 0), (S, S, 0), (S, S, 1), (S, P, 0)]
    assert len(cases) >= 38
    cases += [(pts[64 + i], pts[65 + i], 1) for i in range(64 - len(cases))]
    assert len(cases) == 64
    recs = [lr.xyzz_words(a, rng) + lr.affine_words(b) + [s] for a, b, s in cases]
    for (a, b, s), got in zip(cases, run(ctx, lr.OP_MADD, recs, 32)):
        assert canonical_point(got) == bn.g1_add(a, lr.signed(b, s)), (a, b, s)


def test_full_addition(ctx):
    rng = random.Random(59)
    pts = lr.g1_points(rng, 64)
    cases = [(pts[i], pts[i + 1]) for i in range(0, 54)]
    P, S = pts[60], pts[61]
    cases += [(P, P), (P, bn.ec_neg(P, bn.FQ)), (bn.ec_neg(S, bn.FQ), S), (P, None), (None, S), (None, None), (S, S),
              (S, P), (P, S), (pts[62], pts[63])]
    assert len(cases) == 64
    recs = [lr.xyzz_words(a, rng) + lr.xyzz_words(b, rng) for a, b in cases]
    for (a, b), got in zip(cases, run(ctx, lr.OP_ADD, recs, 32)):
        assert canonical_point(got) == bn.g1_add(a, b), (a, b)


def test_piece_with_exceptional_cases_at_every_position(ctx):
    """A piece of 8 bases summed as the accumulation kernel sums it (generic additions in 29-bit limbs, ZZ tested once
    at the end, the piece redone with the exact addition on a hit). The accumulator meets its own value (doubling) or
    its opposite at the first possible, a middle and the last position; infinity bases at the first, a middle and the
    last position; one piece sums to infinity; one is nothing but one base; one is nothing but infinity."""
    rng = random.Random(67)
    A = lr.g1_points(rng, 8)
    neg = lambda P: bn.ec_neg(P, bn.FQ)

    def prefix_sum(k):
        acc = None
        for P in A[:k]:
            acc = bn.g1_add(acc, P)
        return acc
    pieces = []
    for pos in (1, 4, 7):                       # the base at `pos` equals +-(the sum of the bases before it)
        for sign in (0, 1):
            for flag in (0, 1):                 # through the point itself or through the negate flag
                seq = [(P, 0) for P in A]
                S = prefix_sum(pos)
                want_minus = sign ^ flag
                seq[pos] = (neg(S) if want_minus else S, flag)
                pieces.append(seq)
    for pos in (0, 3, 7):
        seq = [(P, rng.randrange(2)) for P in A]
        seq[pos] = (None, pos & 1)
        pieces.append(seq)
    pieces.append([(A[0], 0)] * 8)                                      # 8 A0: doubling, then additions
    pieces.append([(A[0], k & 1) for k in range(8)])                    # sums to infinity, passing through it 4 times
    pieces.append([(None, 0)] * 8)
    pieces.append([(None, 0)] * 6 + [(A[1], 0), (A[1], 0)])             # doubling as the last addition after infinities
    pieces.append([(P, 0) for P in A[:7]] + [(prefix_sum(7), 1)])       # the whole piece sums to infinity at its end
    pieces.append([(P, 1) for P in A])                                  # no exceptional case at all
    recs = [sum((lr.affine_words(P) + [f] for P, f in seq), []) for seq in pieces]
    for seq, got in zip(pieces, run(ctx, lr.OP_PIECE, recs, 32)):
        want = None
        for P, f in seq:
            want = bn.g1_add(want, lr.signed(P, f))
        assert canonical_point(got) == want, seq


def test_bad_op_is_an_error(zk, ctx):
    for op in (-1, 9):
        with pytest.raises(zk.ZkpoaError):
            ctx.fq29_prim(op, bytes(4 * 64), 1, 32)


# ---- the MSM ---------------------------------------------------------------------------------------------------
K0 = 8


@pytest.fixture(scope="module")
def msm_input():
    """n = 2^12 points. The order of the entries inside a bucket is the sort's, not the input's, so the input cannot
    choose the position inside a piece (test_piece_with_exceptional_cases_at_every_position does that); it plants
    groups that share one scalar -- and so one bucket in every window -- whose pieces consist of exceptional cases in
    whatever order they arrive:
      * 24 copies of one base T (three pieces' worth of nothing but T: doubling),
      * 8 x (T2, -T2) (opposite pairs and doublings),
      * 16 copies of T3 among 32 infinity bases (the second T3 of a piece falls on any position, behind infinities),
      * 40 more infinity bases with random scalars,
      * a base U and its opposite alone with their scalar: that bucket sums to infinity in every window,
      * scalars 0, 1 and r - 1 on ordinary bases, and 1200 bases drawn with signs from 40 distinct ones (repeats
        and opposite pairs in every bucket at c = 4 and 8), the rest distinct."""
    rng = random.Random(61)
    n = 1 << 12
    scal = b"".join(le(rng.randrange(bn.R)) for _ in range(n))
    bases = bytearray(co.fixed_base_g1(b"".join(le(rng.randrange(bn.R)) for _ in range(n)), 8))
    scal = bytearray(scal)
    pos = list(range(n))
    rng.shuffle(pos)
    it = iter(pos)

    def put(i, base, k):
        bases[64 * i:64 * i + 64] = base
        scal[32 * i:32 * i + 32] = le(k)

    def base_at(i):
        return bytes(bases[64 * i:64 * i + 64])

    def neg(b):
        return g16.g1_to_bytes(bn.ec_neg(g16.g1_from_bytes(b), bn.FQ))
    T, T2, T3, U = (base_at(pos[-1 - k]) for k in range(4))
    s1, s2, s3, s4 = (rng.randrange(bn.R) for _ in range(4))
    for _ in range(24):
        put(next(it), T, s1)
    for _ in range(8):
        put(next(it), T2, s2)
        put(next(it), neg(T2), s2)
    for _ in range(16):
        put(next(it), T3, s3)
    for _ in range(32):
        put(next(it), bytes(64), s3)
    for _ in range(40):
        i = next(it)
        put(i, bytes(64), int.from_bytes(scal[32 * i:32 * i + 32], "little"))
    put(next(it), U, s4)
    put(next(it), neg(U), s4)
    for k in (0, 1, bn.R - 1, 0, 1, bn.R - 1):
        put(next(it), base_at(next(it)), k)
    few = [base_at(next(it)) for _ in range(40)]
    for _ in range(1200):
        i = next(it)
        put(i, rng.choice(few) if rng.randrange(4) else neg(rng.choice(few)),
            int.from_bytes(scal[32 * i:32 * i + 32], "little"))
    bases, scal = bytes(bases), bytes(scal)
    return bases, scal, n, co.msm_g1(bases, scal, n, 8)


@pytest.mark.parametrize("c", [4, 8, 13])
def test_msm_pieces_meet_every_exceptional_case(ctx, msm_input, c):
    """c = 4: 64 windows of 8 buckets, ~500 entries per bucket: 64 pieces and three partial-sum levels; c = 8: ~32 per
    bucket, two levels; c = 13: one entry per bucket except where the input repeats a scalar digit."""
    bases, scal, n, want = msm_input
    ctx.set_option("msm_c", c)
    ctx.set_option("msm_k0", K0)
    try:
        got = ctx.msm_g1(bases, scal, n)
    finally:
        ctx.set_option("msm_k0", 0)
        ctx.set_option("msm_c", 0)
    assert got == want
