"""The G1 MSM's partial sums in the packed 29-bit form (csrc/fq29.hip.h, csrc/msm.hip.h): the device functions of the
partial-sum levels and the bucket reduction through zkpoa_fq29_prim (packed + packed -> packed with the infinity flags and
the exact redo, a piece closed into the packed form, packed -> canonical wire XYZZ), and whole MSMs whose inputs make equal
and opposite partial sums and infinities meet in every kernel -- the piece close, the partial-sum levels, the row and
column sums, the per-bit trees and the tree over more than 256 columns -- in the classic and the fixed-base form.
Expected values come from oracle/py (points) and the C oracle (MSMs)."""
import ctypes
import random
import struct

import pytest

from conftest import le
from oracle import c_oracle as co
from oracle.py import bn254 as bn
from oracle.py import groth16 as g16
import limb29_ref as lr
import limb29_packed_ref as pr

pytestmark = pytest.mark.gpu

Q = lr.Q
N_PAIRS = 4096


def run(ctx, op, records, out_words):
    return lr.unpack(ctx.fq29_prim(op, lr.pack(records), len(records), out_words), out_words)


@pytest.fixture(scope="module")
def points():
    return lr.g1_points(random.Random(101), N_PAIRS + 8)


# ---- a. the device functions ---------------------------------------------------------------------------------------
def test_packed_addition_random_pairs(ctx, points):
    """4096 pairs, every coordinate a random representative below 2^256 (ZZ below 3q): the generic addition, no redo"""
    rng = random.Random(103)
    perm = list(range(N_PAIRS))
    rng.shuffle(perm)
    pairs = [(points[i], points[j]) for i, j in enumerate(perm) if i != j]
    assert len(pairs) >= N_PAIRS - 8
    recs = [pr.packed_words(a, rng) + pr.packed_words(b, rng) for a, b in pairs]
    for (a, b), got in zip(pairs, run(ctx, pr.OP_PACKED_ADD, recs, 36)):
        assert pr.packed_point(got[:32]) == bn.g1_add(a, b)
        assert got[32:] == [0, 0, 0, 0]


def test_packed_addition_special_pairs(ctx, points):
    """P + P, P + (-P), infinity on either side and on both, and the 3q-representatives of one point against each
    other: the flag says whether the exact addition redid the sum, and poison is never what comes back"""
    rng = random.Random(107)
    P, S = points[0], points[1]
    inf = [0] * 32
    cases = []                                              # (a words, b words, expected point, redo expected)
    for _ in range(4):
        cases.append((pr.packed_words(P, rng), pr.packed_words(P, rng), bn.g1_add(P, P), 1))
        cases.append((pr.packed_words(P, rng), pr.packed_words(pr.neg(P), rng), None, 1))
        cases.append((inf, pr.packed_words(P, rng), P, 0))
        cases.append((pr.packed_words(P, rng), inf, P, 0))
        cases.append((pr.packed_words(P, rng), pr.packed_words(S, rng), bn.g1_add(P, S), 0))
    cases.append((inf, inf, None, 0))
    for t in (1, 7):
        for j in range(3):
            for k in range(3):                              # the same words but for multiples of q; and another t
                cases.append((pr.packed_words(P, t=t, rep=j), pr.packed_words(P, t=t, rep=k), bn.g1_add(P, P), 1))
                cases.append((pr.packed_words(P, t=t, rep=j), pr.packed_words(P, t=t + 1, rep=k), bn.g1_add(P, P), 1))
                cases.append((pr.packed_words(P, t=t, rep=j), pr.packed_words(pr.neg(P), t=t, rep=k), None, 1))
                cases.append((pr.packed_words(S, t=t, rep=j), pr.packed_words(P, t=t, rep=k), bn.g1_add(S, P), 0))
    got = run(ctx, pr.OP_PACKED_ADD, [a + b for a, b, _, _ in cases], 36)
    for (a, b, want, redo), g in zip(cases, got):
        assert pr.packed_point(g[:32]) == want, (a, b)
        assert g[32:] == [redo, 0, 0, 0], (a, b)
        if want is None:
            assert g[:32] == inf                            # a sum that is infinity is stored as all-zero


def test_piece_closes_into_the_packed_form(ctx, points):
    """pieces of 8 bases as msm_accum0_kernel sums and closes them: generic ones, the accumulator meeting its own value
    or its opposite at the first possible, a middle and the last position, infinity bases, nothing but infinity, a
    piece that sums to infinity"""
    rng = random.Random(109)
    # independent multiples of the generator: lr.g1_points is an arithmetic progression, and a signed sum of its members
    # can be another member -- an exceptional case nobody asked for
    indep = [bn.g1_mul(bn.G1_GEN, rng.randrange(1, bn.R)) for _ in range(24)]
    A = indep[:8]

    def prefix(k):
        acc = None
        for P in A[:k]:
            acc = bn.g1_add(acc, P)
        return acc
    pieces = [([(P, rng.randrange(2)) for P in rng.sample(indep[8:], 8)], 0) for _ in range(24)]
    for pos in (1, 4, 7):
        for minus in (0, 1):
            for flag in (0, 1):
                seq = [(P, 0) for P in A]
                seq[pos] = (pr.neg(prefix(pos)) if minus ^ flag else prefix(pos), flag)
                pieces.append((seq, 1))
    for pos in (0, 3, 7):
        seq = [(P, rng.randrange(2)) for P in A]
        seq[pos] = (None, pos & 1)
        pieces.append((seq, 0))
    pieces.append(([(None, 0)] * 8, 0))
    pieces.append(([(A[0], 0)] * 8, 1))
    pieces.append(([(A[0], k & 1) for k in range(8)], 1))
    pieces.append(([(P, 0) for P in A[:7]] + [(prefix(7), 1)], 1))
    pieces.append(([(None, 0)] * 7 + [(A[2], 1)], 0))
    recs = [sum((lr.affine_words(P) + [f] for P, f in seq), []) for seq, _ in pieces]
    for (seq, redo), g in zip(pieces, run(ctx, pr.OP_PIECE_PACKED, recs, 36)):
        want = None
        for P, f in seq:
            want = bn.g1_add(want, lr.signed(P, f))
        assert pr.packed_point(g[:32]) == want, seq
        assert g[32:] == [redo, 0, 0, 0], seq


def test_packed_to_wire(ctx, points):
    """what the last kernel of the reduction writes for the host: canonical wire XYZZ of the same point"""
    rng = random.Random(113)
    pts = points[100:356] + [None]
    recs = [pr.packed_words(P, rng) for P in pts]
    pts += [points[5]] * 3
    recs += [pr.packed_words(points[5], t=3, rep=k) for k in range(3)]
    for P, got in zip(pts, run(ctx, pr.OP_PACKED_TO_WIRE, recs, 32)):
        for c in range(4):
            assert pr.word_value(got[8 * c:8 * c + 8]) < Q
        assert lr.xyzz_point(got) == P
        if P is None:
            assert got == [0] * 32


def test_a_sum_goes_through_every_form(ctx, points):
    """piece -> packed, + packed -> packed, -> wire: the chain of forms one bucket's sum passes through"""
    rng = random.Random(127)
    seqs = [[(P, rng.randrange(2)) for P in rng.sample(points[200:300], 8)] for _ in range(64)]
    sums = []
    for seq in seqs:
        acc = None
        for P, f in seq:
            acc = bn.g1_add(acc, lr.signed(P, f))
        sums.append(acc)
    closed = [g[:32] for g in run(ctx, pr.OP_PIECE_PACKED, [sum((lr.affine_words(P) + [f] for P, f in s), []) for s in seqs], 36)]
    added = [g[:32] for g in run(ctx, pr.OP_PACKED_ADD, [closed[i] + closed[i + 1] for i in range(0, 64, 2)], 36)]
    for i, got in enumerate(run(ctx, pr.OP_PACKED_TO_WIRE, added, 32)):
        assert lr.xyzz_point(got) == bn.g1_add(sums[2 * i], sums[2 * i + 1])


# ---- b. whole MSMs ---------------------------------------------------------------------------------------------------
K0 = 8          # the smallest piece length the option accepts


def msm_plan(zk, n, c, k0, merged=0):
    f = zk.lib().zkpoa_test_msm_plan
    out = (ctypes.c_uint64 * 13)()
    assert f(n, c, merged, 0, None, k0, out, 13) == 13
    return dict(zip(("c", "W", "Wb", "ne", "TB", "K0", "K", "logS", "logRows"), out))


def build_input(n):
    """Bases from {P, -P, T, -T, infinity}, scalars from seven full-width values and their opposites: s and r - s fall
    into the same bucket of every window with opposite signs. Every scalar class gets the SAME list of bases, so the
    buckets of s1..s4 hold one value V, those of r - s5, r - s6 hold -V, and s7 with r - s7 cancels to infinity through
    equal and opposite piece sums; every piece, bucket, row and column sum is a small multiple of P plus one of T. An
    eighth of the points draw base and scalar freely from the same sets, and a sixteenth is an ordinary random block."""
    rng = random.Random(131 + n)
    fb = co.fixed_base_g1(b"".join(le(rng.randrange(bn.R)) for _ in range(n // 16 + 2)), 8)
    base = lambda i: fb[64 * i:64 * i + 64]
    negb = lambda b: g16.g1_to_bytes(bn.ec_neg(g16.g1_from_bytes(b), bn.FQ))
    P, T = base(n // 16), base(n // 16 + 1)
    kinds = [P, negb(P), T, negb(T), bytes(64)]
    s = [rng.randrange(1, bn.R) for _ in range(7)]
    classes = s[:4] + [bn.R - s[4], bn.R - s[5], s[6], bn.R - s[6]]
    structured = n - n // 8 - n // 16
    per = structured // len(classes)
    shared = [rng.choice(kinds) for _ in range(per)]
    items = [(b, k) for k in classes for b in shared]
    every = s + [bn.R - v for v in s] + [0, 1, bn.R - 1]
    items += [(rng.choice(kinds), rng.choice(every)) for _ in range(n - n // 16 - len(items))]
    items += [(base(i), rng.randrange(bn.R)) for i in range(n // 16)]
    assert len(items) == n
    rng.shuffle(items)
    bases = b"".join(b for b, _ in items)
    scal = b"".join(le(k) for _, k in items)
    return bases, scal, n, co.msm_g1(bases, scal, n, 8)


@pytest.fixture(scope="module")
def msm_input():
    return build_input(1 << 12)


def forced_msm(ctx, bases, scal, n, c):
    ctx.set_option("msm_c", c)
    ctx.set_option("msm_k0", K0)
    try:
        return ctx.msm_g1(bases, scal, n)
    finally:
        ctx.set_option("msm_k0", 0)
        ctx.set_option("msm_c", 0)


@pytest.mark.parametrize("c", [4, 8, 13])
def test_msm_equal_and_opposite_sums_at_every_level(zk, ctx, msm_input, c):
    """c = 4: 8 buckets per window, ~500 entries each: 64 pieces of 8 and three partial-sum levels; c = 8 and 13: shorter
    chains, more buckets per row and column sum"""
    bases, scal, n, want = msm_input
    plan = msm_plan(zk, n, c, K0)
    assert plan["c"] == c and plan["K0"] == K0
    if c == 4:
        pieces = -(-(n // 8) // K0)                                 # of one scalar class's share of a bucket, at least
        levels, k = 0, plan["K"]
        while pieces > 1:
            pieces, levels = -(-pieces // k), levels + 1
        assert levels >= 3
    assert forced_msm(ctx, bases, scal, n, c) == want


def test_msm_more_than_256_columns(zk, ctx):
    """the smallest forced window whose plan has more than 256 columns, so that msm_tree_sum_kernel finishes the sums"""
    n = 1 << 10
    c = next(c for c in range(4, 23) if msm_plan(zk, n, c, K0)["logS"] > 8)
    assert msm_plan(zk, n, c, K0)["c"] == c
    bases, scal, _, want = build_input(n)
    assert forced_msm(ctx, bases, scal, n, c) == want


def test_msm_fixed_base_form(ctx, msm_input):
    """the same inputs through a fixed-base table: one bucket set for all windows, so sums of different windows meet"""
    import torch
    bases, scal, n, want = msm_input
    d_b = torch.frombuffer(bytearray(bases), dtype=torch.uint8).cuda()
    d_s = torch.frombuffer(bytearray(scal), dtype=torch.uint8).cuda()
    ctx.set_option("msm_k0", K0)
    table = ctx.msm_table(1, d_b.data_ptr(), n, 8)
    try:
        assert table.info()[1] == 8
        assert ctx.msm_table_run(table, d_s.data_ptr()) == want
    finally:
        table.close()
        ctx.set_option("msm_k0", 0)
