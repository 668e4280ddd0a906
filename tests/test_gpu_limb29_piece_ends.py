"""The two ends of a G1 piece on the device (csrc/fq29.hip.h: xyzz29_open multiplies the wire words by 32 and
g1piece29_close divides ZZ, ZZZ by 32, neither by a Montgomery product): short pieces through zkpoa_fq29_prim, where the
opening and the closing are most of the work -- lengths 1, 2 and 3 with each sign, an infinity base first and last,
and the accumulator meeting +-base at position 1 (the earliest a piece can be poisoned, so that the poison goes through
the closing division and the piece is redone exactly) -- and small MSMs with a forced narrow window and pieces of at
most 8, where pieces of length 1 and 2 and their partial-sum levels occur, against the C oracle."""
import random

import pytest

from conftest import le
from oracle import c_oracle as co
from oracle.py import bn254 as bn
import limb29_ref as lr
import limb29_packed_ref as pr

pytestmark = pytest.mark.gpu

Q = lr.Q
SLOTS = 8           # OP_PIECE and OP_PIECE_PACKED take 8 bases; a shorter piece is filled up with infinity bases


def run(ctx, op, records, out_words):
    return lr.unpack(ctx.fq29_prim(op, lr.pack(records), len(records), out_words), out_words)


def short_pieces():
    """[(sequence of (point or None, negate flag), redo expected)], every sequence SLOTS long"""
    rng = random.Random(251)
    P, S, T = (bn.g1_mul(bn.G1_GEN, rng.randrange(1, bn.R)) for _ in range(3))
    inf = (None, 0)
    seqs = []
    for n in (1, 2, 3):
        for signs in range(1 << n):
            seq = [(B, (signs >> i) & 1) for i, B in enumerate((P, S, T)[:n])]
            seqs.append((seq + [inf] * (SLOTS - n), 0))                    # the piece, then nothing
            seqs.append(([inf] + seq + [inf] * (SLOTS - n - 1), 0))        # an infinity base first
            seqs.append(([inf] * (SLOTS - n - 1) + seq + [(None, 1)], 0))  # the piece at the end, an infinity base last
    for s in (0, 1):
        for t in (0, 1):                                                   # acc = +-base at position 1
            seqs.append(([(P, s), (P, t)] + [inf] * (SLOTS - 2), 1))
            seqs.append(([(P, s), (pr.neg(P), t), (S, 0)] + [inf] * (SLOTS - 3), 1))
            seqs.append(([inf, (P, s), (P, t), (T, 1)] + [inf] * (SLOTS - 4), 1))
    return seqs


def expected(seq):
    want = None
    for B, f in seq:
        want = bn.g1_add(want, lr.signed(B, f))
    return want


def records(seqs):
    return [sum((lr.affine_words(B) + [f] for B, f in seq), []) for seq, _ in seqs]


def test_short_pieces_canonical(ctx):
    seqs = short_pieces()
    for (seq, _), got in zip(seqs, run(ctx, lr.OP_PIECE, records(seqs), 32)):
        for c in range(4):
            assert pr.word_value(got[8 * c:8 * c + 8]) < Q, seq
        assert lr.xyzz_point(got) == expected(seq), seq


def test_short_pieces_packed(ctx):
    seqs = short_pieces()
    for (seq, redo), got in zip(seqs, run(ctx, pr.OP_PIECE_PACKED, records(seqs), 36)):
        want = expected(seq)
        assert pr.packed_point(got[:32]) == want, seq
        assert got[32:] == [redo, 0, 0, 0], seq
        if want is None:
            assert got[:32] == [0] * 32, seq
        elif not redo:                          # closed by the division: ZZ, ZZZ below 1.0625 q, X below 2^256
            assert 16 * pr.word_value(got[16:24]) < 17 * Q and 16 * pr.word_value(got[24:32]) < 17 * Q, seq


@pytest.mark.parametrize("n", [1, 2, 63, 70])
def test_small_msm_with_pieces_of_one_and_two(ctx, n):
    """c = 4: eight buckets a window, so 63 and 70 points leave about 8 entries a bucket in each of the 64 windows,
    some above: a piece of 8 and a short one (1, 2, ...) joined by a partial-sum level, others below: one short piece;
    1 and 2 points are pieces of length 1 only"""
    import torch
    rng = random.Random(257 + n)
    bases = co.fixed_base_g1(b"".join(le(rng.randrange(bn.R)) for _ in range(n)), 8)
    scal = b"".join(le(rng.choice([rng.randrange(bn.R), bn.R - 1 - rng.randrange(1 << 20), rng.randrange(1 << 64)]))
                    for _ in range(n))
    want = co.msm_g1(bases, scal, n, 8)
    d_b = torch.frombuffer(bytearray(bases), dtype=torch.uint8).cuda()
    d_s = torch.frombuffer(bytearray(scal), dtype=torch.uint8).cuda()
    ctx.set_option("msm_c", 4)
    ctx.set_option("msm_k0", 8)
    try:
        got = ctx.msm_g1_device(d_b.data_ptr(), d_s.data_ptr(), n)
    finally:
        ctx.set_option("msm_k0", 0)
        ctx.set_option("msm_c", 0)
    assert got == want
