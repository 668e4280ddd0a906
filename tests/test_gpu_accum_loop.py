"""The control flow of the G1 accumulation loop (msm_accum0_kernel, 29-bit branch): it is unrolled by two, holds the
current and the prefetched base in two register sets that swap roles, and reads `sorted` through a 16-byte block
cache. G1 MSMs with c = 4 and K0 = 8 forced, against the C oracle: pieces of every length 1..8 (a bucket of 9 entries
is a full piece and a piece of one), starting at every offset mod 4 of `sorted`, so the block cache is entered at each
position and crossed at both parities of the unroll; an infinity base at every position of an odd and an even piece;
a repeated base, so that the redo with the exact addition runs after the unrolled loop.

A scalar d << 4w with 1 <= d <= 7 has the one signed digit d, in window w: the point lands in bucket d of window w and
nowhere else, so the bucket sizes below are the piece lengths."""
import random

import pytest

from conftest import le
from oracle import c_oracle as co
from oracle.py import bn254 as bn

pytestmark = pytest.mark.gpu

C, K0 = 4, 8
COUNTS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33, 257]
# bucket sizes in the order of `sorted` (seven buckets, digits 1..7, per window): every length 1..9, and the running sum
# of the sizes -- where a bucket's first piece starts -- puts every piece length 1..8 at every offset mod 4 within the
# first 257 entries (test_schedule_has_every_length_and_offset)
SIZES = [1, 2, 3, 4, 5, 6, 7,
         9, 9, 9, 9, 2, 2, 3, 2, 2, 3, 3, 3, 4, 5, 4, 5, 4, 5, 4, 5, 6, 6, 7, 6, 6, 7, 7, 7,
         8, 9, 1, 3, 2, 5, 4, 9, 7, 8, 6, 2, 1, 3, 4, 9, 8, 7, 5, 3, 6]


@pytest.fixture(scope="module")
def pool():
    """257 distinct affine bases, made once"""
    rng = random.Random(2929)
    n = 257
    b = co.fixed_base_g1(b"".join(le(rng.randrange(bn.R)) for _ in range(n)), 8)
    return [b[64 * i:64 * i + 64] for i in range(n)]


def schedule(n):
    """the single-digit scalars of n points: SIZES filled in order, cut at n"""
    out = []
    for i, size in enumerate(SIZES):
        out += [(i % 7 + 1) << (C * (i // 7))] * size
    assert len(out) >= n
    return out[:n]


def msm_checked(ctx, bases, scalars):
    n = len(bases)
    b, s = b"".join(bases), b"".join(le(k) for k in scalars)
    want = co.msm_g1(b, s, n, 4)
    ctx.set_option("msm_c", C)
    ctx.set_option("msm_k0", K0)
    try:
        got = ctx.msm_g1(b, s, n)
    finally:
        ctx.set_option("msm_k0", 0)
        ctx.set_option("msm_c", 0)
    assert got == want


def test_schedule_has_every_length_and_offset():
    """the input itself, no device: at 257 points every piece length 1..8 starts at every offset mod 4"""
    seen, off = set(), 0
    for size in SIZES:
        size = min(size, 257 - off)
        for j in range(0, size, K0):
            seen.add((min(K0, size - j), (off + j) % 4))
        off += size
    assert off == 257 and {(l, o) for l in range(1, 9) for o in range(4)} <= seen


@pytest.mark.parametrize("n", COUNTS)
def test_piece_lengths_and_offsets(ctx, pool, n):
    msm_checked(ctx, pool[:n], schedule(n))


def test_full_scalars_with_negated_bases(ctx, pool):
    """random 254-bit scalars: ~32 entries per bucket, pieces of 8 with negated bases at both parities"""
    rng = random.Random(4)
    msm_checked(ctx, pool, [rng.randrange(bn.R) for _ in pool])


@pytest.mark.parametrize("length", [7, 8])
def test_infinity_base_at_every_position(ctx, pool, length):
    """one piece of odd and of even length behind 0..3 other entries, the all-zero base at each of its positions in turn
    (the first, every middle one, the last), then at all of them"""
    for lead in range(4):
        scal = [1] * lead + [2] * length
        for pos in list(range(length)) + [None]:
            bases = list(pool[:lead + length])
            for i in range(length):
                if pos is None or i == pos:
                    bases[lead + i] = bytes(64)
            msm_checked(ctx, bases, scal)


@pytest.mark.parametrize("length", [2, 3, 7, 8, 9])
def test_repeated_base_redoes_the_piece(ctx, pool, length):
    """the same base in every entry of a piece (the second addition meets acc = base whatever the order), and the same
    base twice among distinct ones: the generic sum is poisoned and the piece is summed again, exactly"""
    for lead in range(4):
        scal = [1] * lead + [3] * length
        msm_checked(ctx, pool[:lead] + [pool[100]] * length, scal)
        for at in range(length - 1):
            bases = list(pool[:lead + length])
            bases[lead + at + 1] = bases[lead + at]
            msm_checked(ctx, bases, scal)
