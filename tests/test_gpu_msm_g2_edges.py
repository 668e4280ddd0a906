"""The G2 MSM's accumulation and bucket reduction at their edges. G2 runs RedWire<Fq2>, msm_accum0_kernel<Fq2> and its own
instantiations of the partial-sum levels, the row and column sums, the per-bit trees and the tree over more than 256
columns; the G1 MSM runs other code since its sums moved to 29-bit limbs, so tests/test_gpu_limb29_reduction.py no
longer vouches for any of it. These are the G2 twins of those tests: inputs whose piece, bucket, row and column sums meet
as equal, opposite and infinity at forced windows with the shortest piece, in the classic and the fixed-base form;
forced windows on every parity of the rows x columns split and every sort-pass count; repeated and opposite bases.
Expected values: the C oracle's MSM, the big-int oracle's scalar multiples. Bit-exact."""
import ctypes
import functools
import random

import pytest

from conftest import le
from oracle import c_oracle as co
from oracle.py import bn254 as bn
from oracle.py import groth16 as g16
from test_gpu_kernels import _g2_oracle_case

pytestmark = pytest.mark.gpu
R = bn.R
K0 = 8          # the smallest piece length the option accepts
SIZE = 128


def msm_plan(zk, n, c, k0, merged=0):
    f = zk.lib().zkpoa_test_msm_plan
    out = (ctypes.c_uint64 * 13)()
    assert f(n, c, merged, 1, None, k0, out, 13) == 13                 # for_g2 = 1: the request a G2 MSM makes
    return dict(zip(("c", "W", "Wb", "ne", "TB", "K0", "K", "logS", "logRows"), out))


def neg_bytes(b):
    return g16.g2_to_bytes(bn.ec_neg(g16.g2_from_bytes(b), bn.FQ2))


@functools.lru_cache(maxsize=None)
def build_input(n):
    """Bases from {P, -P, T, -T, infinity}, scalars from seven full-width values and their opposites: s and r - s fall
    into the same bucket of every window with opposite signs. Every scalar class gets the SAME list of bases, so the
    buckets of s1..s4 hold one value V, those of r - s5, r - s6 hold -V, and s7 with r - s7 cancels to infinity through
    equal and opposite piece sums; every piece, bucket, row and column sum is a small multiple of P plus one of T. An
    eighth of the points draw base and scalar freely from the same sets, and a sixteenth is an ordinary random block.
    -> (bases, scalars, n, the C oracle's sum), computed once."""
    rng = random.Random(137 + n)
    fb = co.fixed_base_g2(b"".join(le(rng.randrange(R)) for _ in range(n // 16 + 2)), 8)
    base = lambda i: fb[SIZE * i:SIZE * i + SIZE]
    P, T = base(n // 16), base(n // 16 + 1)
    kinds = [P, neg_bytes(P), T, neg_bytes(T), bytes(SIZE)]
    s = [rng.randrange(1, R) for _ in range(7)]
    classes = s[:4] + [R - s[4], R - s[5], s[6], R - s[6]]
    structured = n - n // 8 - n // 16
    per = structured // len(classes)
    shared = [rng.choice(kinds) for _ in range(per)]
    items = [(b, k) for k in classes for b in shared]
    every = s + [R - v for v in s] + [0, 1, R - 1]
    items += [(rng.choice(kinds), rng.choice(every)) for _ in range(n - n // 16 - len(items))]
    items += [(base(i), rng.randrange(R)) for i in range(n // 16)]
    assert len(items) == n
    rng.shuffle(items)
    bases = b"".join(b for b, _ in items)
    scal = b"".join(le(k) for _, k in items)
    return bases, scal, n, co.msm_g2(bases, scal, n, 8)


def forced_msm(ctx, bases, scal, n, c, k0=K0):
    ctx.set_option("msm_c", c)
    ctx.set_option("msm_k0", k0)
    try:
        return ctx.msm_g2(bases, scal, n)
    finally:
        ctx.set_option("msm_k0", 0)
        ctx.set_option("msm_c", 0)


@pytest.mark.parametrize("c", [4, 8, 13])
def test_g2_equal_and_opposite_sums_at_every_level(zk, ctx, c):
    """c = 4: 8 buckets per window, ~250 entries each: 32 pieces of 8 and three partial-sum levels; c = 8 and 13: shorter
    chains, more buckets per row and column sum"""
    bases, scal, n, want = build_input(1 << 11)
    plan = msm_plan(zk, n, c, K0)
    assert plan["c"] == c and plan["K0"] == K0
    if c == 4:
        pieces = -(-(n // 8) // K0)                                 # of one scalar class's share of a bucket, at least
        levels, k = 0, plan["K"]
        while pieces > 1:
            pieces, levels = -(-pieces // k), levels + 1
        assert levels >= 3
    assert forced_msm(ctx, bases, scal, n, c) == want


def test_g2_more_than_256_columns(zk, ctx):
    """the smallest forced window whose plan has more than 256 columns, so that msm_tree_sum_kernel<Fq2> finishes the sums"""
    n = 1 << 10
    c = next(c for c in range(4, 23) if msm_plan(zk, n, c, K0)["logS"] > 8)
    assert msm_plan(zk, n, c, K0)["c"] == c and msm_plan(zk, n, c - 1, K0)["logS"] <= 8
    bases, scal, _, want = build_input(n)
    assert forced_msm(ctx, bases, scal, n, c) == want


# both parities of the rows x S split (c - 1 even and odd) on each sort-pass count (1: c <= 9, 2: c <= 17, 3 beyond)
@pytest.mark.parametrize("c", [4, 5, 9, 10, 17, 18])
def test_g2_forced_windows(zk, ctx, c):
    """random bases with every 13th at infinity, witness-like scalars, the planner's own piece length"""
    n = 2000
    bases, sc, want = _g2_oracle_case(n, "witness")
    plan = msm_plan(zk, n, c, 0)
    assert plan["c"] == c and plan["logS"] + plan["logRows"] == c - 1 and plan["logS"] - plan["logRows"] == (c - 1) % 2
    assert forced_msm(ctx, bases, sc, n, c, k0=0) == want


def test_g2_repeated_and_opposite_bases(ctx):
    """All bases equal (the accumulation meets its own value: the doubling case) and G / -G pairs (P + (-P))."""
    n = 512
    G = g16.g2_to_bytes(bn.G2_GEN)
    negG = neg_bytes(G)
    sc = le(5) * n
    assert g16.g2_from_bytes(ctx.msm_g2(G * n, sc, n)) == bn.g2_mul(bn.G2_GEN, 5 * n)
    bases = (G + negG) * (n // 2)
    assert ctx.msm_g2(bases, sc, n) == bytes(SIZE)
    sc2 = b"".join(le(7 if i % 2 == 0 else 3) for i in range(n))
    assert g16.g2_from_bytes(ctx.msm_g2(bases, sc2, n)) == bn.g2_mul(bn.G2_GEN, 4 * (n // 2))
    # the same with the shortest piece, so the equal and opposite values also meet as partial sums
    assert g16.g2_from_bytes(forced_msm(ctx, G * n, sc, n, 4)) == bn.g2_mul(bn.G2_GEN, 5 * n)
    assert forced_msm(ctx, bases, sc, n, 4) == bytes(SIZE)
    assert g16.g2_from_bytes(forced_msm(ctx, bases, sc2, n, 4)) == bn.g2_mul(bn.G2_GEN, 4 * (n // 2))


def test_g2_fixed_base_form(ctx):
    """the structured input through a G2 fixed-base table: one bucket set for all windows, so sums of different windows meet"""
    import torch
    bases, scal, n, want = build_input(1 << 11)
    d_b = torch.frombuffer(bytearray(bases), dtype=torch.uint8).cuda()
    d_s = torch.frombuffer(bytearray(scal), dtype=torch.uint8).cuda()
    ctx.set_option("msm_k0", K0)
    table = None
    try:
        table = ctx.msm_table(2, d_b.data_ptr(), n, 8)
        assert table.info()[1] == 8
        assert ctx.msm_table_run(table, d_s.data_ptr()) == want
    finally:
        if table is not None:
            table.close()
        ctx.set_option("msm_k0", 0)
