"""The packed partial-sum form of zk-proof-of-assets_amd/csrc/fq29.hip.h on the CPU: tools/limb29_check.cpp includes the
header's own text, g++ compiles it with -DZKPOA_LIMB29_CHECK (every column addition checked for leaving 64 bits) and the
results are compared with Python integers and oracle/py/bn254.py:
  * X brought below 2^256 over the whole class-X range (multiples of q and their neighbours, the edges of the quotient
    estimate, just below 13q, just above 2^256), and the store / load round trip of a whole sum;
  * xyzz29s_add on operands of the loaded class (every coordinate any representative below 2^256) and on its own
    stored results, six levels deep;
  * a piece closed straight into the packed form; what a poisoned sum looks like.
The overflow counter must stay 0. The program is also built once with -fsanitize=address,undefined (a plain host
program with its own main) and has to give the same bytes."""
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
Q8 = Q >> 232
N_RANDOM = 10000


def build(tmp_path_factory, name, flags):
    out = str(tmp_path_factory.mktemp(name) / "limb29_check")
    subprocess.run(["g++", "-std=c++17", "-DZKPOA_LIMB29_CHECK", *flags, "-I",
                    os.path.join(ROOT, "zk-proof-of-assets_amd", "csrc"), os.path.join(ROOT, "tools", "limb29_check.cpp"),
                    "-o", out], check=True, capture_output=True, text=True)
    return out


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    return build(tmp_path_factory, "limb29p", ["-O2"])


def run_raw(binary, op, records):
    data = struct.pack("<I", len(records)) + lr.pack(records)
    rc = subprocess.run([binary, str(op)], input=data, capture_output=True, timeout=300)
    assert rc.returncode == 0, rc.stderr[-2000:]
    assert rc.stderr == b""
    return rc.stdout


def run(binary, op, records, out_words):
    out = run_raw(binary, op, records)
    assert len(out) == 4 * out_words * len(records) + 8
    assert struct.unpack("<Q", out[-8:])[0] == 0          # no column left 64 bits
    return lr.unpack(out[:-8], out_words)


def x_cases(rng, n_random):
    vals = [rng.randrange(13 * Q) for _ in range(n_random)]
    vals += [k * Q + d for k in range(13) for d in (-1, 0, 1) if k * Q + d >= 0]
    vals += [13 * Q - 1, 13 * Q - 2, (1 << 256) - 1, 1 << 256, (1 << 256) + 1, (1 << 256) + (1 << 232), (1 << 232) - 1]
    for k in range(1, 13):                                  # limb 8 at the edges of the quotient estimate
        for e in (-1, 0, 1):
            top = k * (Q8 + 1) + e
            vals += [v for v in (top << 232, (top << 232) | ((1 << 232) - 1)) if v < 13 * Q]
    assert all(0 <= v < 13 * Q for v in vals)
    return [lr.limbs(v) for v in vals] + [lr.max_elem("X")] + lr.special_values("X")


def check_x(rec, got):
    v = lr.value(rec)
    l, w, back = got[:9], got[9:17], got[17:26]
    assert lr.is_normalised(l), (rec, got)
    r = lr.value(l)
    assert r < Q + 14 * (1 << 232) < (1 << 256), (rec, got)
    assert r <= v and (v - r) % Q == 0, (rec, got)
    assert pr.word_value(w) == r and back == l, (rec, got)


def test_x_below_2p256(check_bin):
    recs = x_cases(random.Random(71), N_RANDOM)
    for rec, got in zip(recs, run(check_bin, pr.OP_X_BELOW, recs, 26)):
        check_x(rec, got)


def sum_cases(rng, n_random):
    recs = [sum((lr.rand_elem(rng, c) for c in cs), []) for cs in ("XNNN", "WWNW", "XWNN") for _ in range(n_random // 3)]
    recs.append(sum((lr.max_elem(c) for c in "XNNN"), []))
    recs.append(lr.max_elem("W") * 4)
    recs.append(lr.limbs(0) * 4)
    return recs


def check_round_trip(rec, got):
    w, back = got[:32], got[32:]
    for c in range(4):
        v = lr.value(rec[9 * c:9 * c + 9])
        r = pr.word_value(w[8 * c:8 * c + 8])
        if c == 0:
            assert r <= v and (v - r) % Q == 0, (rec, got)
        else:
            assert r == v, (rec, got)                       # y, zz, zzz are stored as they are
        assert back[9 * c:9 * c + 9] == lr.limbs(r), (rec, got)


def test_store_load_round_trip(check_bin):
    recs = sum_cases(random.Random(73), 3000)
    for rec, got in zip(recs, run(check_bin, pr.OP_PACK_UNPACK, recs, 68)):
        check_round_trip(rec, got)


def test_additions_of_loaded_operands(check_bin):
    """512 pairs of random representatives; then 64 points summed as a tree, every level's operands the stored results
    of the level before (x normalised from class X, the other coordinates product outputs)"""
    rng = random.Random(79)
    pts = lr.g1_points(rng, 1024 + 64)
    pairs = [(pts[2 * i], pts[2 * i + 1]) for i in range(512)]
    recs = [pr.packed_words(a, rng) + pr.packed_words(b, rng) for a, b in pairs]
    recs += [pr.packed_words(a, rep=k) + pr.packed_words(b, rep=2 - k) for k, (a, b) in zip((0, 1, 2), pairs)]
    for (a, b), got in zip(pairs + pairs[:3], run(check_bin, pr.OP_PACKED_ADD, recs, 32)):
        assert pr.packed_point(got) == bn.g1_add(a, b)
    level = [(pr.packed_words(P, rng), P) for P in pts[1024:]]
    while len(level) > 1:
        recs = [level[i][0] + level[i + 1][0] for i in range(0, len(level), 2)]
        want = [bn.g1_add(level[i][1], level[i + 1][1]) for i in range(0, len(level), 2)]
        got = run(check_bin, pr.OP_PACKED_ADD, recs, 32)
        for g, w in zip(got, want):
            assert pr.packed_point(g) == w
        level = list(zip(got, want))


def test_exceptional_sum_is_poisoned(check_bin):
    """acc = +-b, through any representatives: ZZ comes out 0 (mod q) as one of 0, q, 2q, and stays so through a
    later addition -- what the kernels test before they store"""
    rng = random.Random(83)
    P, S = lr.g1_points(rng, 2)
    recs = [pr.packed_words(P, rng) + pr.packed_words(P, rng), pr.packed_words(P, rng) + pr.packed_words(pr.neg(P), rng)]
    recs += [pr.packed_words(P, t=5, rep=j) + pr.packed_words(P, t=5, rep=k) for j in range(3) for k in range(3)]
    got = run(check_bin, pr.OP_PACKED_ADD, recs, 32)
    for g in got:
        zz = pr.word_value(g[16:24])
        assert zz in (0, Q, 2 * Q), g
    for g in run(check_bin, pr.OP_PACKED_ADD, [g + pr.packed_words(S, rng) for g in got if any(g)], 32):
        assert pr.word_value(g[16:24]) in (0, Q, 2 * Q), g


def piece_cases(rng):
    # (independent multiples of the generator: a signed sum of members of lr.g1_points' arithmetic progression can be
    # another member, an exceptional case where none is meant)
    pts = [bn.g1_mul(bn.G1_GEN, rng.randrange(1, bn.R)) for _ in range(33)]
    pieces = [[(P, rng.randrange(2)) for P in rng.sample(pts, n)] for n in (1, 2, 3, 8, 16, 33)]
    pieces.append([(None, 0), (pts[0], 1), (None, 1), (pts[1], 0)])
    pieces.append([(None, 0)] * 3)
    pieces.append([])
    poisoned = [[(pts[0], 0), (pts[0], 0), (pts[1], 0)], [(pts[0], 0), (pts[0], 1), (pts[2], 0)]]
    return pieces, poisoned


def piece_record(seq):
    return [len(seq)] + sum((lr.affine_words(P) + [s] for P, s in seq), [])


def test_piece_closes_into_the_packed_form(check_bin):
    pieces, poisoned = piece_cases(random.Random(89))
    got = run(check_bin, pr.OP_PIECE_PACKED, [piece_record(s) for s in pieces + poisoned], 33)
    for seq, g in zip(pieces, got):
        want = None
        for P, s in seq:
            want = bn.g1_add(want, lr.signed(P, s))
        assert g[32] == 1 and pr.packed_point(g[:32]) == want, seq
    for g in got[len(pieces):]:
        assert g[32] == 0 and pr.word_value(g[16:24]) in (0, Q, 2 * Q)


def test_sanitized_build_gives_the_same_bytes(check_bin, tmp_path_factory):
    san = build(tmp_path_factory, "limb29san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    rng = random.Random(97)
    pts = lr.g1_points(rng, 16)
    pieces, poisoned = piece_cases(rng)
    sets = {pr.OP_X_BELOW: x_cases(rng, 200),
            pr.OP_PACK_UNPACK: sum_cases(rng, 60),
            pr.OP_PACKED_ADD: [pr.packed_words(pts[i], rng) + pr.packed_words(pts[i + 1], rng) for i in range(15)] +
                              [pr.packed_words(pts[0], rng) * 2, [0] * 64],
            pr.OP_PIECE_PACKED: [piece_record(s) for s in pieces + poisoned]}
    for op, recs in sets.items():
        assert run_raw(san, op, recs) == run_raw(check_bin, op, recs), op
