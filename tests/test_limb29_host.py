"""zk-proof-of-assets_amd/csrc/fq29.hip.h on the CPU: tools/limb29_check.cpp includes the header's own text, g++ compiles
it with -DZKPOA_LIMB29_CHECK (every column addition checked for leaving 64 bits), and the results are compared with
Python integers. Operands: random members of every operand class the header defines, operands with every limb at the
maximum its class allows, and the values 0, 1, q - 1, q, 2q - 1 and the largest multiple of q of the class; a chain of
64 mixed additions and full additions against oracle/py/bn254.py. The overflow counter must stay 0."""
import os
import random
import struct
import subprocess

import pytest

from conftest import ROOT
from oracle.py import bn254 as bn
import limb29_ref as lr

N_RANDOM = 10000


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("limb29") / "limb29_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-DZKPOA_LIMB29_CHECK", "-I",
                    os.path.join(ROOT, "zk-proof-of-assets_amd", "csrc"), os.path.join(ROOT, "tools", "limb29_check.cpp"),
                    "-o", out], check=True, capture_output=True, text=True)
    return out


def run(check_bin, op, records, out_words):
    data = struct.pack("<I", len(records)) + lr.pack(records)
    rc = subprocess.run([check_bin, str(op)], input=data, capture_output=True, timeout=300)
    assert rc.returncode == 0
    assert len(rc.stdout) == 4 * out_words * len(records) + 8
    overflows = struct.unpack("<Q", rc.stdout[-8:])[0]
    assert overflows == 0
    return lr.unpack(rc.stdout[:-8], out_words)


@pytest.mark.parametrize("op", [lr.OP_MUL, lr.OP_SQR, lr.OP_DOT2])
def test_products(check_bin, op):
    recs = lr.product_cases(random.Random(29 + op), N_RANDOM)[op]
    assert len(recs) >= N_RANDOM - 8
    for rec, got in zip(recs, run(check_bin, op, recs, 9)):
        lr.check_product(op, rec, got)


@pytest.mark.parametrize("op", [lr.OP_SUB4, lr.OP_SUB14])
def test_sub_norm(check_bin, op):
    recs = lr.sub_cases(random.Random(31 + op), N_RANDOM)[op]
    for rec, got in zip(recs, run(check_bin, op, recs, 9)):
        lr.check_sub(op, rec, got)


def test_relimb_round_trip(check_bin):
    recs = lr.relimb_cases(random.Random(37), N_RANDOM)
    for rec, got in zip(recs, run(check_bin, lr.OP_RELIMB, recs, 17)):
        lr.check_relimb(rec, got)


def test_chain_of_64_mixed_additions(check_bin):
    """one piece: 64 bases with signs, infinity bases among them (first, middle, last position), summed from an empty
    accumulator; every prefix of the chain is checked, so each of the 64 additions is"""
    rng = random.Random(41)
    pts = lr.g1_points(rng, 64)
    for i in (0, 31, 63):
        pts[i] = None
    negs = [rng.randrange(2) for _ in pts]
    recs, want = [], []
    acc = None
    for k in range(1, 65):
        recs.append([k] + sum((lr.affine_words(P) + [s] for P, s in zip(pts[:k], negs[:k])), []))
        acc = bn.g1_add(acc, lr.signed(pts[k - 1], negs[k - 1]))
        want.append(acc)
    got = run(check_bin, lr.OP_PIECE, recs, 32)
    for k, (g, w) in enumerate(zip(got, want)):
        for c in range(4):
            assert int.from_bytes(struct.pack("<8I", *g[8 * c:8 * c + 8]), "little") < 3 * lr.Q
        assert lr.xyzz_point(g) == w, k
    assert want[0] is None and got[0] == [0] * 32       # an empty piece is all-zero words


def test_full_additions(check_bin):
    rng = random.Random(43)
    pts = lr.g1_points(rng, 65)
    recs = [lr.xyzz_words(pts[i], rng) + lr.xyzz_words(pts[i + 1], rng) for i in range(64)]
    got = run(check_bin, lr.OP_ADD, recs, 36)
    for i, g in enumerate(got):
        words = []
        for c in range(4):
            l = g[9 * c:9 * c + 9]
            assert lr.is_normalised(l) and lr.value(l) < 3 * lr.Q
            words += list(struct.unpack("<8I", (lr.value(l) % lr.Q).to_bytes(32, "little")))
        assert lr.xyzz_point(words) == bn.g1_add(pts[i], pts[i + 1]), i


def test_exceptional_sum_shows_zz_zero(check_bin):
    """acc = +-base is not handled by the generic formulas: ZZ becomes 0 (mod q) and stays 0 through later additions,
    which is what the kernels test once per piece before they redo it with the exact addition"""
    rng = random.Random(47)
    P, S, T = lr.g1_points(rng, 3)
    for seq in ([(P, 0), (P, 0), (S, 0)], [(P, 0), (P, 1), (S, 0), (T, 1)], [(P, 0), (S, 0), (bn.g1_add(P, S), 1), (T, 0)]):
        rec = [len(seq)] + sum((lr.affine_words(p) + [s] for p, s in seq), [])
        g = run(check_bin, lr.OP_PIECE, [rec], 32)[0]
        zz = int.from_bytes(struct.pack("<8I", *g[16:24]), "little")
        assert zz % lr.Q == 0 and zz < 3 * lr.Q
