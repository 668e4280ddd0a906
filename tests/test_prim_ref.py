"""The reference of tests/test_gpu_primitives.py checked without a GPU: tests/prim_ref.py against the C oracle's
field and group operations on the canonical part of the edge set, and the affine addition it uses against the
Jacobian one, so a wrong reference fails here and not only on the GPU box."""
import random

import pytest

import prim_ref as pr
from oracle import c_oracle as co
from oracle.py import bn254 as bn

Q, R = pr.Q, pr.R


@pytest.mark.parametrize("field,p", [(0, Q), (1, R)])
def test_edge_set(field, p):
    E = pr.edge_set(p)
    assert 50 <= len(E) <= 80 and all(0 <= e < 2 * p for e in E)
    for v in (0, 1, p - 1, p, p + 1, 2 * p - 1, pr.M % p, pr.M % p + p, p - pr.M % p, 2 * p - pr.M % p):
        assert v in E


@pytest.mark.parametrize("field,p", [(0, Q), (1, R)])
def test_field_ref_vs_c_oracle(field, p):
    E = [e for e in pr.edge_set(p) if e < p]
    a = [x for x in E for _ in E]
    b = [y for _ in E for y in E]
    A, B = pr.pack(a), pr.pack(b)

    def oracle(op, x, y=None):
        return pr.unpack(co.field_op(field, op, x, y))

    def ref(name, *ops):
        return pr.field_ref(name, p, [list(o) for o in ops])

    mul, add, sub = oracle(0, A, B), oracle(1, A, B), oracle(2, A, B)
    assert ref("mul", a, b) == [mul]
    assert ref("add", a, b) == [add]
    assert ref("sub", a, b) == [sub]
    assert ref("inv", E) == [oracle(3, pr.pack(E))]
    assert ref("sqr", E) == [oracle(0, pr.pack(E), pr.pack(E))]
    assert ref("neg", E) == ref("neg_2p", E) == [oracle(2, pr.pack([0] * len(E)), pr.pack(E))]
    assert ref("dbl", E) == [oracle(1, pr.pack(E), pr.pack(E))]
    assert ref("canon", E) == ref("reduce_2p", E) == [E]
    assert ref("is_zero", E) == [[int(e == 0) for e in E]]
    assert ref("eq", a, b) == [[int(x == y) for x, y in zip(a, b)]]
    # the sums of products: the oracle's products added with its own addition
    rng = random.Random(field)
    t = [[rng.choice(E) for _ in range(500)] for _ in range(8)]
    prods = [oracle(0, pr.pack(t[2 * j]), pr.pack(t[2 * j + 1])) for j in range(4)]
    s01, s23 = (oracle(1, pr.pack(prods[j]), pr.pack(prods[j + 1])) for j in (0, 2))
    s012 = oracle(1, pr.pack(s01), pr.pack(prods[2]))
    assert ref("dot2", *t[:4]) == [s01]
    assert ref("dot3", *t[:6]) == [s012]
    assert ref("mul_pair", *t[:4]) == [prods[0], prods[1]]
    assert ref("sqr_pair", t[0], t[2]) == [oracle(0, pr.pack(t[0]), pr.pack(t[0])), oracle(0, pr.pack(t[2]), pr.pack(t[2]))]
    assert ref("dot2_pair", *t) == [s01, s23]
    # a lazy operand (value + p) gives the same residue
    assert ref("mul", [x + p for x in a], b) == [mul]


def test_field_mismatches_flags_range_and_value():
    p = Q
    ops = [[1, p, 0]]
    assert pr.field_mismatches("canon", p, ops, [[1, 0, 0]]) == []
    assert pr.field_mismatches("canon", p, ops, [[1, p, 0]])[0][4].startswith("out of range")
    assert pr.field_mismatches("neg", p, ops, [[2 * p - 1, p, 0]]) == []
    assert pr.field_mismatches("neg", p, ops, [[2 * p - 1, p, p]])[0][4] == "neg(0) != 0"
    assert pr.field_mismatches("neg_2p", p, ops, [[2 * p - 1, p, 2 * p]]) == []
    assert pr.field_mismatches("is_zero", p, ops, [[0, 0, 1]])[0][4] == "flag"
    assert pr.field_mismatches("mul", p, [[5], [7]], [[2 * p]])[0][4].startswith("out of range")
    assert pr.field_mismatches("mul", p, [[5], [7]], [[35]])[0][4] == "value mod p"


def test_fq2_ref_vs_fq2_ops():
    rng = random.Random(3)
    E = pr.edge_set(Q)
    a = [(rng.choice(E), rng.choice(E)) for _ in range(300)] + [(0, 0), (Q, 0), (0, Q)]
    b = [(rng.choice(E), rng.choice(E)) for _ in range(len(a))]
    std = lambda v: pr.from_mont(v)          # noqa: E731
    mont = lambda v: pr.to_mont(v)           # noqa: E731
    F = bn.FQ2
    assert pr.fq2_ref("mul", [a, b]) == [mont(F.mul(std(x), std(y))) for x, y in zip(a, b)]
    assert pr.fq2_ref("sqr", [a]) == [mont(F.sqr(std(x))) for x in a]
    assert pr.fq2_ref("add", [a, b]) == [mont(F.add(std(x), std(y))) for x, y in zip(a, b)]
    assert pr.fq2_ref("sub", [a, b]) == [mont(F.sub(std(x), std(y))) for x, y in zip(a, b)]
    assert pr.fq2_ref("neg", [a]) == [mont(F.neg(std(x))) for x in a]
    inv = pr.fq2_ref("inv", [a])
    for x, i in zip(a, inv):
        assert i == (0, 0) if F.is_zero(std(x)) else F.mul(std(x), std(i)) == (1, 0)


def _rand_points(group, n, seed):
    rng = random.Random(seed)
    fb = co.fixed_base_g1 if group == 1 else co.fixed_base_g2
    return pr.affine_list(group, fb(pr.pack(rng.randrange(1, R) for _ in range(n)), 2))


@pytest.mark.parametrize("group", [1, 2])
def test_ec_add_vs_c_oracle_and_jacobian(group):
    """bn254.ec_add (the curve reference) against the C oracle's mixed addition and against bn254.jac_add, on random
    points and the exceptional cases (P + P, P + (-P), infinity on either side)."""
    F = pr.curve_field(group)
    P = _rand_points(group, 24, group)
    S = _rand_points(group, 24, group + 10)
    a = P + P + P + [None] + P[:2]
    b = S + P + [bn.ec_neg(x, F) for x in P] + [S[0]] + [None, None]
    want = [bn.ec_add(x, y, F) for x, y in zip(a, b)]
    got = co.group_add(group, b"".join(pr.affine_bytes(group, x) for x in a),
                       b"".join(pr.affine_bytes(group, y) for y in b))
    assert pr.affine_list(group, got) == want
    jac = [bn.jac_to_affine(bn.jac_add(bn.jac_from_affine(x, F), bn.jac_from_affine(y, F), F), F) for x, y in zip(a, b)]
    assert jac == want
    assert all(bn.ec_is_on_curve(w, F, bn.B1 if group == 1 else bn.B2) for w in want)
    assert [bn.ec_mul(x, 5, F) for x in P[:4]] == [bn.ec_add(bn.ec_double(bn.ec_double(x, F), F), x, F) for x in P[:4]]


@pytest.mark.parametrize("group", [1, 2])
def test_xyzz_checker(group):
    """xyzz_of builds what xyzz_mismatch accepts, with any scale and lazy coordinates; a wrong point, a broken
    ZZ^3 = ZZZ^2, an out-of-range coordinate or a non-infinity are each reported."""
    F = pr.curve_field(group)
    rng = random.Random(group)
    P, S = _rand_points(group, 2, 50 + group)
    lam = rng.randrange(2, Q) if group == 1 else (rng.randrange(Q), rng.randrange(1, Q))
    for l in (1, -1, lam):
        for lazy in ((False,) * 4, (True,) * 4, (True, False, True, False)):
            assert pr.xyzz_mismatch(group, pr.xyzz_of(group, P, l, lazy), P) is None
    x, y, zz, zzz = pr.xyzz_of(group, P, lam)
    assert pr.xyzz_mismatch(group, (x, y, zz, zzz), S) == "wrong point"
    assert pr.xyzz_mismatch(group, (x, y, zz, zz), P) == "ZZ^3 != ZZZ^2"
    assert pr.xyzz_mismatch(group, (x, y, zz, zzz), None) == "not infinity"
    assert pr.xyzz_mismatch(group, pr.xyzz_of(group, P, lam, (False, False, True, False)), P) is None
    big = 2 * Q if group == 1 else (2 * Q, 0)
    assert pr.xyzz_mismatch(group, (big, y, zz, zzz), P).startswith("coordinate out")
    for rep in (0, Q):
        inf = pr.xyzz_inf(group, rng, rep)
        assert pr.xyzz_mismatch(group, inf, None) is None
        assert pr.xyzz_mismatch(group, inf, P) == "infinity"
    # the XYZZ bytes round-trip
    pts = [pr.xyzz_of(group, P, lam, (True, False, True, False)), pr.xyzz_inf(group, rng, Q)]
    assert pr.xyzz_list(group, pr.xyzz_bytes(pts)) == pts
    assert F.eq(pr.from_mont(pts[0][2]), F.sqr(lam if group == 2 else lam % Q))
