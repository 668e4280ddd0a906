"""The BN254 field and curve primitives one by one on the device (zkpoa_field_prim / zkpoa_curve_prim: the product's
own Fq / Fr / Fq2 and XYZZ functions), on raw lazy inputs against the big-int reference in tests/prim_ref.py.

Every field op runs over three input sets in both fields: the edge set (prim_ref.edge_set: the two representations of
0, 1 and -1, both ends of [0, 2p), limb boundaries, neighbours of p and 2p), a band just under 2p (the largest
Montgomery T with varied quotients) and uniform values over [0, 2p). Inputs stay inside each primitive's stated
preconditions. A result must be right mod p and inside the range its function promises; the squaring and the
lockstep pair forms must also be bit-identical to the single products they replace."""
import functools
import random

import pytest

import prim_ref as pr
from oracle import c_oracle as co
from oracle.py import bn254 as bn

pytestmark = pytest.mark.gpu
Q, R = pr.Q, pr.R
FIELDS = [pytest.param("fq", 0, Q, id="fq"), pytest.param("fr", 1, R, id="fr")]
KINDS = ["edge", "nearmax", "uniform"]
N_NEAR = 4099
N_UNI = (1 << 16) + 77          # not a multiple of the 256-thread block
N_EDGE_TUPLES = 1 << 14
PAIR_OPS = ("mul_pair", "sqr_pair", "dot2_pair")


# ---- operand sets ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pool(p, kind):
    """(eight operand arrays in [0, 2p), three in [0, p), one in [0, 4p)) of one input set, seeded"""
    rng = random.Random("%s-%d" % (kind, p))
    if kind == "nearmax":
        return ([pr.near_max(rng, N_NEAR, 2 * p) for _ in range(8)], [pr.near_max(rng, N_NEAR, p) for _ in range(3)],
                pr.near_max(rng, N_NEAR, 4 * p))
    if kind == "uniform":
        return ([pr.uniform(rng, N_UNI, 2 * p) for _ in range(8)], [pr.uniform(rng, N_UNI, p) for _ in range(3)],
                pr.uniform(rng, N_UNI, 4 * p))
    E = pr.edge_set(p)
    Ep = [e for e in E if e < p]
    n = N_EDGE_TUPLES
    return ([[rng.choice(E) for _ in range(n)] for _ in range(8)], [[rng.choice(Ep) for _ in range(n)] for _ in range(3)],
            None)


def field_operands(name, p, kind):
    """The operand arrays of FIELD_OPS[name] for one input set (lists of raw ints)."""
    nin = pr.FIELD_OPS[name][1]
    E = pr.edge_set(p)
    if kind == "lockstep":          # pair forms: a near-max chain beside a zero chain, and the other way round
        rng = random.Random("lockstep-%d" % p)
        half = nin // 2
        ops = [[0] * N_NEAR for _ in range(nin)]
        for i in range(N_NEAR):
            lo = 0 if i % 2 == 0 else half
            for j in range(lo, lo + half):
                ops[j][i] = 2 * p - 1 - rng.randrange(1 << 200)
        return ops
    if kind == "edge" and nin == 1:
        return [E + [e + 2 * p for e in E]] if name == "reduce_2p" else [E]
    if kind == "edge" and nin == 2:
        return [[a for a in E for _ in E], [b for _ in E for b in E]]
    lazy, below_p, below_4p = _pool(p, kind)
    if name == "reduce_2p":          # its precondition is a < 4p
        return [below_4p]
    if name == "dot3":               # b operands < p
        return [lazy[0], below_p[0], lazy[1], below_p[1], lazy[2], below_p[2]]
    ops = [list(x) for x in lazy[:nin]]
    if name in ("dot2", "dot2_pair"):
        # one operand of the second product may be exactly 2p (neg_2p(0): Fq2 mul, the y3 of the G1 additions)
        for i in range(len(ops[0])):
            if i % 4 == 1:
                ops[3][i] = 2 * p
            elif i % 4 == 3:
                ops[2][i] = 2 * p
            if name == "dot2_pair" and i % 4 == 2:
                ops[7][i] = 2 * p
            elif name == "dot2_pair" and i % 4 == 0:
                ops[6][i] = 2 * p
    return ops


def run_field(ctx, field, name, ops, raw=True):
    op, _, nout = pr.FIELD_OPS[name]
    return [pr.unpack(b) for b in ctx.field_prim(field, op, [pr.pack(x) for x in ops], nout, raw)]


def _field_cases():
    for fname, field, p in (("fq", 0, Q), ("fr", 1, R)):
        for name in pr.FIELD_OPS:
            for kind in KINDS + (["lockstep"] if name in PAIR_OPS else []):
                yield pytest.param(field, p, name, kind, id="%s-%s-%s" % (fname, name, kind))


# ---- field ops ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,p,name,kind", list(_field_cases()))
def test_field_prim(ctx, field, p, name, kind):
    ops = field_operands(name, p, kind)
    outs = run_field(ctx, field, name, ops)
    assert pr.field_mismatches(name, p, ops, outs) == []


@pytest.mark.parametrize("fname,field,p", FIELDS)
def test_is_zero_only_for_0_and_p(ctx, fname, field, p):
    E = pr.edge_set(p)
    (got,) = run_field(ctx, field, "is_zero", [E])
    assert [e for e, g in zip(E, got) if g] == [0, p]


@pytest.mark.parametrize("kind", KINDS + ["lockstep"])
@pytest.mark.parametrize("fname,field,p", FIELDS)
def test_pair_forms_bitwise_equal_single_ops(ctx, fname, field, p, kind):
    """mul_pair / sqr_pair / dot2_pair advance two carry chains in lockstep (the second carry in an SGPR pair): each
    output must be the very bits the single op gives on the same operands, so nothing crosses between the chains."""
    ops = field_operands("mul_pair", p, kind)
    pair = run_field(ctx, field, "mul_pair", ops)
    assert pair == run_field(ctx, field, "mul", ops[:2]) + run_field(ctx, field, "mul", ops[2:])
    ops = field_operands("sqr_pair", p, kind)
    pair = run_field(ctx, field, "sqr_pair", ops)
    assert pair == run_field(ctx, field, "sqr", ops[:1]) + run_field(ctx, field, "sqr", ops[1:])
    ops = field_operands("dot2_pair", p, kind)
    pair = run_field(ctx, field, "dot2_pair", ops)
    assert pair == run_field(ctx, field, "dot2", ops[:4]) + run_field(ctx, field, "dot2", ops[4:])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname,field,p", FIELDS)
def test_sqr_bitwise_equals_mul(ctx, fname, field, p, kind):
    """the squaring's pre-doubled cross products give the same T, hence the same Montgomery quotients and bits"""
    (a,) = field_operands("sqr", p, kind)
    assert run_field(ctx, field, "sqr", [a]) == run_field(ctx, field, "mul", [a, a])


@pytest.mark.parametrize("fname,field,p", FIELDS)
def test_canonical_store(ctx, fname, field, p):
    """raw = 0 stores the canonical value of the same result"""
    for name in ("mul", "sub", "dot2_pair"):
        ops = field_operands(name, p, "edge")
        raw = run_field(ctx, field, name, ops)
        assert run_field(ctx, field, name, ops, raw=False) == [[v % p for v in r] for r in raw]


# ---- Fq2 ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fq2_pool(kind):
    rng = random.Random("fq2-" + kind)
    if kind == "edge":
        E = pr.edge_set(Q)
        return [[(rng.choice(E), rng.choice(E)) for _ in range(N_EDGE_TUPLES)] for _ in range(2)]
    gen = (lambda: pr.near_max(rng, N_NEAR, 2 * Q)) if kind == "nearmax" else (lambda: pr.uniform(rng, N_UNI, 2 * Q))
    return [list(zip(gen(), gen())) for _ in range(2)]


def run_fq2(ctx, name, ops, raw=True):
    op, _ = pr.FQ2_OPS[name]
    (out,) = ctx.field_prim(2, op, [pr.pack2(x) for x in ops], 1, raw)
    return pr.unpack2(out)


def fq2_mismatches(name, ops, got, limit=5):
    want = pr.fq2_ref(name, ops)
    bad = []
    for i, (w, g) in enumerate(zip(want, got)):
        if not all(0 <= c < 2 * Q for c in g) or (g[0] % Q, g[1] % Q) != w:
            bad.append((i, [o[i] for o in ops], g))
            if len(bad) >= limit:
                break
    return bad


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(pr.FQ2_OPS))
def test_fq2_prim(ctx, name, kind):
    ops = _fq2_pool(kind)[:pr.FQ2_OPS[name][1]]
    assert fq2_mismatches(name, ops, run_fq2(ctx, name, ops)) == []


def test_fq2_mul_by_c1_zero_or_p(ctx):
    """b.c1 in {0, p}: the product's neg_2p operand is then 2p or p, the ends of what dot2 accepts"""
    rng = random.Random(7)
    E = pr.edge_set(Q)
    a = [(x, y) for x in E for y in (0, 1, Q - 1, Q, 2 * Q - 1)]
    a += list(zip(pr.near_max(rng, 512, 2 * Q), pr.near_max(rng, 512, 2 * Q)))
    b = [(rng.choice(E + [2 * Q - 1 - rng.randrange(1 << 200)]), rng.choice((0, Q))) for _ in a]
    assert fq2_mismatches("mul", [a, b], run_fq2(ctx, "mul", [a, b])) == []
    assert fq2_mismatches("mul", [b, a], run_fq2(ctx, "mul", [b, a])) == []


def test_fq2_inv_of_zero(ctx):
    zeros = [(0, 0), (Q, 0), (0, Q), (Q, Q)]
    assert [(x % Q, y % Q) for x, y in run_fq2(ctx, "inv", [zeros])] == [(0, 0)] * 4
    assert run_fq2(ctx, "inv", [zeros], raw=False) == [(0, 0)] * 4


def test_unknown_field_curve_and_op_are_errors(zk, ctx):
    two = bytes(64)                  # two Fq / Fr elements or one Fq2 element
    for field, op in ((3, 0), (-1, 0), (0, 17), (1, -1), (2, 6)):
        with pytest.raises(zk.ZkpoaError, match="field_prim"):
            ctx.field_prim(field, op, [two, two])
        with pytest.raises(zk.ZkpoaError, match="field_prim"):
            ctx.field_prim(field, op, [])
    for group, op in ((0, 0), (3, 0), (1, 5), (2, -1)):
        with pytest.raises(zk.ZkpoaError, match="curve_prim"):
            ctx.curve_prim(group, op, a=bytes(128), b=bytes(128), k=[0], n=1)
        with pytest.raises(zk.ZkpoaError, match="curve_prim"):
            ctx.curve_prim(group, op, n=0)


# ---- curve -------------------------------------------------------------------------------------------
N_PTS = 24
K_SMALL = [0, 1, 2, 3, 7, 1 << 16, 1 << 31, (1 << 32) - 1]


@functools.lru_cache(maxsize=None)
def _points(group):
    rng = random.Random(group)
    fb = co.fixed_base_g1 if group == 1 else co.fixed_base_g2
    pts = pr.affine_list(group, fb(pr.pack(rng.randrange(1, R) for _ in range(2 * N_PTS)), 4))
    return pts[:N_PTS], pts[N_PTS:]


def _lams(group, rng):
    """1, -1 and random scales (G2: random elements of Fq2)"""
    def rnd():
        return rng.randrange(2, Q) if group == 1 else (rng.randrange(Q), rng.randrange(1, Q))
    return [1, -1] + [rnd() for _ in range(4)]


def _lazy(rng):
    return tuple(rng.random() < 0.5 for _ in range(4))


def _check_points(group, got_buf, want):
    got = pr.xyzz_list(group, got_buf)
    assert len(got) == len(want)
    bad = [(i, why) for i, (g, w) in enumerate(zip(got, want)) for why in [pr.xyzz_mismatch(group, g, w)] if why]
    assert bad == []


@pytest.mark.parametrize("group", [1, 2])
def test_xyzz_add(ctx, group):
    F = pr.curve_field(group)
    rng = random.Random(100 + group)
    Ps, Qs = _points(group)
    a, b, want = [], [], []

    def case(x, y, w):
        a.append(x)
        b.append(y)
        want.append(w)

    for P, S in zip(Ps, Qs):
        l1, l2 = rng.sample(_lams(group, rng), 2)
        nP = bn.ec_neg(P, F)
        case(pr.xyzz_of(group, P, l1, _lazy(rng)), pr.xyzz_of(group, S, l2, _lazy(rng)), bn.ec_add(P, S, F))
        same = pr.xyzz_of(group, P, l1, _lazy(rng))
        case(same, same, bn.ec_double(P, F))                                     # P + P, same representation
        case(pr.xyzz_of(group, P, l1, _lazy(rng)), pr.xyzz_of(group, P, l2, _lazy(rng)), bn.ec_double(P, F))
        case(pr.xyzz_of(group, P, l1, _lazy(rng)), pr.xyzz_of(group, nP, l2, _lazy(rng)), None)
        case(pr.xyzz_of(group, P, l1, _lazy(rng)), pr.xyzz_of(group, nP, l1, _lazy(rng)), None)
        for rep in (0, Q):
            case(pr.xyzz_inf(group, rng, rep), pr.xyzz_of(group, P, l1, _lazy(rng)), P)
            case(pr.xyzz_of(group, P, l1, _lazy(rng)), pr.xyzz_inf(group, rng, rep), P)
            case(pr.xyzz_inf(group, rng, rep), pr.xyzz_inf(group, rng, Q - rep), None)
    # P + P where the two u's differ by exactly p (one coordinate lazy, the other canonical)
    for P in Ps:
        l1 = _lams(group, rng)[2]
        case(pr.xyzz_of(group, P, l1, (True, True, False, False)), pr.xyzz_of(group, P, l1), bn.ec_double(P, F))
        case(pr.xyzz_of(group, P, l1, (False, False, True, True)), pr.xyzz_of(group, P, l1), bn.ec_double(P, F))
    out = ctx.curve_prim(group, pr.CURVE_OPS["add"], a=pr.xyzz_bytes(a), b=pr.xyzz_bytes(b))
    _check_points(group, out, want)


@pytest.mark.parametrize("group", [1, 2])
def test_xyzz_add_affine(ctx, group):
    F = pr.curve_field(group)
    rng = random.Random(200 + group)
    Ps, Qs = _points(group)
    a, b, k, want = [], [], [], []
    for P, S in zip(Ps, Qs):
        lam = _lams(group, rng)[2 + rng.randrange(4)]                  # acc.zz != 1
        nP = bn.ec_neg(P, F)
        for base in (S, P, nP, None):
            for neg in (0, 1):
                addend = bn.ec_neg(base, F) if neg else base
                a.append(pr.xyzz_of(group, P, lam, _lazy(rng)))
                b.append(base)
                k.append(neg)
                want.append(bn.ec_add(P, addend, F))
        for rep in (0, Q):                                             # onto an infinity accumulator
            for neg in (0, 1):
                a.append(pr.xyzz_inf(group, rng, rep))
                b.append(S)
                k.append(neg)
                want.append(bn.ec_neg(S, F) if neg else S)
    ab = b"".join(pr.affine_bytes(group, P) for P in b)
    out = ctx.curve_prim(group, pr.CURVE_OPS["add_affine"], a=pr.xyzz_bytes(a), b=ab, k=k)
    _check_points(group, out, want)


@pytest.mark.parametrize("group", [1, 2])
def test_xyzz_dbl(ctx, group):
    F = pr.curve_field(group)
    rng = random.Random(300 + group)
    Ps, _ = _points(group)
    a = [pr.xyzz_of(group, P, lam, _lazy(rng)) for P in Ps for lam in _lams(group, rng)[:3]]
    want = [bn.ec_double(P, F) for P in Ps for _ in range(3)]
    a += [pr.xyzz_inf(group, rng, 0), pr.xyzz_inf(group, rng, Q)]
    want += [None, None]
    _check_points(group, ctx.curve_prim(group, pr.CURVE_OPS["dbl"], a=pr.xyzz_bytes(a)), want)
    ab = b"".join(pr.affine_bytes(group, P) for P in Ps)
    _check_points(group, ctx.curve_prim(group, pr.CURVE_OPS["dbl_affine"], b=ab),
                  [bn.ec_double(P, F) for P in Ps])


@pytest.mark.parametrize("group", [1, 2])
def test_xyzz_mul_small(ctx, group):
    F = pr.curve_field(group)
    rng = random.Random(400 + group)
    Ps, _ = _points(group)
    a, k, want = [], [], []
    for i, P in enumerate(Ps[:16]):
        lam = _lams(group, rng)[i % 6]
        for kk in K_SMALL + [rng.randrange(1 << 32), rng.randrange(1 << 12)]:
            a.append(pr.xyzz_of(group, P, lam, _lazy(rng)))
            k.append(kk)
            want.append(bn.ec_mul(P, kk, F))
    out = ctx.curve_prim(group, pr.CURVE_OPS["mul_small"], a=pr.xyzz_bytes(a), k=k)
    _check_points(group, out, want)
