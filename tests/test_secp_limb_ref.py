"""tests/secp_limb_ref.py against % on big integers, and the branch census of its operand sets: the sets must reach every
arm of every correction of csrc/secp256k1.hip.h, which random operands never do (about 2^-190 per product). The conditions
are asserted on the restatement's tags, never on the code under test. No GPU; the last test alone loads the library, to
hold the hook's ctypes signature against its header."""
import os
import random
import re

import pytest

import secp_limb_ref as lr
import secp_ref as sr
import sign_ref as sg
from conftest import ROOT

P, N, K, C = lr.P, lr.N, lr.K, lr.C


@pytest.fixture(scope="module")
def census():
    return lr.census()


def test_fp_values():
    """every Fp function at every operand of the sets; the two arms of a correction never both apply"""
    for a, b in lr.fp_pairs():
        v, t = lr.fp_mul(a, b)
        assert v == a * b % P and not (t["carry"] and t["ge"]), (a, b)
        v, t = lr.fp_add(a, b)
        assert v == (a + b) % P and not (t["carry"] and t["ge"]), (a, b)
        assert lr.fp_sub(a, b)[0] == (a - b) % P, (a, b)
    rng = random.Random(1)
    for a in lr.FP_SCALARS + [rng.randrange(P) for _ in range(2000)]:
        v, t = lr.fp_sqr(a)
        assert v == a * a % P and not (t["carry"] and t["ge"]) and t == lr.fp_mul(a, a)[1], a
        assert lr.fp_neg(a)[0] == -a % P and lr.fp_dbl(a)[0] == 2 * a % P, a
    for a in lr.FP_SCALARS + [rng.randrange(P) for _ in range(5)]:
        assert lr.fp_inv(a)[0] == pow(a, P - 2, P), a
        assert lr.fp_sqrt_candidate(a)[0] == pow(a, (P + 1) // 4, P), a
    for a in lr.any256():
        assert lr.fp_ge_p(a)[0] == int(a >= P), a


def test_sc_values():
    for a, b in lr.sc_pairs():
        v, t = lr.sc_mul(a, b)
        assert v == a * b % N and not (t["carry"] and t["ge"]), (a, b)
        # what the bounds t < 2^512 -> w1 < 2^386 -> w2 < 2^259 say: no fold loses a carry, w2 ends at limb 8, and the
        # sixth high limb that the second fold reads is zero
        assert not t["lost"] and t["w2_high"] == [0, 0, 0] and t["w2_8"] < 8 and t["w1_13"] == 0, (a, b)
        v, t = lr.sc_add(a, b)
        assert v == (a + b) % N and not (t["carry"] and t["ge"]), (a, b)
    rng = random.Random(2)
    for a in lr.SC_SCALARS + [rng.randrange(N) for _ in range(2000)]:
        assert lr.sc_neg(a)[0] == -a % N, a
        assert lr.sc_add_c(a, 1)[0] == (a + C) % (1 << 256) and lr.sc_add_c(a, 0)[0] == a, a
    for a in lr.SC_SCALARS + [rng.randrange(N) for _ in range(3)]:
        assert lr.sc_inv(a)[0] == pow(a, N - 2, N), a
    for a in lr.any256() + [rng.getrandbits(256) for _ in range(2000)]:
        assert lr.sc_ge_n(a)[0] == int(a >= N) and lr.sc_is_high(a)[0] == int(a > lr.HALF), a
        assert lr.sc_reduce_once(a)[0] == a % N and lr.sc_key_from_hash(a)[0] == a % (N - 1) + 1, a
    # a fold on its own: 8 high limbs of all ones, the largest thing the first fold is handed
    out, t = lr.sc_fold(lr.limbs(lr.ONES), lr.limbs(lr.ONES), 8, 14)
    assert lr.value(out) == lr.ONES + lr.ONES * C and not t["lost"]


def test_recoding_values():
    rng = random.Random(3)
    for k in lr.recode_set() + [rng.randrange(lr.HALF + 1) for _ in range(2000)]:
        (mag, sgn), t = lr.recode_signed4(k)
        assert lr.recode_canonical(mag, sgn & lr.M32, sgn >> 32) == lr.recode_by_division(k), k
        assert sum(d * 16**i for i, d in enumerate(t["digits"])) == k and all(-7 <= d <= 8 for d in t["digits"]), k
        assert not t["carries"][63], k


def test_fp_product_census(census):
    seen = census["fp_mul"]
    assert min(seen.get(o, 0) for o in ("none", "ge", "carry")) >= 20, seen
    assert [lr.fp_mul(P - 1, P - u)[1]["outcome"] for u in (K - 1, K, K + 1)] == ["ge", "carry", "carry"]
    assert {(P - 1, P - u) for u in (K - 1, K, K + 1)} <= set(lr.fp_pairs())
    assert {0, 0x1000003D0} <= census["fp_mul_top"]
    # (p - u)(p - v) = u v modulo p: the ge arm below K, the carry arm from K on
    for u, v in ((1, K - 1), (2, 977), (976, 978)):
        assert lr.fp_mul(P - u, P - v)[1]["outcome"] == "ge"
    for u, v in ((1, K), (977, 1 << 32), (K, K - 1)):
        assert lr.fp_mul(P - u, P - v)[1]["outcome"] == "carry"
    assert census["fp_sqr"][P - 65536] == "ge" and census["fp_sqr"][P - 65537] == "carry"


def test_sc_product_census(census):
    seen = census["sc_mul"]
    assert min(seen.get(o, 0) for o in ("none", "ge", "carry")) >= 10, seen
    for o in ("ge", "none"):
        assert 0 in census["sc_w2_8"][o] and any(census["sc_w2_8"][o] - {0}), o
    t = lr.sc_mul(N - 1, N - 1)[1]
    assert (t["outcome"], t["w2_8"]) == ("ge", 1)
    assert lr.sc_mul(N - 1, N - C)[1]["outcome"] == "carry"
    # (2^128 - 1)^2 = 2^256 - 2^129 + 1 is below n (2^129 > 2^256 - n): no correction; (2^128 - 1) 2^128 is not
    t = lr.sc_mul((1 << 128) - 1, (1 << 128) - 1)[1]
    assert (t["outcome"], t["w2_8"]) == ("none", 0)
    t = lr.sc_mul((1 << 128) - 1, 1 << 128)[1]
    assert (t["outcome"], t["w2_8"]) == ("ge", 0)
    assert {(N - 1, N - 1), (N - 1, N - C), ((1 << 128) - 1, (1 << 128) - 1), ((1 << 128) - 1, 1 << 128)} <= set(lr.sc_pairs())


def test_sum_and_difference_census(census):
    assert 7 in census["fp_sub_depth"] and {0, 1} <= census["fp_sub_depth"]
    assert {P - 1, P, (1 << 256) - 1, 1 << 256, (1 << 256) + 1} <= census["fp_add_sums"]
    assert census["sc_add"] == {"none", "ge", "carry"}
    sums = {a + b for a, b in lr.sc_pairs()}
    assert {N - 1, N, (1 << 256) - 1, 1 << 256} <= sums


def test_recoding_census():
    tags = [lr.recode_signed4(k)[1] for k in lr.recode_set()]
    for window in (0, 31, 62):
        assert any(t["carries"][window] for t in tags), window
    assert not any(t["carries"][63] for t in tags)
    digits = {d for t in tags for d in t["digits"]}
    assert {7, 8, -7} <= digits
    assert 0 in lr.recode_set() and all(k <= lr.HALF for k in lr.recode_set()) and len(lr.recode_set()) >= len(sg.edge_keys()) - 2


def test_comparison_sets():
    a = set(lr.any256())
    assert {N - 2, N - 1, N, N + 1, lr.ONES, lr.HALF - 1, lr.HALF, lr.HALF + 1, P - 1, P, P + 1} <= a
    assert len(lr.FP_SCALARS) >= 40 and len(lr.SC_SCALARS) >= 30 and all(v < P for v in lr.FP_SCALARS) and all(v < N for v in lr.SC_SCALARS)


def test_ladder_cases_are_what_they_say():
    cases = lr.ladder_cases()
    assert len(cases) == 8 * 11 * 11 + 13
    by_name = {c[0]: c for c in cases}
    assert by_name["through infinity"][4] == sr.G and by_name["cancel 1"][4] is None
    infinite = [c for c in cases if c[4] is None]
    assert len(infinite) >= 20
    hx = lr.ladder_bases()["x>=n"]
    assert sr.on_curve(hx) and N <= hx[0] < P
    rng = random.Random(4)
    for name, pt, u2, u1, want in rng.sample(cases, 40):
        assert sr.on_curve(pt) and want == sr.add(sr.mul(u2, pt), sr.mul(u1, sr.G)), name


def test_hook_signature_matches_header(zk):
    """zk-proof-of-assets_amd/_abi.py's SECP_PRIM_SIGNATURES against include/zkpoa_secp_prim.h, as tests/test_abi.py holds
    the main table against zkpoa_prover.h; the public header takes the hook in by an #include beside its test hooks."""
    from test_abi import _c_class, _ctypes_class
    from zkpoa_amd import _abi
    text = open(os.path.join(ROOT, "include", "zkpoa_secp_prim.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    protos = {name: (_c_class(ret + " ret"), [_c_class(a.strip().replace("struct ", "")) for a in args.split(",")])
              for ret, name, args in re.findall(r"([\w \t*]+?[\s*])(zkpoa_\w+)\s*\(([^()]*)\)\s*;", text)}
    assert list(protos) == list(_abi.SECP_PRIM_SIGNATURES) == ["zkpoa_secp_prim"]
    restype, argtypes = _abi.signature(_abi.SECP_PRIM_SIGNATURES["zkpoa_secp_prim"])
    assert (_ctypes_class(restype), [_ctypes_class(t) for t in argtypes]) == protos["zkpoa_secp_prim"]
    fn = zk.lib().zkpoa_secp_prim
    assert list(fn.argtypes) == argtypes and fn.restype == restype
    main = open(os.path.join(ROOT, "include", "zkpoa_prover.h")).read()
    assert '#include "zkpoa_secp_prim.h"' in main
    assert main.index("zkpoa_fq29_prim(") < main.index('#include "zkpoa_secp_prim.h"') < main.index("zkpoa_ntt_form(")
    assert sorted(v[0] for v in lr.OPS.values()) == list(range(21))
