"""The MSM planner (csrc/msm_plan.hpp msm_make_plan) and the workspace sizes of its plans (csrc/msm.hip.h layouts) against
tests/golden/gen/msm_plan.json, through the test hook zkpoa_test_msm_plan. No GPU. The file was recorded from the planner
as it stood while the scalars' digit density was a thread-local hint and the forced piece length a process-wide static:
a plan is now a function of its request alone, and every plan, entry form and byte count is what it was.

The grid: n x c x for_g2 x merged x density in the file's order, k0 = 0; then k0_rows: n x merged x density x k0 with
c = 0 and for_g2 = 0. Densities are 32 doubles indexed by the window width: bits d[c] = 1, limbs64 d[c] = ceil(64 / c),
uniform d[c] = ceil(254 / c) (the density branch with the entry count of no density at all)."""
import ctypes
import itertools
import json
import os

import pytest

from conftest import ROOT

OUT = ["c", "W", "Wb", "ne", "TB", "K0", "K", "logS", "logRows", "sparse", "sort_bytes", "g1_accum_bytes", "g2_accum_bytes"]


def density(kind):
    per = {"none": None, "bits": lambda c: 1, "limbs64": lambda c: -(-64 // c), "uniform": lambda c: -(-254 // c)}[kind]
    return None if per is None else (ctypes.c_double * 32)(*[float(per(max(c, 1))) for c in range(32)])


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "gen", "msm_plan.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def plan(zk):
    f = zk.lib().zkpoa_test_msm_plan
    dens = {kind: density(kind) for kind in ("none", "bits", "limbs64", "uniform")}

    def call(n, c, for_g2, merged, kind, k0=0, cap=13):
        out = (ctypes.c_uint64 * 13)(*([0xdead] * 13))
        rc = f(n, c, merged, for_g2, dens[kind], k0, out if cap is not None else None, cap or 0)
        return rc, list(out)
    call.raw = f
    return call


def grid(golden):
    assert golden["order"] == ["n", "c", "for_g2", "merged", "density"] and golden["out"] == OUT
    assert golden["n"] == [0, 1, 255, 1024, 3000, 60000, 1 << 16, 1 << 20, 1 << 24, 1 << 26, 1 << 27, 1 << 28]
    assert golden["c"] == [0, 3, 4, 14, 22, 23, 25, 26] and golden["for_g2"] == [0, 1] and golden["merged"] == [0, 1]
    assert golden["density"] == ["none", "bits", "limbs64", "uniform"]
    keys = list(itertools.product(*(golden[a] for a in golden["order"])))
    assert len(keys) == len(golden["rows"]) == 1536
    return list(zip(keys, golden["rows"]))


def k0_grid(golden):
    assert golden["k0_order"] == ["n", "merged", "density", "k0"]
    assert golden["k0_n"] == [3000, 1 << 20] and golden["k0_density"] == ["none", "bits"] and golden["k0"] == [7, 8, 64, 512, 513]
    keys = list(itertools.product(golden["k0_n"], [0, 1], golden["k0_density"], golden["k0"]))
    assert len(keys) == len(golden["k0_rows"]) == 40
    return list(zip(keys, golden["k0_rows"]))


def test_every_plan_equals_the_recorded_one(plan, golden):
    for (n, c, for_g2, merged, kind), want in grid(golden):
        assert plan(n, c, for_g2, merged, kind) == (13, want), (n, c, for_g2, merged, kind)
    for (n, merged, kind, k0), want in k0_grid(golden):
        assert plan(n, 0, 0, merged, kind, k0) == (13, want), (n, merged, kind, k0)


def test_recorded_plans_follow_the_stated_rules(golden):
    """The file itself against the rules csrc/msm_plan.hpp and csrc/msm.hip.h state."""
    rows = {k: dict(zip(OUT, r)) for k, r in grid(golden)}
    for (n, c, for_g2, merged, kind), p in rows.items():
        assert p["W"] == -(-254 // p["c"]) and p["Wb"] == (1 if merged else p["W"])
        assert p["TB"] == p["Wb"] << (p["c"] - 1) and p["logS"] + p["logRows"] == p["c"] - 1 and 0 <= p["logS"] - p["logRows"] <= 1
        assert p["ne"] == (n * p["W"] if merged else n) % (1 << 32) and p["K"] == 4
        assert p["K0"] in (32, 64, 128, 256)                         # a power of two in 32..256 unless forced
        if for_g2:
            assert p["K0"] <= 64                                     # a quarter of the G1 length, at least 32
        if c in range(4, 26 if merged else 23):
            assert p["c"] == c                                       # a valid width is taken as it is ...
        else:
            assert p == rows[(n, 0, for_g2, merged, kind)]           # ... any other is ignored: the cost model's
            assert 4 <= p["c"] <= (25 if merged else 22)
        # the compact entry list: fixed-base form only, and only for scalars with few non-zero digits
        d = {"bits": 1, "limbs64": -(-64 // p["c"]), "uniform": p["W"]}.get(kind)
        assert p["sparse"] == int(bool(merged and n and d is not None and d < 0.6 * p["W"]))
        assert all(p[b] == 0 for b in OUT[10:]) if n == 0 else all(p[b] > 0 for b in OUT[10:])
    # fewer digits per scalar: the model never picks a narrower window for them
    for n, for_g2, merged in itertools.product(golden["n"], [0, 1], [0, 1]):
        assert rows[(n, 0, for_g2, merged, "bits")]["c"] <= rows[(n, 0, for_g2, merged, "none")]["c"] or n == 0
    # forced piece length: 8..512 is taken, anything else leaves the rule's
    for (n, merged, kind, k0), r in k0_grid(golden):
        base = rows[(n, 0, 0, merged, kind)]
        p = dict(zip(OUT, r))
        assert p["K0"] == (k0 if 8 <= k0 <= 512 else base["K0"]) and [p[b] for b in OUT[:5]] == [base[b] for b in OUT[:5]]
        if not 8 <= k0 <= 512:
            assert p == base


def test_hook_argument_checks(plan):
    ok = plan(1024, 0, 0, 0, "none")
    assert ok[0] == 13
    assert plan((1 << 28) + 1, 0, 0, 0, "none")[0] == -1
    assert plan(1024, -1, 0, 0, "none")[0] == -1 and plan(1024, 32, 0, 0, "none")[0] == -1
    assert plan(1024, 0, 2, 0, "none")[0] == -1 and plan(1024, 0, 0, 2, "none")[0] == -1 and plan(1024, 0, 0, -1, "none")[0] == -1
    assert plan(1024, 0, 0, 0, "none", k0=-1)[0] == -1
    assert plan(1024, 0, 0, 0, "none", cap=None)[0] == 13            # no buffer, nothing to write: only the count
    null = ctypes.POINTER(ctypes.c_uint64)()
    assert plan.raw(1024, 0, 0, 0, None, 0, null, 13) == -1      # ... but a null buffer with room promised is refused
    rc, short = plan(1024, 0, 0, 0, "none", cap=4)                    # a short buffer: the first words, the rest untouched
    assert rc == 13 and short[:4] == ok[1][:4] and short[4:] == [0xdead] * 9
