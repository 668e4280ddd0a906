"""The Fr NTT's pass plans (csrc/ntt.hip.h ntt_plan) for every size 2^0 .. 2^28 at the default and at both forced tile
sizes, against tests/golden/gen/ntt_plan.json: the passes and the launch geometry recorded from the code as it stood
before the plan became one function of (k, tile_log). No GPU: the plans of 2^23 .. 2^28 are otherwise reached only by
proofs and transforms of that size."""
import ctypes
import json
import os

import pytest

from conftest import ROOT

TILES = {"default": 0, "tile10": 10, "tile11": 11}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "gen", "ntt_plan.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def plan(zk):
    f = zk.lib().zkpoa_test_ntt_plan

    def call(k, tile_log, cap=7 * 8):
        out = (ctypes.c_uint32 * max(cap, 1))()
        n = f(k, tile_log, out, cap)
        return n, [list(out[7 * i:7 * i + 7]) for i in range(min(max(n, 0), cap // 7))]
    return call


@pytest.mark.parametrize("tile", sorted(TILES))
def test_every_plan_equals_the_recorded_one(plan, golden, tile):
    assert golden["fields"] == ["s_lo", "B", "logT", "grid_x", "threads", "lds_bytes", "direct"]
    assert len(golden[tile]) == 29
    for k, want in enumerate(golden[tile]):
        n, got = plan(k, TILES[tile])
        assert (n, got) == (len(want), want), "k=%d %s" % (k, tile)


def test_recorded_plans_are_the_documented_splits(golden):
    """The golden file itself against the splits DESIGN.md states, and the rules for threads, LDS and grid."""
    stages = {t: ["+".join(str(p[1]) for p in plan) for plan in golden[t]] for t in TILES}
    d = stages["default"]
    assert d[0] == "" and d[1:12] == [str(k) for k in range(1, 12)]
    assert d[12:22] == ["11+%d" % (k - 11) for k in range(12, 22)]
    assert d[22:] == ["11+6+5", "10+7+6", "10+7+7", "10+8+7", "10+8+8", "10+6+6+5", "10+6+6+6"]
    assert [p[2] for p in (plan[1] for plan in golden["default"][12:22])] == [22 - k for k in range(12, 22)]
    t10 = stages["tile10"]
    assert t10[11:20] == ["10+%d" % (k - 10) for k in range(11, 20)]
    assert t10[20:23] == ["10+5+5", "10+6+5", "10+6+6"] and t10[23:] == d[23:]
    assert [p[6] for p in golden["tile10"][20]] == [0, 1, 1] and [p[6] for p in golden["tile10"][22]] == [0, 1, 0]
    for t in TILES:
        for k, plan in enumerate(golden[t]):
            assert sum(p[1] for p in plan) == k
            for s_lo, B, logT, grid, threads, lds, direct in plan:
                tl = B + logT
                assert logT <= s_lo and grid << tl == 1 << k and lds == 32 << tl
                assert threads == (64 if tl <= 8 else 512 if tl == 11 else 1 << (tl - 2))
                assert direct == (1 if s_lo > 0 and s_lo + B <= 21 else 0)


def test_hook_argument_checks(plan):
    assert plan(29, 0)[0] == -1 and plan(5, 9)[0] == -1 and plan(5, 12)[0] == -1 and plan(5, 1)[0] == -1
    assert plan(0, 0) == (0, [])
    n, got = plan(28, 0, cap=7 * 2 + 3)          # a short buffer: the count is whole, only whole passes are written
    assert n == 4 and len(got) == 2 and got == plan(28, 0)[1][:2]
