"""Every MSM kernel stays inside the region the workspace layout gave it (csrc/msm.hip.h MsmSortLayout / MsmAccumLayout,
carved from one lane arena, csrc/device_ctx.hpp Arena). Under ZKPOA_WS_GUARD=1 every region is followed by guard bytes
that start at its exact size; both phases of an MSM look at all of them when their kernels have finished, and a changed
byte fails the call with an error that names the region. The parity tests cannot see such a write: it lands in padding,
or in a neighbour that is written later.

Every case here runs under the guard and asserts two things: the call raises nothing, and the result equals the C oracle
(or the golden proof). The shapes fill the regions to the counts the layout states: every bucket two pieces (level-0
pieces at >= 0.9 of msm_piece_cap), one bucket holding all n (the partial-sum levels at full depth), every sort-pass
count and reduction split, the scan-tile boundary, tiny n, the fixed-base, chunked and shared-sort forms, the
three-launch scans. The last tests check the check: ZKPOA_TEST_WS_CLOBBER=k lets the host overwrite one byte of the k-th
guard, the MSM must fail naming that region, and the same context must compute correctly afterwards."""
import contextlib
import functools
import json
import os
import random
import subprocess
import sys

import pytest

from conftest import ROOT, golden_case, le
from oracle import c_oracle as co
import msm_sort_ref as ref

pytestmark = pytest.mark.gpu
R = ref.R
GUARD_ERROR = "workspace guard"


@pytest.fixture(autouse=True)
def guarded(monkeypatch):
    """the row is read at every use: each test of this module runs with the guard on and the self-test hook off"""
    monkeypatch.setenv("ZKPOA_WS_GUARD", "1")
    monkeypatch.delenv("ZKPOA_TEST_WS_CLOBBER", raising=False)


@contextlib.contextmanager
def forced(ctx, c=0, k0=0, max_points=0):
    ctx.set_option("msm_c", c)
    ctx.set_option("msm_k0", k0)
    ctx.set_option("msm_max_points", max_points)
    try:
        yield
    finally:
        ctx.set_option("msm_c", 0)
        ctx.set_option("msm_k0", 0)
        ctx.set_option("msm_max_points", 0)


@functools.lru_cache(maxsize=None)
def bases(group, n):
    """n distinct random points, computed once per (group, n) and shared by the tests of that size"""
    rng = random.Random("ws-bases-%d-%d" % (group, n))
    fb = co.fixed_base_g1 if group == 1 else co.fixed_base_g2
    return fb(b"".join(le(rng.randrange(1, R)) for _ in range(n)), 8)


def point_bytes(group):
    return 64 if group == 1 else 128


@functools.lru_cache(maxsize=None)
def oracle(group, n, scal):
    """the C oracle's sum over the shared bases: once per (group, n, scalars)"""
    sc = b"".join(le(s) for s in scal)
    return (co.msm_g1 if group == 1 else co.msm_g2)(bases(group, n), sc, n, 8)


def run_msm(ctx, group, n, scal):
    """the MSM under the guard: a guard hit would raise here"""
    sc = b"".join(le(s) for s in scal)
    fn = ctx.msm_g1 if group == 1 else ctx.msm_g2
    return fn(bases(group, n), sc, n)


def witness_like(rng, n):
    out = []
    for _ in range(n):
        u = rng.random()
        out.append(rng.randrange(2) if u < 0.55 else rng.randrange(1 << 64) if u < 0.9 else rng.randrange(R))
    return tuple(out)


def uniform(rng, n):
    return tuple(rng.randrange(R) for _ in range(n))


# ---- a. regions filled to their stated counts ------------------------------------------------------------------------
def two_pieces_per_bucket(c, k0):
    """n = Nb * (K0 + 1) scalars; scalar i has the digit ((i + w) mod Nb) + 1 in every window below the top one and zero
    there: every bucket of those windows holds K0 + 1 entries, i.e. two pieces. The digits are at most Nb (no carry) and
    the value stays below 2^(c (W - 1)) <= (r - 1) / 2 (no sign flip), so the recoding leaves them as they are."""
    nb, W = 1 << (c - 1), ref.windows(c)
    n = nb * (k0 + 1)
    scal = tuple(ref.digits_value([(((i + w) % nb) + 1, 0) for w in range(W - 1)], c) for i in range(n))
    assert max(scal) <= ref.HALF
    return scal


# (c, K0) -> n, level-0 pieces, msm_piece_cap = n * W / K0 + TB + 1: worked out by hand from the construction
FILLED = {(4, 8): (72, 1008, 1089), (5, 8): (144, 1600, 1735), (9, 8): (2304, 14336, 15777), (4, 32): (264, 1008, 1041)}


@pytest.mark.parametrize("c,k0,group", [(4, 8, 1), (5, 8, 1), (9, 8, 1), (4, 32, 1), (4, 8, 2)])
def test_every_bucket_two_pieces_fills_the_piece_regions(ctx, c, k0, group):
    """pbkt, order (msm_piece_cap words each) and P1 (msm_piece_cap sums) at >= 0.9 of their count, elist / sorted at
    ~0.98 of n * W -- asserted from the plan that ran and the totals phase A returned, which equal the model's"""
    scal = two_pieces_per_bucket(c, k0)
    n, pieces, cap = FILLED[(c, k0)]
    assert len(scal) == n
    got = ctx.test_msm_sort(b"".join(le(s) for s in scal), n, c, for_g2=group == 2, k0=k0)
    plan = dict(zip(("c", "W", "Wb", "ne", "TB", "K0"), got["plan"]))
    assert (plan["c"], plan["K0"]) == (c, k0)
    piece_cap = n * plan["W"] // plan["K0"] + plan["TB"] + 1
    assert piece_cap == cap
    model = ref.sort_result(scal, c, False, k0)
    assert (got["total_entries"], got["max_count"], got["total1"]) == (model["total_entries"], model["max_count"], model["total1"])
    assert got["total1"] == pieces and got["max_count"] == k0 + 1
    assert got["total1"] >= 0.9 * piece_cap, (got["total1"], piece_cap)
    assert got["total_entries"] == n * (plan["W"] - 1) >= 0.96 * n * plan["W"]
    with forced(ctx, c, k0):
        assert run_msm(ctx, group, n, scal) == oracle(group, n, scal)


# ---- b. one bucket holds everything ------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [4, 9])
@pytest.mark.parametrize("value", [1, R - 1])
def test_one_bucket_holds_everything(ctx, c, value):
    """4097 scalars equal to 1 (or r - 1): max_count == n, so the partial-sum levels run to full depth and P1 / P2
    ping-pong against p2_cap = p1_cap / 2 + 1; one segment per window is the most skewed input of a multi-pass sort"""
    n, k0 = 4097, 8
    scal = (value,) * n
    got = ctx.test_msm_sort(b"".join(le(s) for s in scal), n, c, k0=k0)
    assert got["max_count"] == n and got["total_entries"] == n and got["total1"] == -(-n // k0)
    with forced(ctx, c, k0):
        assert run_msm(ctx, 1, n, scal) == oracle(1, n, scal)


# ---- c. every sort-pass count and reduction split ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def witness_case(n):
    return witness_like(random.Random("ws-witness-%d" % n), n)


@pytest.mark.parametrize("c", [4, 5, 8, 9, 10, 11, 14, 16, 17, 18, 20, 22])
def test_forced_windows_g1(ctx, c):
    """the widths and sizes of test_gpu_kernels.test_msm_forced_windows: one, two and three sort passes, odd and even
    splits of the bucket matrix"""
    n = 4096 if c < 16 else 40000
    scal = witness_case(n)
    with forced(ctx, c):
        assert run_msm(ctx, 1, n, scal) == oracle(1, n, scal)


@pytest.mark.parametrize("c", [4, 8, 9, 16, 17])
def test_forced_windows_g2(ctx, c):
    n = 700
    scal = witness_case(n)
    with forced(ctx, c):
        assert run_msm(ctx, 2, n, scal) == oracle(2, n, scal)


@pytest.mark.parametrize("c,tb", [(6, 1376), (7, 2368)])
def test_bucket_counts_on_either_side_of_one_scan_tile(ctx, c, tb):
    """TB = 1376 and 2368: below and above one scan tile of 2048 words (block_sums, the scans' second tile)"""
    n = 300
    assert ref.windows(c) << (c - 1) == tb and (tb < 2048) == (c == 6)
    scal = witness_case(n)
    with forced(ctx, c):
        for group in (1, 2):
            assert run_msm(ctx, group, n, scal) == oracle(group, n, scal)


# ---- d. small n --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257])
def test_small_n(ctx, n):
    scal = uniform(random.Random("ws-small-%d" % n), n)
    for c in (4, 0):                                       # forced, and the plan's own window
        with forced(ctx, c):
            for group in (1, 2):
                got = run_msm(ctx, group, n, scal)
                assert got == (oracle(group, n, scal) if n else bytes(point_bytes(group))), (c, group)


# ---- e. the other forms ------------------------------------------------------------------------------------------------
def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


@pytest.mark.parametrize("dist", ["uniform", "witness"])
def test_fixed_base_table_msm(ctx, dist):
    """the merged plan (one bucket set, n * W entries in it) through a table, dense uniform and sparse witness-like scalars"""
    n = 3000
    rng = random.Random("ws-table-" + dist)
    scal = uniform(rng, n) if dist == "uniform" else witness_like(rng, n)
    d_b, d_s = _dev(bases(1, n)), _dev(b"".join(le(s) for s in scal))
    table = ctx.msm_table(1, d_b.data_ptr(), n, 0)
    try:
        want = oracle(1, n, scal)
        assert ctx.msm_table_run(table, d_s.data_ptr()) == want
        assert ctx.msm_table_run(table, d_s.data_ptr(), lane=3) == want
    finally:
        table.close()


def test_chunked_msm(ctx):
    """msm_max_points = 40, n = 200: five MSMs in a row in one arena, each carving and stamping it anew"""
    n = 200
    scal = witness_case(n)
    with forced(ctx, max_points=40):
        for group in (1, 2):
            assert run_msm(ctx, group, n, scal) == oracle(group, n, scal)


@pytest.mark.parametrize("tables", [False, True])
@pytest.mark.parametrize("tag", ["n8", "n128"])
def test_golden_proofs_bit_exact(ctx, zk, tag, tables):
    """a whole proof: A, B1 and B2 share one sort, so B2 (and A or B1) accumulate in an arena of their own over another
    lane's sort regions (own_arena == false), and the lanes are sized by the prover's budget"""
    g = golden_case(tag)
    rs = json.loads(g["rs.json"])
    key = ctx.load_zkey(g["circuit.zkey"])
    try:
        if tables:
            assert key.precompute() > 0
        for _ in range(2):
            pts, pub = ctx.prove(key, g["witness.wtns"], int(rs["r"]), int(rs["s"]))
            assert zk.proof_to_json(pts) == g["proof_rapidsnark.json"]
            assert zk.public_to_json(pub) == g["public_rapidsnark.json"]
    finally:
        key.close()


_SCAN3_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as entry
c = entry.load_package().Context(0)
read = lambda name: open(sys.argv[2] + "/" + name, "rb").read()
print(c.msm_g1(read("b1"), read("s"), 700).hex())
print(c.msm_g2(read("b2"), read("s"), 700).hex())
c.close()
"""


def test_three_launch_scans_under_the_guard(tmp_path):
    """ZKPOA_SCAN=3 is latched: a fresh child under a time limit of its own, with both variables set, runs one G1 and one
    G2 MSM (the three-launch scans write block_sums, which the one-launch scans leave alone)"""
    n = 700
    scal = witness_case(n)
    for name, data in (("b1", bases(1, n)), ("b2", bases(2, n)), ("s", b"".join(le(s) for s in scal))):
        (tmp_path / name).write_bytes(data)
    rc = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-s", "-c", _SCAN3_CHILD, ROOT, str(tmp_path)],
                        env=dict(os.environ, ZKPOA_SCAN="3", ZKPOA_WS_GUARD="1"), capture_output=True, text=True)
    assert rc.returncode == 0, rc.stdout + rc.stderr
    assert GUARD_ERROR not in rc.stderr
    got1, got2 = (bytes.fromhex(h) for h in rc.stdout.split())
    assert got1 == oracle(1, n, scal) and got2 == oracle(2, n, scal)


# ---- f. the check itself -----------------------------------------------------------------------------------------------
# the regions of a one-pass sort (c - 1 <= 8 key bits) and of the accumulation, in arena order
SORT_1PASS = ["counts", "misc", "len_hist", "off0", "po_a", "elist", "pre", "base[0]", "sorted", "block_sums", "pbkt", "order"]
ACCUM = ["po_b", "po_c", "accum block_sums", "accum misc", "buckets", "P1", "P2", "X", "Y1", "Y2"]


def guard_bytes(exact):
    """a region of `exact` bytes: its guard runs from there to the 256-byte rounded end plus 256 bytes"""
    return -exact % 256 + 256


@pytest.mark.parametrize("region,phase", [("counts", "sort"), ("misc", "sort"), ("P2", "accumulation")])
def test_a_clobbered_guard_fails_the_msm_and_names_the_region(zk, monkeypatch, region, phase):
    """No kernel is involved: the host overwrites one byte of the k-th guard (inside the arena's own allocation) just
    before the phase looks at its guards. The MSM fails with the guard error naming that region; with the hook back at
    0 the same context computes the same MSM correctly, still under the guard. The guard's length in the message shows
    where it begins: at the region's exact size (misc: 16 words, so 192 bytes of padding belong to the guard; P2: p2_cap
    sums of 128 bytes), not at the rounded end -- a one-word overrun is inside it."""
    import ctypes
    n, c = 300, 4
    scal = witness_case(n)
    regions = SORT_1PASS + ACCUM
    k = regions.index(region) + 1
    assert (k <= len(SORT_1PASS)) == (phase == "sort")
    words = (ctypes.c_uint64 * 13)()
    assert zk.lib().zkpoa_test_msm_plan(n, c, 0, 0, None, 0, words, 13) == 13
    W, TB, K0 = words[1], words[4], words[5]
    p2_cap = (n * W // K0 + TB + 1) // 2 + 1
    length = guard_bytes({"counts": TB * 4, "misc": 16 * 4, "P2": p2_cap * 128}[region])
    assert {"counts": length == 256, "misc": length == 448, "P2": length == 384}[region]
    ctx = zk.Context(0)
    try:
        ctx.set_option("msm_c", c)
        monkeypatch.setenv("ZKPOA_TEST_WS_CLOBBER", str(k))
        with pytest.raises(zk.ZkpoaError) as err:
            run_msm(ctx, 1, n, scal)
        text = str(err.value)
        print(text)
        assert GUARD_ERROR in text and "the %s phase" % phase in text and "region '%s'" % region in text
        assert "(guard %d of %d)" % (k, len(SORT_1PASS) if phase == "sort" else len(regions)) in text
        assert "first changed byte at offset 0 of the guard's %d bytes" % length in text
        monkeypatch.setenv("ZKPOA_TEST_WS_CLOBBER", "0")
        assert run_msm(ctx, 1, n, scal) == oracle(1, n, scal)
        monkeypatch.delenv("ZKPOA_WS_GUARD")                      # and with the guard off again
        assert run_msm(ctx, 1, n, scal) == oracle(1, n, scal)
    finally:
        ctx.close()


def test_the_clobber_hook_does_nothing_without_the_guard(ctx, monkeypatch):
    monkeypatch.delenv("ZKPOA_WS_GUARD")
    monkeypatch.setenv("ZKPOA_TEST_WS_CLOBBER", "1")
    n = 300
    scal = witness_case(n)
    assert run_msm(ctx, 1, n, scal) == oracle(1, n, scal)
