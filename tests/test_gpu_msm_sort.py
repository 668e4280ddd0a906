"""Phase A of the MSM (csrc/msm.hip.h msm_sort_phase: digits or the compact entry list, up to three count / scan / scatter
passes, the paired scans, the piece ordering) stage by stage, through the test hook zkpoa_test_msm_sort, against the
plain reference tests/msm_sort_ref.py; and the witness density measurement (zkpoa_test_msm_density). Every comparison
is exact. The final point of an MSM does not see a wrong piece order, an oversized max_count, a wrong piece-length
histogram or a wrong density -- these tests do, and they name the stage and the bucket."""
import ctypes
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, le
from oracle import c_oracle as co
import msm_sort_ref as ref

pytestmark = pytest.mark.gpu
R, HALF = ref.R, ref.HALF
CH = 16384              # entries per sort task (msm_sort.hip.h SortPlan::CH)
WG_SCALARS = 2048       # scalars per workgroup of msm_entries_kernel, which stages up to WG_STAGE entries in LDS
WG_STAGE = 8192
PLAN_WORDS = ("c", "W", "Wb", "ne", "TB", "K0", "K", "logS", "logRows", "sparse", "sort_bytes", "g1_bytes", "g2_bytes")


# ---- inputs ----------------------------------------------------------------------------------------------------------
def witness_like(rng, n, bits=0.55, limbs=0.35):
    """bits, 64-bit limbs and a rest of full-width values, as a witness has them"""
    out = []
    for _ in range(n):
        u = rng.random()
        out.append(rng.randrange(2) if u < bits else rng.randrange(1 << 64) if u < bits + limbs else rng.randrange(R))
    return tuple(out)


def uniform(rng, n):
    return tuple(rng.randrange(R) for _ in range(n))


def mixed(rng, n):
    half = n // 2
    out = list(uniform(rng, half)) + list(witness_like(rng, n - half))
    rng.shuffle(out)
    return tuple(out)


def pass_bits(c):
    """key bits per sort pass, as make_sort_plan splits the c - 1 bucket bits (from the top, at most 8 per pass)"""
    left = c - 1
    npass = 1 if left <= 8 else -(-left // 8)
    out = []
    for l in range(npass):
        out.append(-(-left // (npass - l)))
        left -= out[-1]
    return out


# ---- the checker -----------------------------------------------------------------------------------------------------
def plan_words(zk, n, c, merged, for_g2, density, k0):
    dens = (ctypes.c_double * 32)(*density) if density is not None else None
    out = (ctypes.c_uint64 * 13)()
    assert zk.lib().zkpoa_test_msm_plan(n, c, int(merged), int(for_g2), dens, k0, out, 13) == 13
    return list(out)


@functools.lru_cache(maxsize=2)
def reference(scal, c, merged, k0):
    """computed once per (input, width, form, piece length), shared by the tests that run the case, never changed"""
    res = ref.sort_result(scal, c, merged, k0)
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


def check(zk, ctx, scal, c=0, merged=False, for_g2=False, density=None, k0=0, lane=0):
    """run phase A on the device and compare all it hands on with the reference -> (device result, reference, plan)"""
    n = len(scal)
    words = plan_words(zk, n, c, merged, for_g2, density, k0)
    plan = dict(zip(PLAN_WORDS, words))
    got = ctx.test_msm_sort(b"".join(le(s) for s in scal), n, c, merged, for_g2, density, k0, lane)
    assert got["plan"] == words
    assert c == 0 or plan["c"] == c
    want = reference(scal, plan["c"], bool(merged), plan["K0"])
    assert (plan["W"], plan["TB"]) == (want["W"], want["TB"])
    dev = {k: np.frombuffer(got[k], dtype=np.uint32) for k in ("counts", "off0", "po_a", "sorted", "pbkt", "order", "len_hist")}

    def same(name):
        bad = np.nonzero(dev[name] != want[name].astype(np.uint32))[0] if len(dev[name]) == len(want[name]) else None
        assert bad is not None, "%s: %d words, expected %d" % (name, len(dev[name]), len(want[name]))
        assert len(bad) == 0, "%s differs first at index %d: %d, expected %d" % (
            name, bad[0], dev[name][bad[0]], want[name][bad[0]])
    same("counts")
    same("off0")
    same("po_a")
    for k in ("total_entries", "max_count", "total1"):
        assert got[k] == want[k], k
    same("len_hist")
    # the payloads of every bucket as a multiset: order inside a bucket is free
    bucket_of = np.repeat(np.arange(plan["TB"], dtype=np.int64), want["counts"])
    keys = ref.keys(bucket_of, dev["sorted"])
    bad = np.nonzero(keys != want["keys"])[0]
    first = [int(k[bad[0]]) for k in (keys, want["keys"])] if len(bad) else [0, 0]
    assert len(bad) == 0, "bucket %d: payload %#x, expected %#x in bucket %d" % (
        first[0] >> 32, first[0] & 0xffffffff, first[1] & 0xffffffff, first[1] >> 32)
    same("pbkt")
    order = dev["order"].astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(want["total1"])), "order is no permutation of the pieces"
    lens = want["piece_len"][order]
    rise = np.nonzero(lens[1:] > lens[:-1])[0]
    assert len(rise) == 0, "order: piece %d (length %d) comes before piece %d (length %d)" % (
        order[rise[0]], lens[rise[0]], order[rise[0] + 1], lens[rise[0] + 1])
    return got, want, plan


# ---- the cases: name -> (scalars, request), built once ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    rng = random.Random("msm-sort-" + name)
    kind, _, arg = name.partition(":")
    if kind == "classic" or kind == "merged":          # a few thousand scalars, no multiple of 256
        return mixed(rng, 3001), dict(c=int(arg), merged=kind == "merged")
    if kind == "chunks":                               # pass 0: three chunks per window, the last ragged
        return mixed(rng, 2 * CH + 37), dict(c=13)
    if kind == "hot_segment":                          # > CH scalars are 1 or r - 1: one later-pass segment spans two tasks
        scal = [rng.choice((1, R - 1)) for _ in range(CH + 2000)] + list(witness_like(rng, 40000 - CH - 2000, 0.2, 0.6))
        rng.shuffle(scal)
        return tuple(scal), dict(c=int(arg))
    if kind == "edges":
        scal = ref.edge_scalars(int(arg)) + list(uniform(rng, 700))
        rng.shuffle(scal)
        return tuple(scal), dict(c=int(arg))
    raise KeyError(name)


# ---- pass structure --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["classic:4", "classic:9", "classic:10", "classic:17", "classic:18", "classic:22",
                                  "merged:17", "merged:25"])
def test_widths_on_both_sides_of_every_pass_boundary(zk, ctx, name):
    """c - 1 key bits: one pass up to 8 (c = 4, 9), two up to 16 (10, 17), three beyond (18, 22: 7 + 7 + 7); merged c = 25:
    24 bits, 8 + 8 + 8"""
    scal, req = case(name)
    assert len(scal) % 256
    assert len(pass_bits(req["c"])) == {4: 1, 9: 1, 10: 2, 17: 2, 18: 3, 22: 3, 25: 3}[req["c"]]
    assert max(pass_bits(25)) == 8 and pass_bits(22) == [7, 7, 7]
    check(zk, ctx, scal, **req)


# ---- task geometry ---------------------------------------------------------------------------------------------------
def test_three_chunks_in_pass_0_the_last_ragged(zk, ctx):
    scal, req = case("chunks")
    assert -(-len(scal) // CH) == 3 and len(scal) % CH == 37
    check(zk, ctx, scal, **req)


@pytest.mark.parametrize("c", [10, 18])
def test_a_later_pass_segment_longer_than_one_task(zk, ctx, c):
    """more than 16384 scalars equal to 1 or r - 1: the segment of window 0 that holds bucket 0 is longer than one task in
    pass 1 (c = 18: and in pass 2), so the second task's (blockIdx.x - tpo[seg]) * CH matters; both signs in one bucket"""
    scal, req = case("hot_segment:%d" % c)
    got, want, plan = check(zk, ctx, scal, **req)
    bits = pass_bits(c)
    left = c - 1
    for b in bits[:-1]:                                 # the segment entering each later pass that starts at bucket 0
        left -= b
        seg = int(want["counts"][:1 << left].sum())
        assert CH < seg <= 2 * CH, seg
    assert want["counts"][0] > CH
    payloads = np.frombuffer(got["sorted"], dtype=np.uint32)[:int(want["counts"][0])]
    assert 0 < np.count_nonzero(payloads >> 31) < len(payloads)


# ---- hot keys for lds_count_rank ---------------------------------------------------------------------------------------
def test_all_scalars_equal(zk, ctx):
    """one bucket per window holds all n: every ballot of lds_count_rank is one key"""
    n, c, k0 = 5000, 12, 32
    rng = random.Random(5)
    s = next(s for s in iter(lambda: rng.randrange(R), None) if all(m for m, _ in ref.recode(s, c)[0]))
    got, want, plan = check(zk, ctx, (s,) * n, c=c, k0=k0)
    assert got["max_count"] == n and got["total_entries"] == n * plan["W"]
    hist = np.frombuffer(got["len_hist"], dtype=np.uint32)
    assert hist[k0] == plan["W"] * (n // k0) and hist[n % k0] == plan["W"] and hist.sum() == got["total1"]
    assert got["total1"] == plan["W"] * -(-n // k0)


def test_two_scalars_alternating_lane_by_lane(zk, ctx):
    rng = random.Random(6)
    a, b = rng.randrange(R), rng.randrange(R)
    got, want, plan = check(zk, ctx, (a, b) * 2500 + (a,), c=11)
    assert got["max_count"] >= 2500


def test_all_zero_scalars(zk, ctx):
    """no entry and no piece: the ordering kernel is not launched"""
    got, want, plan = check(zk, ctx, (0,) * 3000, c=9)
    assert (got["total_entries"], got["max_count"], got["total1"]) == (0, 0, 0)
    assert got["sorted"] == b"" and got["order"] == b"" and not any(got["counts"])


# ---- small n and piece lengths -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 2049])
def test_small_n_and_piece_lengths(zk, ctx, n):
    scal = witness_like(random.Random(n), n, 0.7, 0.2)
    for k0, for_g2 in ((8, False), (512, False), (0, False), (0, True)):
        got, want, plan = check(zk, ctx, scal, k0=k0, for_g2=for_g2)
        assert plan["K0"] == k0 or k0 == 0
    if n == 0:
        assert got["total1"] == 0 and got["sorted"] == b""


def test_forced_piece_lengths_cut_a_hot_bucket(zk, ctx):
    """2049 scalars of which most are 1: with k0 = 8 the hot bucket is hundreds of pieces, with 512 a handful"""
    scal = witness_like(random.Random(77), 2049, 0.9, 0.05)
    few = check(zk, ctx, scal, c=8, k0=512)[0]
    many = check(zk, ctx, scal, c=8, k0=8)[0]
    assert few["max_count"] == many["max_count"] > 512
    assert many["total1"] > few["total1"] + 64


# ---- digit edges planted among random scalars ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", [4, 13, 22])
def test_digit_edges_among_random_scalars(zk, ctx, c):
    scal, req = case("edges:%d" % c)
    assert {0, R - 1, HALF, HALF + 1, (1 << (3 * c)) - 1} <= set(scal)
    check(zk, ctx, scal, **req)


# ---- sparse form: the compact entry list ---------------------------------------------------------------------------------
SPARSE_C = 17


def workgroup_entries(want, n):
    """entries each workgroup of msm_entries_kernel emits, from the reference's payloads (merged: w * n + i)"""
    idx = (want["keys"] & np.uint64(0x7fffffff)).astype(np.int64) % n
    return np.bincount(idx // WG_SCALARS, minlength=-(-n // WG_SCALARS))


@functools.lru_cache(maxsize=None)
def sparse_case(kind):
    rng = random.Random("sparse-" + kind)
    light = lambda n: witness_like(rng, n, 0.7, 0.25)
    density = ref.density(light(5000))                 # of a witness: what the plan is made with, whatever the scalars
    if kind == "staged":
        return light(5000), density
    if kind == "unstaged":
        return uniform(rng, 5000), density
    return uniform(rng, WG_SCALARS) + light(2 * WG_SCALARS + 100), density     # the first workgroup overflows its stage


@pytest.mark.parametrize("kind", ["staged", "unstaged", "mixed"])
def test_sparse_form_staged_and_unstaged(zk, ctx, kind):
    scal, density = sparse_case(kind)
    got, want, plan = check(zk, ctx, scal, c=SPARSE_C, merged=True, density=density)
    assert plan["sparse"] == 1
    per_wg = workgroup_entries(want, len(scal))
    assert per_wg.sum() == got["total_entries"]
    if kind == "staged":
        assert (per_wg <= WG_STAGE).all() and per_wg.min() > 0
    elif kind == "unstaged":
        assert (per_wg > WG_STAGE).all()
    else:
        assert (per_wg > WG_STAGE).any() and (per_wg <= WG_STAGE).any()


def test_dense_and_sparse_form_hand_on_the_same(zk, ctx):
    """the entry form is a choice of the plan, not of the result: without the density the same scalars go through the dense
    digit array (checked against the same reference)"""
    scal, density = sparse_case("staged")
    _, _, plan = check(zk, ctx, scal, c=SPARSE_C, merged=True)
    assert plan["sparse"] == 0


# ---- lanes and reuse -----------------------------------------------------------------------------------------------------
def test_lanes_and_reuse(zk, ctx):
    """lane 0, lane 3, then twice in a row on one lane (the scans' generation counter, the one memset of the arena head);
    an ordinary MSM on the context afterwards: the hook leaves the lanes usable"""
    scal, req = case("classic:10")
    other, other_req = case("classic:9")
    for lane in (0, 3, 3, 3):
        check(zk, ctx, scal, lane=lane, **req)
    check(zk, ctx, other, lane=3, **other_req)
    check(zk, ctx, scal, lane=3, **req)
    rng = random.Random(9)
    n = 700
    bases = co.fixed_base_g1(b"".join(le(rng.randrange(R)) for _ in range(n)), 8)
    sc = b"".join(le(s) for s in witness_like(rng, n))
    assert ctx.msm_g1(bases, sc, n) == co.msm_g1(bases, sc, n, 8)


def test_a_short_buffer_is_an_error_and_nothing_is_written(zk, ctx):
    scal, req = case("classic:9")
    n = len(scal)
    plan = dict(zip(PLAN_WORDS, plan_words(zk, n, req["c"], False, False, None, 0)))
    full = [plan["TB"], plan["TB"] + 1, plan["TB"] + 1, n * plan["W"], n * plan["W"], n * plan["W"], plan["K0"] + 1]
    good = ctx.test_msm_sort(b"".join(le(s) for s in scal), n, req["c"])
    exact = [plan["TB"], plan["TB"] + 1, plan["TB"] + 1, good["total_entries"], good["total1"], good["total1"], plan["K0"] + 1]
    tight = ctx.test_msm_sort(b"".join(le(s) for s in scal), n, req["c"], caps=exact)      # exactly enough room is enough
    free = ("sorted", "order")                              # (atomics place the entries of a bucket, the pieces of a length)
    assert {k: v for k, v in tight.items() if k not in free} == {k: v for k, v in good.items() if k not in free}
    assert all(len(tight[k]) == len(good[k]) for k in free)
    for short in range(7):
        caps = list(exact)
        caps[short] -= 1
        bufs = [(ctypes.c_uint32 * k)() for k in full]
        for b in bufs:
            ctypes.memset(b, 0xA5, ctypes.sizeof(b))
        out = (ctypes.c_void_p * 7)(*[ctypes.addressof(b) for b in bufs])
        words, totals = (ctypes.c_uint64 * 13)(), (ctypes.c_uint32 * 3)()
        data = b"".join(le(s) for s in scal)
        rc = zk.lib().zkpoa_test_msm_sort(ctx._h, 0, data, n, req["c"], 0, 0, None, 0, words, totals, out,
                                          (ctypes.c_uint64 * 7)(*caps))
        assert rc == zk.PROVER_ERROR_SHORT_BUFFER
        assert all(np.all(np.frombuffer(b, dtype=np.uint32) == 0xA5A5A5A5) for b in bufs)
    with pytest.raises(zk.ZkpoaError):
        ctx.test_msm_sort(b"", 0, 40)                      # a width out of range is an error of its own


# ---- three-launch scans ----------------------------------------------------------------------------------------------------
_SCAN3_CHILD = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import __graft_entry__ as entry
import test_gpu_msm_sort as t
zk = entry.load_package()
ctx = zk.Context(0)
for name in sys.argv[2:]:
    scal, req = t.case(name)
    got, want, plan = t.check(zk, ctx, scal, **req)
    print(name, got["total_entries"], got["max_count"], got["total1"])
ctx.close()
"""


def test_three_launch_scans(zk, ctx):
    """ZKPOA_SCAN=3 is read once per process: a fresh child, under a time limit of its own, runs the checker on two of
    the cases above -- three-launch scans, the piece-length histogram from msm_piece_hist_kernel. Its arrays equal the
    reference, and so the default path's."""
    names = ["hot_segment:10", "edges:13"]
    rc = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-s", "-c", _SCAN3_CHILD, ROOT] + names,
                        env=dict(os.environ, ZKPOA_SCAN="3"), capture_output=True, text=True)
    assert rc.returncode == 0, rc.stdout + rc.stderr
    lines = [l.split() for l in rc.stdout.splitlines() if l.split()[:1] and l.split()[0] in names]
    assert [l[0] for l in lines] == names
    for name, *totals in lines:
        scal, req = case(name)
        got = check(zk, ctx, scal, **req)[0]
        assert [int(v) for v in totals] == [got["total_entries"], got["max_count"], got["total1"]]


# ---- density ----------------------------------------------------------------------------------------------------------------
DENSITY_SET = [0, 1, R - 1, HALF, HALF + 1, (1 << 32) - 1, 1 << 32, 1 << 64, (1 << 253) - 1]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 5000])
def test_density_equals_the_reference_bit_for_bit(ctx, n):
    """both sides are an exact integer divided by n in double precision; n = 0 gives the uniform default"""
    rng = random.Random(1000 + n)
    scal = [rng.choice(DENSITY_SET) if rng.random() < 0.6 else rng.randrange(R) for _ in range(n)]
    if n >= 63:
        scal[:len(DENSITY_SET)] = DENSITY_SET
    got = ctx.test_msm_density(b"".join(le(s) for s in scal), n)
    want = ref.density(scal)
    assert got == want, [(c, g, w) for c, (g, w) in enumerate(zip(got, want)) if g != w]
    if n == 0:
        assert got == [float(-(-254 // max(c, 4))) for c in range(32)]


def test_density_of_one_scalar_of_each_kind(ctx):
    for s in DENSITY_SET:
        assert ctx.test_msm_density(le(s), 1) == ref.density([s]), s
