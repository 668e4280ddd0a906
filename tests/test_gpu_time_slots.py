"""What each slot of zkpoa_last_ms holds after the call that fills it (include/zkpoa_prover.h, "measurement"; the slots
are csrc/zkpoa_internal.hpp's MsSlot), at the smallest shapes that run the code: a slot is set by the kernels of its
call, zero after a call that had nothing to launch, and added to where a call launches in rounds. Only the rules are
pinned here, never a duration; the results of the same calls are checked where the calls are tested."""
import json
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN, golden_case, le
from oracle import c_oracle as co
from oracle.py import groth16 as g16

pytestmark = pytest.mark.gpu
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def _rows(rng, n, bits):
    return b"".join(le(rng.randrange(1 << bits)) for _ in range(n))


def test_ntt_slot(ctx):
    rng = random.Random(2)
    ctx.ntt(b"".join(le(rng.randrange(R)) for _ in range(1 << 4)), 4)
    assert ctx.last_ms(2) > 0


def test_merkle_build_slot(ctx):
    rng = random.Random(7)
    tree = ctx.merkle_build(_rows(rng, 3, 160), _rows(rng, 3, 90))
    try:
        assert ctx.last_ms(7) > 0
    finally:
        tree.close()


def test_lane_batch_slot(ctx):
    (entry,) = json.load(open(os.path.join(GOLDEN, "sigs", "signatures_1.json")))
    sig = entry["signature"]
    be = lambda h: int(h, 16).to_bytes(32, "big")
    out = ctx.ecdsa_star(be(sig["r"]), be(sig["s"]), be(sig["msghash"]), bytes([sig["v"]]), bytes.fromhex(entry["address"][2:]))
    assert out[3] == b"\0"
    assert ctx.last_ms(8) > 0
    assert ctx.ecdsa_star(b"", b"", b"", b"", b"") == (b"", b"", b"", b"")          # n = 0: nothing launched
    assert ctx.last_ms(8) == 0


def test_anon_index_slot(ctx):
    ctx.anon_set_audit(_rows(random.Random(9), 3, 160))
    assert ctx.last_ms(9) > 0
    ctx.anon_set_index(0, 0, 0)
    assert ctx.last_ms(9) == 0


def test_find_and_paths_slot(ctx):
    rng = random.Random(10)
    tree = ctx.merkle_build(_rows(rng, 5, 160), _rows(rng, 5, 90))
    try:
        hashes = tree.leaves(1, 2)
        first, count = tree.find(hashes)                  # the first find over a tree builds the index of its leaves as well
        assert list(first) == [1, 2] and list(count) == [1, 1]
        ms_first = ctx.last_ms(10)
        tree.find(hashes)
        ms_second = ctx.last_ms(10)
        print("find on 5 leaves: first %.4f ms of kernels (with the index), second %.4f ms" % (ms_first, ms_second))
        assert ms_first > 0
        assert 0 < ms_second <= ms_first
        assert tree.paths([]) == (b"", b"")
        assert ctx.last_ms(10) == 0
        idx = np.arange((1 << 16) + 1, dtype=np.uint64) % 8                          # two rounds: the second adds to the first
        elems, bits = tree.paths(idx)
        assert ctx.last_ms(10) > 0
        assert elems[-96:] == elems[:96] and len(elems) == 96 * len(idx)             # index 2^16 = 0 mod 8: the second round ran
    finally:
        tree.close()


def test_chain_slot(ctx):
    g = golden_case("n8")
    zkey = g16.read_zkey(g["circuit.zkey"])
    p4, l4 = g16.read_binfile(g["circuit.zkey"], "zkey", 2)[4][0]
    _, w = g16.read_wtns(g["witness.wtns"])
    got = ctx.h_scalars(g["circuit.zkey"][p4:p4 + l4], b"".join(le(x) for x in w), zkey.nVars, zkey.domainSize.bit_length() - 1)
    assert got == g["h_scalars.bin"]
    assert ctx.last_ms(3) > 0


def test_msm_slots(ctx):
    rng = random.Random(1)
    n = 1 << 10
    bases = co.fixed_base_g1(b"".join(le(rng.randrange(R)) for _ in range(n)), 4)
    ctx.msm_g1(bases, b"".join(le(rng.randrange(R)) for _ in range(n)), n)
    assert ctx.last_ms(0) > 0 and ctx.last_ms(1) > 0


def test_ids_out_of_range(ctx):
    assert ctx.last_ms(11) == -1.0 and ctx.last_ms(-1) == -1.0
