"""Merkle-Patricia proofs on the GPU (include/zkpoa_state_proof.h): zkpoa_mpt_verify, zkpoa_eth_account_proofs, the whole
check of a set against a proofs file and `zkpoa-audit --state-proofs`. Every expected status, `where`, value span,
nonce and balance is what tests/mpt_ref.py gives for the proofs of tests/mpt_cases.py; nothing expected comes from
the library. No mutation may make a call fail: a damaged proof is a status."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import mpt_cases as cases
import mpt_ref as m
from conftest import GOLDEN, le
from secp_ref import keccak256
from test_poseidon_oracle import anon_set

pytestmark = pytest.mark.gpu

CSV = os.path.join(GOLDEN, "ref", "merkle", "anonymity_set_10.csv")
VKEY = os.path.join(GOLDEN, "ref", "layer_three_vkey.json")
RUN_1 = os.path.join(GOLDEN, "ref", "1_sigs_1_batches_5_height__layer_three")


def verify(ctx, zk, g, key_kind=None):
    blob, offsets, lengths, first = m.layout(g["proofs"])
    kind = zk.MPT_KEY32 if key_kind is None else key_kind
    status, where, span = ctx.mpt_verify(b"".join(g["keys"]), g["root"], blob, offsets, lengths, first, key_kind=kind)
    return [(s, int(w), int(o), int(n)) for s, w, (o, n) in zip(status, where, span)]


def test_raw_keys_present_and_absent_of_every_kind(zk, ctx):
    kinds = set()
    for g in cases.raw_groups():
        want = cases.expected(g)
        assert verify(ctx, zk, g) == want, g["name"]
        assert ctx.last_ms(8) > 0
        assert {w[0] for w in want} == {m.PRESENT, m.ABSENT}
        kinds |= {cases.absent_kind(g, i) for i, w in enumerate(want) if w[0] == m.ABSENT}
    assert kinds == {"slot", "extension", "leaf"}
    sixteen = [g for g in cases.raw_groups() if g["name"].startswith("sixteen")][0]
    assert len(sixteen["proofs"][0][0]) == 532 and sixteen["proofs"][0][0][:3] == b"\xf9\x02\x11"      # a two-byte list length


def test_keccak_block_edges_in_one_launch(zk, ctx):
    g = cases.keccak_edges_group()                                               # asserts its own node sizes
    want = cases.expected(g)
    assert verify(ctx, zk, g) == want and all(w[0] == m.PRESENT for w in want)


def test_mutations_are_statuses(zk, ctx):
    seen = set()
    for g in cases.mutation_groups():
        want = cases.expected(g)
        assert verify(ctx, zk, g) == want, g["name"]
        seen |= {w[0] for w in want}
        if g["name"] == "trieanyorder":
            assert m.CHILD in {w[0] for w in want}
        if g["name"] == "crafted nodes":
            by_name = dict(zip(g["names"], want))
            assert by_name["a list of 3 items"][:2] == (m.RLP, 1) and by_name["a flag nibble of 4"][:2] == (m.HEX_PREFIX, 1)
            assert by_name["a non-zero pad nibble"][:2] == (m.HEX_PREFIX, 1) and by_name["a good leaf"][0] == m.PRESENT
            assert by_name["a list length that points past the node"][:2] == (m.RLP, 1)
    assert seen == {m.PRESENT, m.ABSENT, m.NO_NODES, m.HASH, m.RLP, m.CHILD, m.SHORT, m.LONG, m.HEX_PREFIX}


def test_lane_counts_and_slab_borders(zk, ctx):
    for n in (1, 63, 64, 65, 257):
        g = cases.lanes_group(n)
        assert verify(ctx, zk, g) == cases.expected(g), n
    g = cases.lanes_group(150)
    want = cases.expected(g)
    ctx.set_option("state_proof_slab", 64)                                       # 64 + 64 + 22: two borders
    try:
        assert verify(ctx, zk, g) == want
    finally:
        ctx.set_option("state_proof_slab", 0)
    assert verify(ctx, zk, g) == want
    with pytest.raises(zk.ZkpoaError):
        ctx.set_option("state_proof_slab", -1)


def test_layout_errors_launch_nothing(zk, ctx):
    g = cases.lanes_group(3)
    blob, offsets, lengths, first = m.layout(g["proofs"])
    assert verify(ctx, zk, g) == cases.expected(g) and ctx.last_ms(8) > 0
    L = zk.lib()

    def raw(offsets, lengths, first, nodes_bytes=len(blob)):
        off, ln, fi = np.array(offsets, dtype=np.uint64), np.array(lengths, dtype=np.uint32), np.array(first, dtype=np.uint64)
        status, where, span = np.full(3, 0xAA, dtype=np.uint8), np.full(3, 0xAAAAAAAA, dtype=np.uint32), np.full(6, 0xAA, dtype=np.uint64)
        ptr = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
        rc = L.zkpoa_mpt_verify(ctx._h, 3, b"".join(g["keys"]), 0, g["root"], blob, nodes_bytes, ptr(off, ctypes.c_uint64),
                                ptr(ln, ctypes.c_uint32), ptr(fi, ctypes.c_uint64), status.ctypes.data, ptr(where, ctypes.c_uint32),
                                ptr(span, ctypes.c_uint64))
        untouched = (status == 0xAA).all() and (where == 0xAAAAAAAA).all() and (span == 0xAA).all()
        return rc, L.zkpoa_last_error(ctx._h).decode(), untouched
    assert raw(offsets, lengths, first)[0] == zk.PROVER_OK
    swapped = [first[0], first[2], first[1], first[3]]
    for bad, text in ((raw(offsets, lengths, swapped), "first_node descends"),
                      (raw([offsets[0] + 4] + offsets[1:], lengths, first), "multiple of 8"),
                      (raw(offsets[:1] + [offsets[2], offsets[1]] + offsets[3:], lengths, first), "descends"),
                      (raw(offsets, lengths, first, len(blob) - 8), "end of the blob"),
                      (raw(offsets, lengths[:-1] + [lengths[-1] + 8], first), "end of the blob")):
        rc, message, untouched = bad
        assert rc == zk.PROVER_ERROR and text in message and untouched, (text, message)
        assert ctx.last_ms(8) == 0


def test_accounts(zk, ctx):
    g, want = cases.account_group()
    blob, offsets, lengths, first = m.layout(g["proofs"])
    status, where, nonce, balance, sroot, code = ctx.eth_account_proofs(b"".join(g["keys"]), g["root"], blob, offsets, lengths, first)
    got = [(status[i], int(nonce[i]), balance[32 * i:32 * i + 32].hex(), sroot[32 * i:32 * i + 32].hex(), code[32 * i:32 * i + 32].hex())
           for i in range(len(want))]
    assert got == want
    assert {w[1] for w in want} >= {0, (1 << 64) - 1} and {int(w[2], 16) for w in want} >= {0, 1, 1 << 64, (1 << 256) - 1}
    assert keccak256(b"contract code").hex() in {w[4] for w in want}
    # the optional outputs left out; and the generic form over the same proofs through ZKPOA_MPT_ADDRESS20
    again = ctx.eth_account_proofs(b"".join(g["keys"]), g["root"], blob, offsets, lengths, first, with_hashes=False)
    assert again[0] == status and again[3] == balance and again[4] is None
    generic = verify(ctx, zk, g, key_kind=zk.MPT_ADDRESS20)
    hashed = cases.expected(dict(g, keys=[keccak256(a) for a in g["keys"]]))
    assert generic == hashed


# ---- the whole check and the executable --------------------------------------------------------------------------------
def addresses20():
    return [a.to_bytes(32, "big")[12:] for a in anon_set()[0]]


@pytest.fixture(scope="module")
def world():
    """The ten-row set inside a trie with 200 other accounts, balances in wei -> (trie, others' addresses)"""
    rng = random.Random(200)
    others = [keccak256(b"other account %d" % i)[:20] for i in range(200)]
    accounts = {a: m.account(rng.randrange(50), rng.randrange(1 << 70)) for a in others}
    accounts.update({a: m.account(i, b) for i, (a, b) in enumerate(zip(addresses20(), anon_set()[1]))})
    return m.account_trie(accounts), others


def lines_for(trie, addresses, seed=1):
    lines = [m.proof_json(a, trie.prove(keccak256(a)), envelope=i % 2 == 1, balance=12345, ident=i) for i, a in enumerate(addresses)]
    random.Random(seed).shuffle(lines)
    return lines


def set_bytes(balances=None):
    addr, bal = anon_set()
    return b"".join(le(a) for a in addr), b"".join(le(b) for b in (balances or bal))


def test_whole_check_through_the_library(zk, ctx, world, tmp_path):
    trie, others = world
    own = addresses20()
    path = tmp_path / "proofs.jsonl"
    m.write_jsonl(path, lines_for(trie, own + others[:7]))
    a, b = set_bytes()
    rep = ctx.anon_set_state_check(a, b, path, trie.root)
    assert rep["ok"] and (rep["rows"], rep["proven_present"], rep["proven_absent"], rep["proofs_read"], rep["proofs_not_in_set"]) == (10, 10, 0, 17, 7)
    assert rep["kernel_ms"] > 0 and rep["first_bad_row"] is None and rep["first_diff_row"] is None
    # one csv balance off by one
    bal = list(anon_set()[1])
    bal[3] += 1
    rep = ctx.anon_set_state_check(a, set_bytes(bal)[1], path, trie.root)
    assert not rep["ok"] and (rep["rows_differ"], rep["first_bad_row"], rep["first_bad_kind"], rep["first_diff_row"]) == (1, 3, 3, 3)
    assert rep["first_diff_chain_balance"] == bal[3] - 1 and rep["proven_present"] == 9
    # a row whose proof is missing; every other row is still examined
    m.write_jsonl(path, lines_for(trie, own[:6] + own[7:]))
    rep = ctx.anon_set_state_check(a, b, path, trie.root)
    assert (rep["ok"], rep["rows_without_proof"], rep["first_bad_row"], rep["first_bad_kind"], rep["proven_present"]) == (False, 1, 6, 1, 9)
    # proofs under another root
    m.write_jsonl(path, lines_for(trie, own))
    rep = ctx.anon_set_state_check(a, b, path, keccak256(b"another root"))
    assert (rep["ok"], rep["rows_failed"], rep["first_bad_row"], rep["first_bad_kind"], rep["first_bad_status"], rep["first_bad_where"]) == \
        (False, 10, 0, 2, m.HASH, 0)
    # a damaged proof beside a good one for the same row: the good one counts
    good = m.proof_json(own[2], trie.prove(keccak256(own[2])))
    damaged = m.proof_json(own[2], trie.prove(keccak256(own[2]))[:-1])
    m.write_jsonl(path, [damaged] + lines_for(trie, own[:2] + own[3:]) + [good])
    assert ctx.anon_set_state_check(a, b, path, trie.root)["ok"]
    m.write_jsonl(path, [damaged] + lines_for(trie, own[:2] + own[3:]))
    rep = ctx.anon_set_state_check(a, b, path, trie.root)
    assert (rep["ok"], rep["rows_failed"], rep["first_bad_row"], rep["first_bad_status"]) == (False, 1, 2, m.SHORT)
    # an absent account: good with csv balance 0, bad with any other
    nobody = keccak256(b"nobody holds this")[:20]
    assert m.verify(trie.root, keccak256(nobody), trie.prove(keccak256(nobody)))[0] == m.ABSENT
    m.write_jsonl(path, lines_for(trie, own + [nobody]))
    a11 = a + le(int.from_bytes(nobody, "big"))
    rep = ctx.anon_set_state_check(a11, b + le(0), path, trie.root)
    assert rep["ok"] and (rep["proven_present"], rep["proven_absent"]) == (10, 1)
    rep = ctx.anon_set_state_check(a11, b + le(5), path, trie.root)
    assert (rep["ok"], rep["rows_differ"], rep["first_diff_row"], rep["first_diff_absent"], rep["first_diff_chain_balance"]) == (False, 1, 10, True, 0)
    # a malformed file is an error that names the line, not a finding
    m.write_jsonl(path, lines_for(trie, own)[:4] + ["{\"address\": 5}"])
    with pytest.raises(zk.ZkpoaError, match="line 5"):
        ctx.anon_set_state_check(a, b, path, trie.root)
    with pytest.raises(zk.ZkpoaError):
        ctx.anon_set_state_check(a, b, tmp_path / "missing.jsonl", trie.root)
    with pytest.raises(zk.ZkpoaError, match="unit_divisor"):
        ctx.anon_set_state_check(a, b, path, trie.root, unit_divisor=7)


def test_balance_units_floor(zk, ctx, tmp_path):
    own, bal = addresses20(), anon_set()[1]
    chain = [b * 10 ** 18 for b in bal]
    chain[0] = 414 * 10 ** 18 + 5
    chain[1] = 84 * 10 ** 18 - 1                                                 # floors to 83
    trie = m.account_trie({a: m.account(1, c) for a, c in zip(own, chain)})
    path = tmp_path / "proofs.jsonl"
    m.write_jsonl(path, lines_for(trie, own))
    a, b = set_bytes()
    assert bal[0] == 414 and bal[1] == 83
    assert ctx.anon_set_state_check(a, b, path, trie.root, unit_divisor=10 ** 18)["ok"]
    rep = ctx.anon_set_state_check(a, b, path, trie.root, unit_divisor=10 ** 9)
    assert not rep["ok"] and rep["rows_differ"] == 10 and rep["first_diff_chain_balance"] == chain[0]


def audit(zk, csv_path, extra):
    return subprocess.run([zk.AUDIT_BIN, "--anon-set", str(csv_path), "--vkey", VKEY, "--public", os.path.join(RUN_1, "public.json"),
                           "--proof", os.path.join(RUN_1, "proof.json"), *extra], capture_output=True, text=True, timeout=120)


def test_executable(zk, world, tmp_path):
    trie, others = world
    own = addresses20()
    path = tmp_path / "proofs.jsonl"
    m.write_jsonl(path, lines_for(trie, own + others[:7]))
    plain = audit(zk, CSV, [])
    assert plain.returncode == 1 and len(plain.stdout.splitlines()) == 6
    # all good, the root from a built header: the verdict names exactly what the run without the options names
    header = m.block_header(trie.root, 19000000)
    rc = audit(zk, CSV, ["--state-proofs", str(path), "--block-header", "0x" + header.hex()])
    lines = rc.stdout.splitlines()
    assert rc.returncode == 1 and lines[0] == "block: number 19000000, hash 0x" + keccak256(header).hex(), rc.stdout + rc.stderr
    assert lines[3].startswith("state: 10 proven present, 0 proven absent, 0 without a proof, 0 with failed proofs, 0 with another balance; "
                               "17 proofs read, 7 for addresses not in the set")
    assert lines[1:3] + lines[4:] == plain.stdout.splitlines() and lines[-1] == plain.stdout.splitlines()[-1] == "AUDIT FAILED: proof"
    (tmp_path / "header.hex").write_text("0x" + header.hex() + "\n")
    again = audit(zk, CSV, ["--state-proofs=" + str(path), "--block-header", "@" + str(tmp_path / "header.hex"), "--balance-unit", "wei"])
    assert again.stdout == rc.stdout and again.returncode == 1
    # one csv balance off by one: the row and both balances on the line
    rows = open(CSV).read().splitlines()
    rows[4] = rows[4].split(",")[0] + ",355"
    (tmp_path / "off.csv").write_text("\n".join(rows) + "\n")
    rc = audit(zk, tmp_path / "off.csv", ["--state-proofs", str(path), "--state-root", "0x" + trie.root.hex()])
    lines = rc.stdout.splitlines()
    assert rc.returncode == 1 and lines[-1] == "AUDIT FAILED: state root proof" and not lines[0].startswith("block:")
    assert "row 3" in lines[2] and "chain balance 354 wei" in lines[2] and "csv balance 355" in lines[2] and own[3].hex() in lines[2]
    # under another root
    rc = audit(zk, CSV, ["--state-proofs", str(path), "--state-root", "0x" + keccak256(b"another root").hex()])
    assert rc.returncode == 1 and rc.stdout.splitlines()[-1] == "AUDIT FAILED: state proof" and "a node's hash differs at node 0" in rc.stdout
    # incomplete sets of the options: exit 2, the usage text, nothing on stdout
    for extra in (["--state-proofs", str(path)], ["--state-root", "0x" + trie.root.hex()], ["--balance-unit", "ether"],
                  ["--state-proofs", str(path), "--state-root", "0x" + trie.root.hex(), "--block-header", "0x" + header.hex()]):
        rc = audit(zk, CSV, extra)
        assert rc.returncode == 2 and rc.stdout == "" and "Usage: zkpoa-audit" in rc.stderr, extra
    for extra in (["--state-root", "0x1234"], ["--block-header", "0x" + header.hex()[:-2]], ["--state-root", "0x" + trie.root.hex(), "--balance-unit", "szabo"]):
        rc = audit(zk, CSV, ["--state-proofs", str(path)] + extra)
        assert rc.returncode == 2 and rc.stdout == "" and rc.stderr.startswith("Error: "), extra
