"""The owned leaves at the prover's scale (include/zkpoa_merkle_paths.h): the lookup through the stable index
(zkpoa_anon_set_find_device, zkpoa_merkle_find), the batched path gather (zkpoa_merkle_paths, zkpoa_merkle_paths_device)
and the `merkle-tree` executable that uses them, with --any-order. Expected values come from the C oracle's level array
(co.merkle_levels) and plain numpy or Python -- a dict over the rows for the finds, a gather from the oracle's array for
the paths, text formatted here for the files -- never from the code under test."""
import functools
import json
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, le
from oracle import c_oracle as co
from oracle.py import poseidon as P
from test_poseidon_oracle import REF_ROOT, anon_set, ref_path_fixture

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
TOP = (1 << 256) - 1


# ---- shared, computed once ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_tree(n, seed=None):
    """(address bytes, balance bytes, k, the oracle's level array) of n random 160-bit addresses and 90-bit balances"""
    rng = random.Random(n if seed is None else seed)
    addr = b"".join(le(rng.randrange(1 << 160)) for _ in range(n))
    bal = b"".join(le(rng.randrange(1 << 90)) for _ in range(n))
    k = max(0, (n - 1).bit_length())
    return addr, bal, k, co.merkle_levels(addr, bal, k, 8)


def gather(levels, k, idx):
    """(path bytes, index-bit bytes) of the leaves idx, gathered from the oracle's level array with numpy"""
    nodes = np.frombuffer(levels, dtype=np.uint8).reshape(-1, 32)
    assert len(nodes) == (2 << k) - 1
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    sizes = [1 << (k - l) for l in range(k)]
    offs = np.array([sum(sizes[:l]) for l in range(k)], dtype=np.int64)           # where level l starts
    lv = np.arange(k, dtype=np.int64)
    at = idx[:, None] >> lv[None, :]
    return nodes[(offs[None, :] + (at ^ 1)).reshape(-1)].tobytes(), (at & 1).astype(np.uint8).tobytes()


# ---- 1. find on crafted keys -------------------------------------------------------------------------------------------
def device_find(ctx, keys, queries, index=True):
    """(first, count) as Python lists, through torch device buffers; a guard word behind each output must survive"""
    import torch
    n, m = len(keys), len(queries)
    raw = lambda ks: torch.from_numpy(np.frombuffer(b"".join(k.to_bytes(32, "little") for k in ks) + bytes(32),
                                                    dtype=np.uint8).copy()).cuda()
    d_keys, d_q = raw(keys), raw(queries)
    d_perm = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
    d_first = torch.full((m + 1,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    d_count = torch.full((m + 1,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if index:
        ctx.anon_set_index(d_keys.data_ptr(), n, d_perm.data_ptr())
    ctx.anon_set_find(d_keys.data_ptr() if n else 0, n, d_perm.data_ptr() if n else 0, d_q.data_ptr(), m,
                      d_first.data_ptr(), d_count.data_ptr())
    first = [int(v) & 0xffffffff for v in d_first.cpu().numpy()]
    count = [int(v) & 0xffffffff for v in d_count.cpu().numpy()]
    assert first[m] == 0x5a5a5a5a and count[m] == 0x5a5a5a5a
    return first[:m], count[:m]


def model_find(keys, queries):
    rows = {}
    for i, k in enumerate(keys):
        f, c = rows.get(k, (i, 0))
        rows[k] = (f, c + 1)
    return [rows.get(q, (NONE, 0))[0] for q in queries], [rows.get(q, (NONE, 0))[1] for q in queries]


def crafted(rng, extremes):
    """n = 4099 keys in shuffled rows, and what was put in: a run of 5 equal keys, pairs that differ only in byte 0 and
    only in byte 31, and (extremes) a key of all 0xff and one of all zero"""
    base = rng.getrandbits(256)
    run = rng.getrandbits(256)
    low = [(base, base ^ 0x01), (base ^ 0x4000, base ^ 0x4055)]                       # byte 0 only
    high = [(base ^ 0x100, base ^ 0x100 ^ (0x01 << 248)), (base ^ 0x200, base ^ 0x200 ^ (0x7f << 248))]   # byte 31 only
    special = [run] * 5 + [k for pair in low + high for k in pair] + ([TOP, 0] if extremes else [])
    keys = special + [rng.getrandbits(256) for _ in range(4099 - len(special))]
    rng.shuffle(keys)
    return keys, run, low, high


def test_find_on_crafted_keys(ctx):
    rng = random.Random(4099)
    keys, run, low, high = crafted(rng, extremes=True)
    assert len(keys) == 4099
    present = rng.sample([k for k in keys if 0 < k < TOP], 500)
    near = [k for pair in low + high for k in pair]
    queries = (present + [run] * 5 + near + [0, TOP, 1, TOP - 1] +
               [k ^ 0x02 for k in near] + [k ^ (0x02 << 248) for k in near] +          # neighbours: lowest and highest byte
               [present[0] + 1, present[0] - 1, present[1] ^ (1 << 255)])
    queries += [rng.getrandbits(256) for _ in range(777 - len(queries))]                # absent random keys
    assert len(queries) == 777
    want = model_find(keys, queries)
    assert want[1].count(0) > 200 and 5 in want[1]
    assert device_find(ctx, keys, queries) == want
    assert ctx.last_ms(10) > 0
    # one below the minimum and one above the maximum, in a set that leaves room for them
    keys, run, low, high = crafted(rng, extremes=False)
    lo, hi = min(keys), max(keys)
    assert 0 < lo and hi < TOP
    queries = [lo - 1, hi + 1, lo, hi, lo + 1, hi - 1, 0, TOP, run]
    assert device_find(ctx, keys, queries) == model_find(keys, queries)


def test_find_at_the_small_ends(ctx):
    a, b = 0x1234 << 200, 77
    assert device_find(ctx, [a], [a, b, a + 1, a - 1, 0]) == ([0, NONE, NONE, NONE, NONE], [1, 0, 0, 0, 0])
    assert device_find(ctx, [a, a], [a, b]) == ([0, NONE], [2, 0])
    assert device_find(ctx, [b, a], [a, b]) == ([1, 0], [1, 1])
    assert device_find(ctx, [a, b, a], []) == ([], [])                                  # m = 0: a no-op
    assert ctx.last_ms(10) == 0
    assert device_find(ctx, [], [a, 0, TOP], index=False) == ([NONE] * 3, [0] * 3)      # n = 0: every count is 0


# ---- 2. find on a tree -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 1000])
def test_tree_find(ctx, n):
    addr, bal, k, levels = oracle_tree(n)
    leaves = [levels[32 * i:32 * i + 32] for i in range(n)]
    assert len({bytes(h) for h in leaves}) == n and bytes(32) not in leaves           # pairwise distinct: count = 1
    rng = random.Random(n + 1)
    order = list(range(n))
    rng.shuffle(order)
    strangers = co.poseidon2(b"".join(le(rng.randrange(1 << 160)) for _ in range(9)), b"".join(le(rng.randrange(1 << 90)) for _ in range(9)), 2)
    queries = b"".join(leaves[i] for i in order) + bytes(32) + strangers
    tree = ctx.merkle_build(addr, bal)
    try:
        first, count = tree.find(queries)
        assert first.dtype == np.uint32 and count.dtype == np.uint32
        assert list(first) == order + [NONE] * 10                                       # the zero hash: padding is not searched
        assert list(count) == [1] * n + [0] * 10
        ms_first = ctx.last_ms(10)
        again = tree.find(queries)
        print("n = %d: first find %.3f ms of kernels (with the index), second %.3f ms" % (n, ms_first, ctx.last_ms(10)))
        assert list(again[0]) == list(first) and list(again[1]) == list(count)
        assert [list(x) for x in tree.find(b"")] == [[], []]
    finally:
        tree.close()


def test_tree_find_of_a_row_that_is_there_three_times(ctx):
    addr, bal, _, _ = oracle_tree(50)
    rows = [(addr[32 * i:32 * i + 32], bal[32 * i:32 * i + 32]) for i in range(50)]
    rows[20] = rows[33] = rows[7]
    a, b = b"".join(r[0] for r in rows), b"".join(r[1] for r in rows)
    hashes = co.poseidon2(a, b, 2)
    tree = ctx.merkle_build(a, b)
    try:
        first, count = tree.find(hashes[32 * 33:32 * 34] + hashes[32 * 8:32 * 9] + hashes[32 * 7:32 * 8])
        assert list(first) == [7, 8, 7] and list(count) == [3, 1, 3]
    finally:
        tree.close()


# ---- 3. paths against the oracle's array -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 17, 4097])
def test_paths_vs_the_oracles_array(ctx, n):
    import torch
    addr, bal, k, levels = oracle_tree(n)
    tree = ctx.merkle_build(addr, bal)
    try:
        assert tree.info()[1] == k
        every = list(range(1 << k))                                                    # padding leaves included
        for idx in (every, every[::-1], [i for i in every for _ in (0, 1)]):
            assert tree.paths(idx) == gather(levels, k, idx)
        assert tree.paths([]) == (b"", b"")
        if n == 4097:                                                                  # one round boundary, 27 MB out
            idx = np.random.default_rng(3).integers(0, 1 << k, size=(1 << 16) + 3)
            got = tree.paths(idx)
            assert ctx.last_ms(10) > 0
            assert got == gather(levels, k, idx)
        with pytest.raises(Exception, match="out of range"):
            tree.paths([0, 1 << k])
        assert tree.paths([(1 << k) - 1, 0]) == gather(levels, k, [(1 << k) - 1, 0])    # the context still works
        if k:
            # the kernel alone: an index that is not below 2^k gives zeros, the others are right, nothing behind the output
            idx = [0, (1 << k) - 1, 1 << k, 1, (1 << 40) + 1, n - 1, (1 << 64) - 1, 1 << 63]
            valid = [i if i < (1 << k) else 0 for i in idx]
            want = bytearray(gather(levels, k, valid)[0])
            for j, i in enumerate(idx):
                if i >= (1 << k):
                    want[32 * k * j:32 * k * (j + 1)] = bytes(32 * k)
            d_idx = torch.from_numpy(np.array(idx, dtype=np.uint64).view(np.int64)).cuda()
            d_out = torch.full((32 * k * len(idx) + 64,), 0xa5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            tree.paths_device(d_idx.data_ptr(), len(idx), d_out.data_ptr())
            got = d_out.cpu().numpy().tobytes()
            assert got[:32 * k * len(idx)] == bytes(want)
            assert got[32 * k * len(idx):] == b"\xa5" * 64
    finally:
        tree.close()


# ---- 4. against the single-leaf entry point ----------------------------------------------------------------------------
def test_paths_are_the_single_paths_back_to_back(ctx):
    addr, bal = anon_set()
    tree = ctx.merkle_build(b"".join(le(a) for a in addr), b"".join(le(b) for b in bal))
    try:
        elems, bits = tree.paths(range(16))
        single = [tree.path(i) for i in range(16)]
        assert elems == b"".join(le(e) for es, _ in single for e in es)
        assert bits == bytes(b for _, bs in single for b in bs)
        leaf_addr, leaf_bal, root, ref_elems, ref_bits = ref_path_fixture()
        i = addr.index(leaf_addr)
        assert i == 3
        assert [int.from_bytes(elems[32 * (4 * i + l):32 * (4 * i + l + 1)], "little") for l in range(4)] == ref_elems
        assert list(bits[4 * i:4 * i + 4]) == ref_bits
        node = P.poseidon([leaf_addr, leaf_bal])
        for e, b in zip(ref_elems, ref_bits):
            node = P.poseidon([e, node] if b else [node, e])
        assert node == root == REF_ROOT
    finally:
        tree.close()


# ---- 5. the executable -------------------------------------------------------------------------------------------------
def poa_text(rows):
    return json.dumps({"accountAttestations": [{"accountData": {"address": {"__bigint__": str(a)}, "balance": {"__bigint__": str(b)}}}
                                               for a, b in rows]})


def expected_files(addr, bal, owned_rows, k, levels):
    """(merkle_root.json, the object of merkle_proofs.json) for the owned rows, from the oracle's level array"""
    rd = lambda node: int.from_bytes(levels[32 * node:32 * node + 32], "little")
    elems, bits = gather(levels, k, owned_rows)
    ints = [int.from_bytes(elems[32 * j:32 * j + 32], "little") for j in range(len(elems) // 32)]
    obj = {"leaves": [{"address": {"__bigint__": str(addr[i])}, "balance": {"__bigint__": str(bal[i])},
                       "hash": {"__bigint__": str(rd(i))}} for i in owned_rows],
           "path_elements": [[{"__bigint__": str(e)} for e in ints[k * j:k * (j + 1)]] for j in range(len(owned_rows))],
           "path_indices": [list(bits[k * j:k * (j + 1)]) for j in range(len(owned_rows))]}
    return '{\n  "__bigint__": "%d"\n}' % rd((2 << k) - 2), obj


def run_cli(zk, tmp_path, name, csv_path, rows, *options):
    (tmp_path / (name + ".json")).write_text(poa_text(rows))
    out = tmp_path / name
    out.mkdir()
    rc = subprocess.run([zk.MERKLE_BIN, "--anon-set", str(csv_path), "--poa-input-data", str(tmp_path / (name + ".json")),
                         "--output-dir", str(out)] + list(options), capture_output=True, text=True, timeout=120)
    return rc, out


def write_set(path, addr, bal):
    path.write_text("address,eth_balance\n" + "".join("0x%040x,%d\n" % (a, b) for a, b in zip(addr, bal)))


def test_cli_reference_set_byte_for_byte_and_any_order(zk, tmp_path):
    addr, bal = anon_set()
    csv_path = os.path.join(GOLDEN, "ref", "merkle", "anonymity_set_10.csv")
    levels = co.merkle_levels(b"".join(le(a) for a in addr), b"".join(le(b) for b in bal), 4, 2)
    owned = [1, 3, 9]
    root_text, obj = expected_files(addr, bal, owned, 4, levels)
    assert root_text == '{\n  "__bigint__": "%d"\n}' % REF_ROOT
    # (a) in the set's order
    rc, out = run_cli(zk, tmp_path, "plain", csv_path, [(addr[i], bal[i]) for i in owned])
    assert rc.returncode == 0, rc.stderr
    assert "Done creating Merkle tree of height 5" in rc.stdout and "Root hash %d written to file" % REF_ROOT in rc.stdout
    assert (out / "merkle_root.json").read_text() == root_text
    assert (out / "merkle_proofs.json").read_text() == json.dumps(obj, indent=2)
    plain_stdout = rc.stdout
    # (b) reversed: the forward scan's refusal by default, every entry's own path under --any-order
    back = owned[::-1]
    rc, out = run_cli(zk, tmp_path, "reversed", csv_path, [(addr[i], bal[i]) for i in back])
    assert rc.returncode != 0
    assert rc.stderr == "Error: Owned leaf %d at index 1 does not exist in the anonymity set\n" % addr[3]
    assert not (out / "merkle_proofs.json").exists()
    rc, out = run_cli(zk, tmp_path, "any", csv_path, [(addr[i], bal[i]) for i in back], "--any-order")
    assert rc.returncode == 0, rc.stderr
    assert rc.stdout.replace(str(out), "DIR") == plain_stdout.replace(str(tmp_path / "plain"), "DIR")
    assert (out / "merkle_root.json").read_text() == root_text
    assert (out / "merkle_proofs.json").read_text() == json.dumps(expected_files(addr, bal, back, 4, levels)[1], indent=2)
    # an address that is in no row: the same message under --any-order
    rc, out = run_cli(zk, tmp_path, "absent", csv_path, [(addr[9], bal[9]), (addr[2], bal[2] + 1)], "--any-order")
    assert rc.returncode != 0
    assert rc.stderr == "Error: Owned leaf %d at index 1 does not exist in the anonymity set\n" % addr[2]
    assert not (out / "merkle_proofs.json").exists() and os.listdir(out) == ["merkle_root.json"]


def test_cli_more_than_one_round_of_owned_entries(zk, tmp_path):
    """2^16 + 5 owned entries, in non-decreasing set order with repeats, over a 40-row set: the writer's round boundary,
    and the indexed route (every leaf is there once). The whole file, byte for byte, against text formatted here."""
    addr_b, bal_b, k, levels = oracle_tree(40)
    assert k == 6
    addr = [int.from_bytes(addr_b[32 * i:32 * i + 32], "little") for i in range(40)]
    bal = [int.from_bytes(bal_b[32 * i:32 * i + 32], "little") for i in range(40)]
    assert len({levels[32 * i:32 * i + 32] for i in range(40)}) == 40                  # all distinct: the indexed route applies
    m = (1 << 16) + 5
    rng = random.Random(5)
    owned = sorted(rng.randrange(40) for _ in range(m))
    assert len(set(owned)) == 40
    # one entry of each array per row, formatted as a 2-space pretty printer does; checked against json.dumps on a sample
    _, rows_obj = expected_files(addr, bal, list(range(40)), k, levels)
    leaf = ['    {\n      "address": {\n        "__bigint__": "%s"\n      },\n      "balance": {\n        "__bigint__": "%s"\n      },\n'
            '      "hash": {\n        "__bigint__": "%s"\n      }\n    }' % (l["address"]["__bigint__"], l["balance"]["__bigint__"], l["hash"]["__bigint__"])
            for l in rows_obj["leaves"]]
    elems = ["    [\n" + ",\n".join('      {\n        "__bigint__": "%s"\n      }' % e["__bigint__"] for e in es) + "\n    ]"
             for es in rows_obj["path_elements"]]
    bits = ["    [\n" + ",\n".join("      %d" % b for b in bs) + "\n    ]" for bs in rows_obj["path_indices"]]
    text = lambda rows: ('{\n  "leaves": [\n' + ",\n".join(leaf[i] for i in rows) + '\n  ],\n  "path_elements": [\n' +
                         ",\n".join(elems[i] for i in rows) + '\n  ],\n  "path_indices": [\n' + ",\n".join(bits[i] for i in rows) + "\n  ]\n}")
    sample = [0, 0, 17, 39]
    assert text(sample) == json.dumps(expected_files(addr, bal, sample, k, levels)[1], indent=2)
    write_set(tmp_path / "set.csv", addr, bal)
    rc, out = run_cli(zk, tmp_path, "many", tmp_path / "set.csv", [(addr[i], bal[i]) for i in owned])
    assert rc.returncode == 0, rc.stderr
    got = (out / "merkle_proofs.json").read_text()
    want = text(owned)
    print("merkle_proofs.json of %d entries: %.1f MB" % (m, len(want) / 1e6))
    assert len(got) == len(want) and got == want
    assert sorted(os.listdir(out)) == ["merkle_proofs.json", "merkle_root.json"]        # no temporary file left


def test_cli_duplicate_rows_and_the_small_ends(zk, tmp_path):
    # (d) one (address, balance) row twice in the set: the forward scan's answer, the first of the two rows
    addr_b, bal_b, _, _ = oracle_tree(11)
    addr = [int.from_bytes(addr_b[32 * i:32 * i + 32], "little") for i in range(11)]
    bal = [int.from_bytes(bal_b[32 * i:32 * i + 32], "little") for i in range(11)]
    addr[8], bal[8] = addr[2], bal[2]
    levels = co.merkle_levels(b"".join(le(a) for a in addr), b"".join(le(b) for b in bal), 4, 2)
    write_set(tmp_path / "twice.csv", addr, bal)
    for name, options in (("scan", []), ("lowest", ["--any-order"])):
        rc, out = run_cli(zk, tmp_path, name, tmp_path / "twice.csv", [(addr[0], bal[0]), (addr[8], bal[8]), (addr[10], bal[10])], *options)
        assert rc.returncode == 0, rc.stderr
        root_text, obj = expected_files(addr, bal, [0, 2, 10], 4, levels)
        assert (out / "merkle_root.json").read_text() == root_text
        assert (out / "merkle_proofs.json").read_text() == json.dumps(obj, indent=2)
    # (e) no owned entry at all; a one-row set (no path elements)
    rc, out = run_cli(zk, tmp_path, "none", tmp_path / "twice.csv", [])
    assert rc.returncode == 0, rc.stderr
    assert (out / "merkle_proofs.json").read_text() == '{\n  "leaves": [],\n  "path_elements": [],\n  "path_indices": []\n}'
    write_set(tmp_path / "one.csv", addr[:1], bal[:1])
    one = co.merkle_levels(le(addr[0]), le(bal[0]), 0, 1)
    for name, options in (("one", []), ("one_any", ["--any-order"])):
        rc, out = run_cli(zk, tmp_path, name, tmp_path / "one.csv", [(addr[0], bal[0])] * 2, *options)
        assert rc.returncode == 0, rc.stderr
        root_text, obj = expected_files(addr, bal, [0, 0], 0, one)
        assert obj["path_elements"] == [[], []] and obj["path_indices"] == [[], []]
        assert (out / "merkle_root.json").read_text() == root_text
        assert (out / "merkle_proofs.json").read_text() == json.dumps(obj, indent=2)
