"""tests/mpt_ref.py pinned on three public facts (no GPU): the empty-trie root, the ethereum/tests `trieanyorder` vector,
and the mainnet genesis header, whose fields are committed under tests/golden/eth/. The host-only entry point
zkpoa_eth_block_header is checked on the same header."""
import json
import os
import random

import pytest

import mpt_ref as m
from conftest import GOLDEN
from secp_ref import keccak256


def genesis():
    with open(os.path.join(GOLDEN, "eth", "mainnet_genesis_header.json")) as f:
        doc = json.load(f)
    fields = []
    for _, v in doc["fields"]:
        if v == "zero256":
            fields.append(bytes(256))
        elif v.startswith("quantity:"):
            fields.append(m._int(int(v[9:], 16)))
        else:
            fields.append(bytes.fromhex(v[2:]))
    return doc, fields


def test_rlp_and_hex_prefix():
    # the yellow paper's and the Ethereum wiki's examples
    assert m.rlp_encode(b"dog") == b"\x83dog" and m.rlp_encode([b"cat", b"dog"]) == b"\xc8\x83cat\x83dog"
    assert m.rlp_encode(b"") == b"\x80" and m.rlp_encode([]) == b"\xc0" and m.rlp_encode(b"\x0f") == b"\x0f"
    assert m.rlp_encode(b"\x04\x00") == b"\x82\x04\x00" and m.rlp_encode([[], [[]], [[], [[]]]]) == bytes.fromhex("c7c0c1c0c3c0c1c0")
    text = b"Lorem ipsum dolor sit amet, consectetur adipisicing elit"
    assert m.rlp_encode(text) == b"\xb8\x38" + text
    rng = random.Random(3)
    for _ in range(50):
        x = [bytes(rng.randrange(256) for _ in range(rng.choice([0, 1, 2, 55, 56, 300]))), [b"", [b"\x7f", b"\x80"]]]
        assert m.rlp_decode(m.rlp_encode(x)) == x
    assert m.hex_prefix([1, 2, 3, 4, 5], False) == bytes.fromhex("112345") and m.hex_prefix([0, 1, 2, 3, 4, 5], False) == bytes.fromhex("00012345")
    assert m.hex_prefix([0, 15, 1, 12, 11, 8], True) == bytes.fromhex("200f1cb8") and m.hex_prefix([15, 1, 12, 11, 8], True) == bytes.fromhex("3f1cb8")


def test_the_empty_root_and_trieanyorder():
    assert m.EMPTY_ROOT.hex() == "56e81f171bcc55a6ff8345e692c0f86e5b48e01b996cadc001622fb5e363b421" == m.Trie({}).root.hex()
    items = {b"do": b"verb", b"dog": b"puppy", b"doge": b"coin", b"horse": b"stallion"}
    for order in (list(items), list(reversed(items))):
        assert m.Trie({k: items[k] for k in order}).root.hex() == "5991bb8c6514148a29db676a14ac506cd2cd5775ace63c30a4fe457715e9ac84"


def test_prove_and_verify_agree_on_a_random_trie():
    rng = random.Random(9)
    keys = [bytes(rng.randrange(256) for _ in range(32)) for _ in range(120)]
    trie = m.Trie({k: b"v" * 40 + k[:4] for k in keys})
    for k in keys:
        proof = trie.prove(k)
        status, where, off, n = m.verify(trie.root, k, proof)
        assert status == m.PRESENT and where == len(proof) - 1 and proof[where][off:off + n] == trie.items[k]
        assert m.verify(trie.root, k, proof[:-1])[:2] == (m.SHORT, len(proof) - 1)
        assert m.verify(trie.root, k, proof + proof[-1:])[:2] == (m.LONG, len(proof))
    for _ in range(60):
        k = bytes(rng.randrange(256) for _ in range(32))
        assert m.verify(trie.root, k, trie.prove(k))[0] == m.ABSENT
    assert m.verify(trie.root, keys[0], [])[0] == m.NO_NODES and m.verify(m.EMPTY_ROOT, keys[0], [])[0] == m.ABSENT
    acc = m.account(7, 10 ** 18)
    assert len(m.account()) == 70 and m.parse_account(acc) == (7, 10 ** 18, m.EMPTY_ROOT, m.EMPTY_CODE)


def test_the_genesis_header():
    doc, fields = genesis()
    rlp = m.rlp_encode(fields)
    assert len(rlp) == doc["rlp_bytes"] == 535 and "0x" + keccak256(rlp).hex() == doc["hash"]
    assert doc["hash"] == "0xd4e56740f876aef8c010b86a40d5f56745a118d0906a34e69aec8c0db1cb8fa3"
    assert m.rlp_decode(rlp) == fields


def test_block_header_entry_point(zk):
    doc, fields = genesis()
    rlp = m.rlp_encode(fields)
    h, root, number = zk.eth_block_header(rlp)
    assert "0x" + h.hex() == doc["hash"] and number == 0
    assert root.hex() == "d7f8974fb5ac78d9ac099b9ad5018bedc2ce0a72dad1827a1709da30580f0544"
    built = m.block_header(keccak256(b"a state"), 19000000, extra=b"later")
    assert zk.eth_block_header(built) == (keccak256(built), keccak256(b"a state"), 19000000)
    london = m.rlp_encode(m.rlp_decode(built) + [m._int(7)])                       # a field appended by a later fork
    assert zk.eth_block_header(london) == (keccak256(london), keccak256(b"a state"), 19000000)
    short_root = m.rlp_encode(fields[:3] + [fields[3][:31]] + fields[4:])
    nine_byte_number = m.rlp_encode(fields[:8] + [b"\x01" + bytes(8)] + fields[9:])
    for bad in (rlp[:-1], rlp[:100], rlp + b"\x00", b"", b"\xc0", m.rlp_encode(fields[:8]), short_root, nine_byte_number,
                m.rlp_encode(rlp), m.rlp_encode(fields[:3] + [[fields[3]]] + fields[4:])):
        with pytest.raises(zk.ZkpoaError):
            zk.eth_block_header(bad)
