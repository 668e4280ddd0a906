"""The proofs that tests/test_mpt_host.py (the walk compiled for the host) and tests/test_gpu_state_proof.py (the kernels)
both run: tries built by tests/mpt_ref.py, their proofs, and proofs damaged on purpose. A group is one call: one root,
keys and one proof per key. What each item must give is mpt_ref.verify's answer and nothing else."""
import functools
import random

import mpt_ref as m
from secp_ref import keccak256


def group(name, root, keys, proofs):
    return {"name": name, "root": root, "keys": list(keys), "proofs": [list(p) for p in proofs]}


def expected(g):
    """-> [(status, where, value offset within the blob, value length)] by the restatement"""
    _, offsets, _, first = m.layout(g["proofs"])
    out = []
    for key, proof, f in zip(g["keys"], g["proofs"], first):
        status, where, off, n = m.verify(g["root"], key, proof)
        out.append((status, where, offsets[f + where] + off if status == m.PRESENT else 0, n))
    return out


def value_for(key):
    return b"value-" + key + b"-of-forty-four-bytes"[:6]      # 44 bytes: no node is short enough to be embedded


def _flip(key, pos, by=1):
    nib = m.nibbles(key)
    nib[pos] = (nib[pos] + by) % 16
    return bytes(16 * nib[i] + nib[i + 1] for i in range(0, 64, 2))


def with_absent(name, keys, rng, extra_positions=()):
    """A trie over `keys`, every key's proof, and proofs for keys that are not in it: each present key with one nibble
    changed at the ends, in the middle and where the caller says."""
    trie = m.Trie({k: value_for(k) for k in keys})
    ask = list(keys)
    for k in keys[:24]:
        for pos in sorted({0, 1, 31, 32, 62, 63, rng.randrange(64), *extra_positions}):
            other = _flip(k, pos, 1 + rng.randrange(15))
            if other not in trie.items:
                ask.append(other)
    return group(name, trie.root, ask, [trie.prove(k) for k in ask])


def absent_kind(g, i):
    """For an item the restatement calls absent: "slot", "extension" or "leaf", by the node that decided it."""
    status, where, _, _ = m.verify(g["root"], g["keys"][i], g["proofs"][i])
    assert status == m.ABSENT
    node = m.rlp_decode(g["proofs"][i][where])
    return "slot" if len(node) == 17 else ("leaf" if node[0][0] & 0x20 else "extension")


def _shared(rng, nib):
    """two keys whose first `nib` nibbles agree and whose next one differs"""
    a = bytes(rng.randrange(256) for _ in range(32))
    return [a, _flip(a, nib, 1 + rng.randrange(15))]


@functools.lru_cache(maxsize=None)
def raw_groups():
    rng = random.Random(5991)
    out = [with_absent("one key", [bytes(rng.randrange(256) for _ in range(32))], rng)]
    for nib in (0, 1, 2, 31, 32, 63):
        out.append(with_absent("two keys sharing %d nibbles" % nib, _shared(rng, nib), rng, (nib, max(nib - 1, 0))))
    base = bytes(rng.randrange(256) for _ in range(32))
    out.append(with_absent("sixteen keys under one branch", [_flip(base, 0, d) for d in range(16)], rng))
    out.append(with_absent("300 random keys", [bytes(rng.randrange(256) for _ in range(32)) for _ in range(300)], rng))
    return out


@functools.lru_cache(maxsize=None)
def big_trie():
    rng = random.Random(300)
    keys = [bytes(rng.randrange(256) for _ in range(32)) for _ in range(300)]
    return m.Trie({k: value_for(k) for k in keys}), keys


def lanes_group(n):
    trie, keys = big_trie()
    keys = [keys[i % len(keys)] for i in range(n)]
    return group("%d lanes" % n, trie.root, keys, [trie.prove(k) for k in keys])


def keccak_edges_group():
    """Leaves of 135, 136 and 137 bytes (the last byte of a rate block, a whole block, one byte more) beside nodes of
    1, 2, 3 and 4 rate blocks: a root branch, under nibble 0 a full branch (532 bytes, 4 blocks), under nibble 1 a
    branch of eight (276 bytes, 3 blocks), their leaves with a 62-nibble path (37 bytes around the value)."""
    rng = random.Random(136)
    tail = bytes(rng.randrange(256) for _ in range(31))
    items = {}
    for second in range(16):
        items[bytes([0x00 + second]) + tail] = bytes([second]) * (98 + second % 3)     # leaves of 135, 136, 137 bytes
    for second in range(8):
        items[bytes([0x10 + second]) + tail] = bytes([second]) * 44
    trie = m.Trie(items)
    keys = list(items)
    g = group("keccak edges", trie.root, keys, [trie.prove(k) for k in keys])
    sizes = {len(n) for p in g["proofs"] for n in p}
    assert {135, 136, 137, 276, 532} <= sizes and {s // 136 + 1 for s in sizes} == {1, 2, 3, 4}
    return g


def _branch_over(children):
    """a branch node whose slot i holds the hash of children[i]"""
    return m.rlp_encode([keccak256(c) for c in children] + [b""] * (17 - len(children)))


def crafted_group():
    """Nodes no honest trie holds, each under its own slot of one root branch, so that their hashes are right and only
    their content is wrong. The key of slot i begins with nibble i."""
    rest = bytes(31)
    h = bytes(range(32))
    crafted = [
        ("a string length that points past the node", b"\xc4\x20\x85ab"),
        ("a list length that points past the node", b"\xf8\x80" + bytes(40)),
        ("a list shorter than the node", m.rlp_encode([b"\x20", b"v" * 40]) + b"\x00"),
        ("a list of 3 items", m.rlp_encode([b"\x20", h, h])),
        ("a list of 18 items", m.rlp_encode([b""] * 18)),
        ("not a list", m.rlp_encode(b"x" * 40)),
        ("a flag nibble of 4", m.rlp_encode([b"\x40" + bytes(31), b"v" * 40])),
        ("a non-zero pad nibble", m.rlp_encode([b"\x21" + bytes(31), b"v" * 40])),
        ("an empty path item", m.rlp_encode([b"", b"v" * 40])),
        ("a path longer than the key's remainder", m.rlp_encode([b"\x20" + bytes(32), b"v" * 40])),
        ("an extension whose child is 31 bytes", m.rlp_encode([b"\x00" + bytes(2), bytes(31)])),
        ("an extension whose child is empty", m.rlp_encode([b"\x00" + bytes(2), b""])),
        ("a leaf whose value is a list", m.rlp_encode([b"\x3a" + bytes(31), [b"v" * 40]])),
        ("a length of length of 5", b"\xfc\x00\x00\x00\x00\x02\x20\x20"),
        ("an empty node", b""),
        ("a good leaf", m.rlp_encode([b"\x3f" + bytes(31), b"v" * 40])),
    ]
    top = _branch_over([c for _, c in crafted])
    keys = [bytes([16 * i + (15 if name == "a good leaf" else 10 if "list" in name and "leaf" in name else 0)]) + rest
            for i, (name, _) in enumerate(crafted)]
    g = group("crafted nodes", keccak256(top), keys, [[top, c] for _, c in crafted])
    g["names"] = [name for name, _ in crafted]
    return g


def mutation_groups():
    """The 300-key trie's proofs, damaged: -> groups (one per root)."""
    trie, keys = big_trie()
    rng = random.Random(7)
    long_key = max(keys[:60], key=lambda k: len(trie.prove(k)))
    proof = trie.prove(long_key)
    assert len(proof) >= 3
    ks, ps = [], []
    for k in range(len(proof)):                                   # one byte flipped in node k, for every k
        for at in (0, len(proof[k]) // 2, len(proof[k]) - 1):
            bad = bytearray(proof[k])
            bad[at] ^= 1 << rng.randrange(8)
            ks.append(long_key)
            ps.append(proof[:k] + [bytes(bad)] + proof[k + 1:])
    ks.append(long_key)
    ps.append(proof[:-1])                                         # the last node dropped
    ks.append(long_key)
    ps.append(proof[:1] + proof[2:])                              # a middle node dropped
    ks.append(long_key)
    ps.append(proof + [proof[-1]])                                # a node appended
    ks.append(long_key)
    ps.append([])                                                 # no nodes
    a, b = keys[1], keys[2]
    ks += [a, b]
    ps += [trie.prove(b), trie.prove(a)]                          # two items' proofs swapped
    absent = _flip(long_key, 63)
    ks.append(absent)
    ps.append(trie.prove(absent) + [proof[-1]])                   # a node after a proof of absence
    out = [group("damaged proofs", trie.root, ks, ps)]
    out.append(group("a wrong root", keccak256(b"another root"), keys[:5], [trie.prove(k) for k in keys[:5]]))
    out.append(group("no nodes under the empty root", m.EMPTY_ROOT, keys[:2], [[], []]))
    out.append(crafted_group())
    any_order = m.Trie({b"do": b"verb", b"dog": b"puppy", b"doge": b"coin", b"horse": b"stallion"})
    padded = [k + bytes(32 - len(k)) for k in any_order.items]
    out.append(group("trieanyorder", any_order.root, padded, [any_order.prove(k) for k in any_order.items]))
    return out


@functools.lru_cache(maxsize=None)
def account_group():
    """Accounts at the edges of the account form, each alone under its first nibble (a 63-nibble leaf path), among them
    three whose leaves are 135, 136 and 137 bytes long. -> (group keyed by address, [(status, nonce, balance, storage
    root, code hash as the ABI returns them)])."""
    code = keccak256(b"contract code")
    storage = keccak256(b"storage")
    values = [m.account(0, 0), m.account(0, 1), m.account(1, 1 << 64), m.account(2, (1 << 256) - 1), m.account((1 << 64) - 1, 5),
              m.account(7, 10 ** 18, storage, code),
              m.rlp_encode([b"", b"\x00\x05", m.EMPTY_ROOT, m.EMPTY_CODE]),             # a balance with a leading zero byte
              m.rlp_encode([b"\x00", b"\x05", m.EMPTY_ROOT, m.EMPTY_CODE]),             # a nonce that is a zero byte
              m.rlp_encode([b"", b"\x05", m.EMPTY_ROOT, m.EMPTY_CODE, b""]),            # five items
              m.rlp_encode([b"", b"\x05", m.EMPTY_ROOT[:31], m.EMPTY_CODE]),            # a 31-byte storage root
              m.account(1 << 64, 5),                                                       # a 9-byte nonce
              m.account((1 << 64) - 1, (1 << 160) - 1), m.account((1 << 64) - 1, (1 << 168) - 1),
              m.account((1 << 64) - 1, (1 << 176) - 1)]
    addresses, taken, counter = [], set(), 0
    while len(addresses) < len(values):
        a = keccak256(b"address %d" % counter)[:20]
        counter += 1
        if keccak256(a)[0] >> 4 not in taken:
            taken.add(keccak256(a)[0] >> 4)
            addresses.append(a)
    trie = m.account_trie(dict(zip(addresses, values)))
    absent = keccak256(b"nobody")[:20]
    addresses.append(absent)
    proofs = [trie.prove(keccak256(a)) for a in addresses]
    assert {135, 136, 137} <= {len(p[-1]) for p in proofs}
    want = []
    for a, p in zip(addresses, proofs):
        status, where, off, n = m.verify(trie.root, keccak256(a), p)
        acc = m.parse_account(p[where][off:off + n]) if status == m.PRESENT else None
        if status == m.PRESENT and acc is None:
            status = m.ACCOUNT
        nonce, balance, sroot, chash = acc or (0, 0, bytes(32), bytes(32))
        want.append((status, nonce, balance.to_bytes(32, "big").hex(), sroot.hex(), chash.hex()))
    assert [w[0] for w in want].count(m.ACCOUNT) == 5 and want[-1][0] == m.ABSENT
    return group("accounts", trie.root, addresses, proofs), want
