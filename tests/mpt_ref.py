"""A pure-Python Merkle-Patricia trie on secp_ref.keccak256: the restatement that decides every expected status of
tests/test_gpu_state_proof.py. RLP, hex-prefix, a builder from a dict (embedded nodes included), prove(), verify() with
the statuses of include/zkpoa_state_proof.h, an account encoder, the blob layout of the C ABI and a writer of the
JSON Lines file. Written from the Ethereum yellow paper (appendices B, C, D); tests/test_mpt_ref.py pins it on public
vectors. Nothing here calls the code under test."""
import json

from secp_ref import keccak256

PRESENT, ABSENT, NO_NODES, HASH, RLP, CHILD, SHORT, LONG, HEX_PREFIX, ACCOUNT = range(10)
STATUS_NAMES = ["present", "absent", "no nodes", "hash", "rlp", "child", "short", "long", "hex-prefix", "account"]
EMPTY_ROOT = keccak256(b"\x80")
EMPTY_CODE = keccak256(b"")


# ---- RLP ---------------------------------------------------------------------------------------------------------------
def _header(n, base):
    if n <= 55:
        return bytes([base + n])
    be = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([base + 55 + len(be)]) + be


def rlp_encode(x):
    """bytes -> a string, list -> a list"""
    if isinstance(x, (bytes, bytearray)):
        x = bytes(x)
        return x if len(x) == 1 and x[0] < 0x80 else _header(len(x), 0x80) + x
    body = b"".join(rlp_encode(v) for v in x)
    return _header(len(body), 0xc0) + body


def rlp_item(data, p, end):
    """The item at data[p:end] -> (is list, payload offset, payload length, offset after it), None when it is malformed
    or leaves [p, end). Length-of-length above 4 is refused: a node is below 2^32 bytes."""
    if p >= end:
        return None
    b = data[p]
    if b < 0x80:
        return False, p, 1, p + 1
    is_list = b >= 0xc0
    base = 0xc0 if is_list else 0x80
    if b - base <= 55:
        payload, n = p + 1, b - base
    else:
        ll = b - base - 55
        if ll > 4 or p + 1 + ll > end:
            return None
        payload, n = p + 1 + ll, int.from_bytes(data[p + 1:p + 1 + ll], "big")
    if payload + n > end:
        return None
    return is_list, payload, n, payload + n


def rlp_decode(data):
    """Strict enough for the tests: the whole of `data` is one item -> bytes or nested lists."""
    def at(p, end):
        it = rlp_item(data, p, end)
        assert it is not None, "malformed RLP"
        is_list, payload, n, nxt = it
        if not is_list:
            return bytes(data[payload:payload + n]), nxt
        out, q = [], payload
        while q < nxt:
            v, q = at(q, nxt)
            out.append(v)
        return out, nxt
    v, nxt = at(0, len(data))
    assert nxt == len(data), "bytes after the item"
    return v


# ---- hex-prefix (yellow paper appendix C) ---------------------------------------------------------------------------------
def nibbles(key):
    return [n for b in key for n in (b >> 4, b & 15)]


def hex_prefix(path, leaf):
    flag = (2 if leaf else 0) + (len(path) & 1)
    full = [flag] + ([] if len(path) & 1 else [0]) + list(path)
    return bytes(16 * full[i] + full[i + 1] for i in range(0, len(full), 2))


# ---- the trie (appendix D) ------------------------------------------------------------------------------------------------
class Trie:
    """Built once from {key bytes: value bytes}; keys may differ in length (the public vector's do). A subtrie is a range
    [lo, hi) of the sorted keys at a depth; every one is built and encoded once."""

    def __init__(self, items):
        self.items = {bytes(k): bytes(v) for k, v in items.items()}
        self.pairs = sorted((nibbles(k), v) for k, v in self.items.items())
        self._nodes = {}                         # (lo, hi, depth) -> (structure, its RLP)
        self.root = keccak256(self._node(0, len(self.pairs), 0)[1]) if self.pairs else EMPTY_ROOT

    def _common(self, lo, hi, depth):
        first, last = self.pairs[lo][0], self.pairs[hi - 1][0]
        common = 0
        while depth + common < min(len(first), len(last)) and first[depth + common] == last[depth + common]:
            common += 1
        return common

    def _children(self, lo, hi, depth):
        """the ranges of a branch: nibble -> (lo, hi)"""
        out = {}
        for i in range(lo, hi):
            path = self.pairs[i][0]
            if len(path) > depth:
                a, _ = out.get(path[depth], (i, i))
                out[path[depth]] = (a, i + 1)
        return out

    def _ref(self, lo, hi, depth):
        """How a parent names a child: the structure itself when its RLP is shorter than 32 bytes, else its hash."""
        node, enc = self._node(lo, hi, depth)
        return node if len(enc) < 32 else keccak256(enc)

    def _node(self, lo, hi, depth):
        key = (lo, hi, depth)
        if key not in self._nodes:
            if hi - lo == 1:
                path, value = self.pairs[lo]
                node = [hex_prefix(path[depth:], True), value]
            else:
                common = self._common(lo, hi, depth)
                if common:
                    node = [hex_prefix(self.pairs[lo][0][depth:depth + common], False), self._ref(lo, hi, depth + common)]
                else:
                    node = [b""] * 17
                    if len(self.pairs[lo][0]) == depth:
                        node[16] = self.pairs[lo][1]
                    for nib, (a, b) in self._children(lo, hi, depth).items():
                        node[nib] = self._ref(a, b, depth + 1)
            self._nodes[key] = (node, rlp_encode(node))
        return self._nodes[key]

    def prove(self, key):
        """The nodes a walk for `key` visits that are referred to by hash, root first (what eth_getProof returns):
        embedded nodes travel inside their parent."""
        path, out = nibbles(bytes(key)), []
        if not self.pairs:
            return out
        lo, hi, depth = 0, len(self.pairs), 0
        while True:
            node, enc = self._node(lo, hi, depth)
            if depth == 0 or len(enc) >= 32:
                out.append(enc)
            if len(node) == 17:
                nxt = self._children(lo, hi, depth).get(path[depth]) if depth < len(path) else None
                if nxt is None:
                    return out
                lo, hi, depth = nxt[0], nxt[1], depth + 1
                continue
            if hi - lo == 1:
                return out
            common = self._common(lo, hi, depth)
            if path[depth:depth + common] != self.pairs[lo][0][depth:depth + common]:
                return out
            depth += common


# ---- verification: the statuses of include/zkpoa_state_proof.h ------------------------------------------------------------
def verify(root, key32, proof):
    """-> (status, where, value offset within its node or None, value length). The first failing condition in walk order
    wins; `where` is the index of the node at which the status arose (SHORT: the proof's length)."""
    if not proof:
        return (ABSENT if root == EMPTY_ROOT else NO_NODES), 0, None, 0
    path = nibbles(key32)
    assert len(path) == 64
    expect, pos, ended = root, 0, None
    for k, node in enumerate(proof):
        if ended is not None:
            return LONG, k, None, 0
        if keccak256(node) != expect:
            return HASH, k, None, 0
        top = rlp_item(node, 0, len(node))
        if top is None or not top[0] or top[3] != len(node):
            return RLP, k, None, 0
        items, p = [], top[1]
        while p < top[3]:
            it = rlp_item(node, p, top[3])
            if it is None or len(items) == 17:
                return RLP, k, None, 0
            items.append(it)
            p = it[3]
        if len(items) not in (2, 17):
            return RLP, k, None, 0
        if len(items) == 17:
            if pos >= 64:
                return HEX_PREFIX, k, None, 0
            is_list, payload, n, _ = items[path[pos]]
            pos += 1
            if not is_list and n == 0:
                ended = (ABSENT, k, None, 0)
                continue
            if is_list or n != 32:
                return CHILD, k, None, 0
            expect = bytes(node[payload:payload + 32])
            continue
        head, second = items
        if head[0]:
            return RLP, k, None, 0
        if head[2] == 0:
            return HEX_PREFIX, k, None, 0
        hp = node[head[1]:head[1] + head[2]]
        flag = hp[0] >> 4
        if flag > 3 or (not flag & 1 and hp[0] & 15):
            return HEX_PREFIX, k, None, 0
        sub = nibbles(hp)[1 if flag & 1 else 2:]
        if len(sub) > 64 - pos:
            return HEX_PREFIX, k, None, 0
        same = path[pos:pos + len(sub)] == sub
        if flag & 2:
            if second[0]:
                return RLP, k, None, 0
            if same and len(sub) == 64 - pos:
                ended = (PRESENT, k, second[1], second[2])
            else:
                ended = (ABSENT, k, None, 0)
            continue
        if not same:
            ended = (ABSENT, k, None, 0)
            continue
        if second[0] or second[2] != 32:
            return CHILD, k, None, 0
        pos += len(sub)
        expect = bytes(node[second[1]:second[1] + 32])
    if ended is None:
        return SHORT, len(proof), None, 0
    return ended


# ---- accounts --------------------------------------------------------------------------------------------------------------
def _int(x):
    return x.to_bytes((x.bit_length() + 7) // 8, "big")


def account(nonce=0, balance=0, storage_root=EMPTY_ROOT, code_hash=EMPTY_CODE):
    return rlp_encode([_int(nonce), _int(balance), storage_root, code_hash])


def parse_account(value):
    """-> (nonce, balance, storage root, code hash), or None for what include/zkpoa_state_proof.h calls no account"""
    top = rlp_item(value, 0, len(value))
    if top is None or not top[0] or top[3] != len(value):
        return None
    fields, p = [], top[1]
    for _ in range(4):
        it = rlp_item(value, p, top[3])
        if it is None or it[0]:
            return None
        fields.append(bytes(value[it[1]:it[1] + it[2]]))
        p = it[3]
    if p != top[3] or len(fields[0]) > 8 or len(fields[1]) > 32 or len(fields[2]) != 32 or len(fields[3]) != 32:
        return None
    if fields[0][:1] == b"\0" or fields[1][:1] == b"\0":
        return None
    return int.from_bytes(fields[0], "big"), int.from_bytes(fields[1], "big"), fields[2], fields[3]


def account_trie(accounts):
    """{20-byte address: account RLP} -> the trie keyed by Keccak-256 of the address"""
    return Trie({keccak256(a): v for a, v in accounts.items()})


# ---- the C ABI's layout and the file -------------------------------------------------------------------------------------
def layout(proofs):
    """A list of proofs (each a list of node bytes) -> (blob, node_offset, node_length, first_node): every node on an
    8-byte boundary, zero between them."""
    blob, offsets, lengths, first = bytearray(), [], [], [0]
    for proof in proofs:
        for node in proof:
            offsets.append(len(blob))
            lengths.append(len(node))
            blob += node + bytes(-len(node) % 8)
        first.append(len(offsets))
    return bytes(blob), offsets, lengths, first


def proof_json(address, proof, envelope=False, balance=None, ident=1):
    """One line of the proofs file: what eth_getProof returns (the members the reader skips included)"""
    obj = {"address": "0x" + address.hex(), "balance": hex(balance if balance is not None else 0), "codeHash": "0x" + EMPTY_CODE.hex(),
           "nonce": "0x0", "storageHash": "0x" + EMPTY_ROOT.hex(), "accountProof": ["0x" + n.hex() for n in proof],
           "storageProof": []}
    return json.dumps({"jsonrpc": "2.0", "id": ident, "result": obj} if envelope else obj)


def write_jsonl(path, lines):
    with open(path, "w") as f:
        f.write("".join(line + "\n" for line in lines))


def block_header(state_root, number, parent=bytes(32), extra=b""):
    """A pre-London header's RLP with the given state root and number"""
    return rlp_encode([parent, keccak256(rlp_encode([])), bytes(20), state_root, EMPTY_ROOT, EMPTY_ROOT, bytes(256), _int(1 << 17),
                       _int(number), _int(5000), b"", _int(1438269988), extra, bytes(32), bytes(8)])
