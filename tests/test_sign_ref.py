"""tests/sign_ref.py pinned without a GPU: its two output texts against the reference's committed files, its RFC 6979
against a public secp256k1 vector, its signatures against the restatement's own verification and recovery, and -- where
the reference checkout is present -- against the reference's one committed signature, from the reference's own key."""
import hashlib
import json
import os
import random
import re

import pytest

import secp_ref as sr
import sign_ref as sg
from conftest import ROOT
from test_secp_ref import fixture_text

N = sr.N
REF_KEYS = os.path.join(os.environ.get("ZKPOA_REFERENCE_DIR", "/root/reference"), "tests", "keys.ts")

# RFC 6979 on secp256k1 with SHA-256: key 1, message "Satoshi Nakamoto" (the vector every secp256k1 library carries)
VECTOR = dict(d=1, z=int.from_bytes(hashlib.sha256(b"Satoshi Nakamoto").digest(), "big"),
              k=0x8f8a276c19f4149656b280621e358cce24f5f52542772691ee69063b74f15d15,
              r=0x934b1ea10a4b3c1757e2b0c017d0b6143ce3c9a7e6a4a49860d7a6ab210ee3d8,
              s=0x2442ce9d2b916064108014783e923ec36b49743e2ffa1c4496f01a512aafd9e5, v=28)


def test_signature_text_is_the_reference_file():
    text = fixture_text("signatures_1.json")
    (e,) = json.loads(text)
    sig = e["signature"]
    entry = (int(sig["r"], 16), int(sig["s"], 16), sig["v"], int(sig["msghash"], 16), bytes.fromhex(e["address"][2:]),
             int(e["balance"][:-1]))
    assert sg.signatures_text([entry]) == text
    # two entries: sorted by address, joined without a space, no newline at the end
    other = (1, 2, 27, 3, bytes(19) + b"\x01", 0)
    two = sg.signatures_text([entry, other])
    assert json.loads(two)[0]["address"] == "0x" + "0" * 39 + "1" and json.loads(two)[1] == e
    assert two == sg.signatures_text([other, entry]) and "}},{" not in two and "},{" in two and not two.endswith("\n")
    assert sg.signatures_text([]) == "[]"


def test_csv_text_is_the_reference_file():
    with open(os.path.join(ROOT, "tests", "golden", "ref", "merkle", "anonymity_set_10.csv")) as f:
        text = f.read()
    rows = [line.split(",") for line in text.split("\n")[1:-1]]
    assert len(rows) == 10
    accounts = [(int(a, 16), int(b)) for a, b in rows]
    assert sg.anon_set_csv(accounts) == text
    assert sg.anon_set_csv(accounts[::-1]) == text


def test_public_rfc6979_vector():
    v = VECTOR
    assert sg.nonce(v["d"], v["z"]) == v["k"]
    g = sg.sign(v["d"], v["z"])
    assert (g["status"], g["k"], g["r"], g["s"], g["v"]) == (0, v["k"], v["r"], v["s"], v["v"])
    assert g["pub"] == sr.G


def test_candidates_follow_the_retry_step():
    """Candidate j + 1 is what section 3.2 h.3 derives from candidate j: restated here without the generator."""
    import hmac
    d, z = 0x1234, (1 << 256) - 1
    mac = lambda key, msg: hmac.new(key, msg, hashlib.sha256).digest()
    x, h = sg.be32(d), sg.be32(z - N)
    k = mac(bytes(32), b"\x01" * 32 + b"\x00" + x + h)
    v = mac(k, b"\x01" * 32)
    k = mac(k, v + b"\x01" + x + h)
    v = mac(k, v)
    want = []
    for _ in range(3):
        v = mac(k, v)
        want.append(int.from_bytes(v, "big"))
        k = mac(k, v + b"\x00")
        v = mac(k, v)
    assert [sg.nonce(d, z, j) for j in range(3)] == want
    assert sg.nonce(d, z) == sg.nonce(d, z - N)            # bits2octets reduces the hash


@pytest.mark.skipif(not os.path.exists(REF_KEYS), reason="reference checkout not present")
def test_reference_key_gives_the_reference_signature():
    """The first key of the reference's list, read where the reference lies (it is never committed here), signs the
    fixture's hash to the fixture's r, s, v and address, and has the fixture's balance."""
    with open(REF_KEYS) as f:
        d = int(re.search(r"pvtkeys[^=]*=\s*\[\s*(\d+)n", f.read()).group(1))
    text = fixture_text("signatures_1.json")
    z = int(json.loads(text)[0]["signature"]["msghash"], 16)
    assert sg.sign_text([(d, sg.default_balance(d))], z) == text


def test_every_signature_verifies_and_recovers():
    rng = random.Random(5)
    keys = [1, 2, N - 1, N - 2, (N - 1) // 2, 1 << 255] + [rng.randrange(1, N) for _ in range(6)]
    hashes = [0, N - 1, N, N + 1, (1 << 256) - 1] + [rng.getrandbits(256) for _ in range(2)]
    for i, d in enumerate(keys):
        for z in hashes[i % 2::2] if i >= 6 else hashes:
            g = sg.sign(d, z)
            assert g["status"] == 0 and 0 < g["s"] <= (N - 1) // 2 and g["v"] in (27, 28)
            assert g["pub"] == sr.mul(d, sr.G)
            assert sr.verify(g["r"], g["s"], z % N, g["pub"])
            status, _, pub, addr = sr.recover(g["r"], g["s"], g["v"], z, g["address"])
            assert (status, pub, addr) == (sr.OK, g["pub"], g["address"])
    for d in (0, N, N + 1, (1 << 256) - 1):
        assert sg.sign(d, 5) == sg.ZERO and sg.public_key(d)["status"] == 1


def test_table_multiplication_is_the_plain_one():
    rng = random.Random(9)
    for k in sg.edge_keys() + [rng.randrange(1, N) for _ in range(40)]:
        assert sg.mul_g(k) == sr.mul(k, sr.G), hex(k)


def test_keys_and_accounts():
    assert [sg.derive_key(b"seed", i) for i in range(3)] == [
        int.from_bytes(hashlib.sha256(b"seed" + bytes(7) + bytes([i])).digest(), "big") % (N - 1) + 1 for i in range(3)]
    assert all(0 < sg.derive_key(b"", i) < N for i in range(50))
    text = "# keys\n\n12\n0x0c , 77\n  0X0D\r\n13,0\n"
    assert sg.read_key_file(text) == [(12, 12), (12, 77), (13, 13), (13, 0)]
    assert sg.read_key_file(sg.key_file_text([5, N - 1])) == [(5, 5), (N - 1, (N - 1) % 1000)]
    a, b = sg.filler_account(b"s", 258)
    dig = sr.keccak256(b"sanon" + bytes(6) + b"\x01\x02")
    assert a == int.from_bytes(dig[12:], "big") and b == int.from_bytes(dig[:8], "big") % 1000000
    keys = [(3, 9), (4, 4)]
    assert sg.anon_set_text(keys, b"", 1) == sg.anon_set_csv([(int.from_bytes(sg.public_key(3)["address"], "big"), 9)])
    assert len(sg.anon_set_text(keys, b"", 5).split("\n")) == 7
