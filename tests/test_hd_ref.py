"""tests/hd_ref.py against the published vectors (tests/golden/hd/vectors.json) and against itself: the public derivation
of a neutered parent gives the neutered private derivation. No library, no GPU."""
import hashlib
import json
import os
import random

import pytest

import hd_ref as hd
import secp_ref as sr
import sign_ref as sg
from conftest import GOLDEN

N = sr.N


@pytest.fixture(scope="module")
def vec():
    with open(os.path.join(GOLDEN, "hd", "vectors.json")) as f:
        return json.load(f)


def test_sha512_is_the_standard_one():
    """The vectors of FIPS 180-4 ("abc") and RFC 4231 (test case 2), so that a hashlib that is not what it says shows."""
    assert hashlib.sha512(b"abc").hexdigest().startswith("ddaf35a193617abacc417349ae204131")
    assert hd.hmac512(b"Jefe", b"what do ya want for nothing?").hex().startswith("164b7a7bfcf819e2e395fbe73b56e0a3")


def test_bip32_vector_1(vec):
    v = vec["bip32_vector_1"]
    key, chain = hd.master(bytes.fromhex(v["seed"]))
    assert key == b"\0" + bytes.fromhex(v["key"]) and chain == bytes.fromhex(v["chain"])
    assert hd.serialize(key, chain) == v["xprv"]
    assert hd.serialize(hd.neuter(key), chain) == v["xpub"]
    assert hd.parse_key(v["xprv"]) == (key, chain, 0, 0)
    assert hd.parse_key(v["xpub"]) == (hd.neuter(key), chain, 0, 0)


def test_development_mnemonic(vec):
    v = vec["development_mnemonic"]
    seed = hd.bip39_seed(v["mnemonic"], v["passphrase"])
    key, chain = hd.derive_path(*hd.master(seed), v["path"])
    xpub = hd.neuter(key)
    for c in v["children"]:
        got = hd.child(key, chain, c["index"])
        assert got["status"] == hd.OK and got["key"] == b"\0" + bytes.fromhex(c["key"][2:])
        assert sr.checksum(got["address"]) == c["address"]
        pub = hd.child(xpub, chain, c["index"])
        assert (pub["key"], pub["chain"], pub["pub"], pub["address"]) == (hd.neuter(got["key"]), got["chain"], got["pub"], got["address"])


def test_public_derivation_of_the_neutered_parent():
    """CKDpub(N(k)) == N(CKDpriv(k)) on random parents and indices."""
    rng = random.Random(32)
    for _ in range(12):
        key, chain = hd.priv_data(rng.randrange(1, N)), rng.randbytes(32)
        for i in (0, 1, rng.randrange(hd.HARDENED), hd.HARDENED - 1):
            a, b = hd.child(key, chain, i), hd.child(hd.neuter(key), chain, i)
            assert a["status"] == b["status"] == hd.OK
            assert (b["key"], b["chain"], b["pub"], b["address"]) == (hd.neuter(a["key"]), a["chain"], a["pub"], a["address"])
    with pytest.raises(ValueError):
        hd.child(hd.neuter(hd.priv_data(5)), bytes(32), hd.HARDENED)


def test_tweak_edges():
    k = 0x1234567
    key, pub = hd.priv_data(k), hd.neuter(hd.priv_data(k))
    for il in (0, N, N + 1, (1 << 256) - 1, N - k):
        assert hd.tweak(key, il)["status"] == hd.INVALID, hex(il)
    for il in (0, N, N - k):
        assert hd.tweak(pub, il)["status"] == hd.INVALID, hex(il)
    dbl = hd.tweak(pub, k)
    assert dbl["status"] == hd.OK and dbl["pub"] == sg.mul_g(2 * k) == hd.tweak(key, k)["pub"]


def test_paths():
    assert hd.parse_path("m") == [] and hd.parse_path("m/0'/1h") == [hd.HARDENED, hd.HARDENED + 1]
    assert hd.parse_path("m/2147483647") == [hd.HARDENED - 1]
    for bad in ("", "n/0", "m/", "m//1", "m/2147483648", "m/1/", "m/-1", "m/0''", "m" + "/0" * 256):
        with pytest.raises(ValueError):
            hd.parse_path(bad)
    assert len(hd.parse_path("m" + "/0" * 255)) == 255
