"""HD-wallet key sources on the device (include/zkpoa_hd_wallet.h): batched SHA-512 and HMAC-SHA512, the BIP-32 children of
private and public parents, the tweak step at its edges, paths, and the HD key source of `ecdsa-sigs-parser sign`,
`anon-set` and `hd-list`. Every output byte of every lane is compared with tests/hd_ref.py; the restatement's answers for
the parents and windows are computed once and shared."""
import ctypes
import hashlib
import json
import os
import random
import subprocess

import pytest

import hd_ref as hd
import secp_ref as sr
import sign_ref as sg
from conftest import GOLDEN
from test_hd_host import test_hd_signatures_match_header  # noqa: F401  (the ABI test runs here as well)
from test_secp_ref import sigs_bin  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

N = sr.N
H = hd.HARDENED
be = sg.be32
WINDOWS = [(0, 300), (H - 32, 64), ((1 << 32) - 130, 130)]       # the middle one: both data forms inside one wave
TOP_ZERO_INDEX = 121    # the first child of BIP-32's vector-1 master key whose key begins with a zero byte


@pytest.fixture(scope="module")
def vec():
    with open(os.path.join(GOLDEN, "hd", "vectors.json")) as f:
        return json.load(f)


# ---- SHA-512, HMAC-SHA512 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [0, 1, 55, 56, 111, 112, 113, 119, 120, 127, 128, 129, 239, 240, 241, 256, 4096])
def test_sha512(ctx, length):
    rng = random.Random(length)
    for n in (1, 65, 257):
        msgs = [rng.randbytes(length) for _ in range(n)]
        got = ctx.sha512(b"".join(msgs) if length else n, length)
        assert len(got) == 64 * n
        assert [i for i, m in enumerate(msgs) if got[64 * i:64 * i + 64] != hashlib.sha512(m).digest()] == [], n


def test_sha512_limits(zk, ctx):
    with pytest.raises(zk.ZkpoaError):
        ctx.sha512(bytes(4097), 4097)
    assert ctx.sha512(b"", 7) == b""
    assert ctx.sha512(b"abc", 3).hex().startswith("ddaf35a193617abacc417349ae204131")


@pytest.mark.parametrize("key_len", [0, 1, 12, 32, 127, 128, 129, 200])
def test_hmac_sha512(ctx, key_len):
    rng = random.Random(key_len)
    key = rng.randbytes(key_len)
    for length in (0, 37, 111, 112, 128):
        msgs = [rng.randbytes(length) for _ in range(65)]
        got = ctx.hmac_sha512(key, b"".join(msgs) if length else 65, length)
        assert len(got) == 64 * 65
        assert [i for i, m in enumerate(msgs) if got[64 * i:64 * i + 64] != hd.hmac512(key, m)] == [], length
    assert ctx.hmac_sha512(key, b"", 5) == b""


def test_hmac_sha512_published_vector(zk, ctx):
    assert ctx.hmac_sha512(b"Jefe", b"what do ya want for nothing?", 28).hex().startswith("164b7a7bfcf819e2e395fbe73b56e0a3")   # RFC 4231
    with pytest.raises(zk.ZkpoaError):
        ctx.hmac_sha512(bytes(4097), b"m", 1)


# ---- children ------------------------------------------------------------------------------------------------------------
def device_children(ctx, key, chain, first, n):
    k33, ch, pk, ad, st = ctx.bip32_children(key, chain, first, n)
    assert (len(k33), len(ch), len(pk), len(ad), len(st)) == (33 * n, 32 * n, 64 * n, 20 * n, n)
    return [dict(status=st[i], key=k33[33 * i:33 * i + 33], chain=ch[32 * i:32 * i + 32],
                 pub=(int.from_bytes(pk[64 * i:64 * i + 32], "big"), int.from_bytes(pk[64 * i + 32:64 * i + 64], "big")),
                 address=ad[20 * i:20 * i + 20]) for i in range(n)]


def device_tweak(ctx, key, tweaks):
    n = len(tweaks)
    k33, pk, ad, st = ctx.bip32_tweak(key, b"".join(be(t) for t in tweaks))
    assert (len(k33), len(pk), len(ad), len(st)) == (33 * n, 64 * n, 20 * n, n)
    return [dict(status=st[i], key=k33[33 * i:33 * i + 33],
                 pub=(int.from_bytes(pk[64 * i:64 * i + 32], "big"), int.from_bytes(pk[64 * i + 32:64 * i + 64], "big")),
                 address=ad[20 * i:20 * i + 20]) for i in range(n)]


def public_of(c):
    """What the public derivation gives where the private one gave c."""
    return dict(c, key=hd.neuter(c["key"])) if c["status"] == hd.OK else c


@pytest.fixture(scope="module")
def parents(vec):
    """name -> (key data, chain code, {first index of a window: the restatement's children}). The vector's master key,
    two random parents, and one whose key is below 2^224 (ser256 pads it with four zero bytes)."""
    rng = random.Random(44)
    v = vec["bip32_vector_1"]
    out = {"vector": (b"\0" + bytes.fromhex(v["key"]), bytes.fromhex(v["chain"]))}
    out["random 1"] = (hd.priv_data(rng.randrange(1, N)), rng.randbytes(32))
    out["random 2"] = (hd.priv_data(rng.randrange(1, N)), rng.randbytes(32))
    out["short key"] = (hd.priv_data(rng.randrange(1 << 200, 1 << 224)), rng.randbytes(32))
    return {name: (key, chain, {first: [hd.child(key, chain, first + i) for i in range(n)] for first, n in WINDOWS})
            for name, (key, chain) in out.items()}


@pytest.mark.parametrize("name", ["vector", "random 1", "random 2", "short key"])
def test_children_private(ctx, parents, name):
    key, chain, want = parents[name]
    for first, n in WINDOWS:
        got = device_children(ctx, key, chain, first, n)
        assert [first + i for i in range(n) if got[i] != want[first][i]] == []
        assert all(c["status"] == hd.OK and c["key"][0] == 0 for c in got)
    for n in (0, 1, 63, 64, 65, 257):
        assert device_children(ctx, key, chain, 0, n) == want[0][:n]
    assert device_children(ctx, key, chain, (1 << 32) - 1, 1) == want[(1 << 32) - 130][-1:]


def test_child_key_with_a_zero_top_byte(ctx, parents):
    """Child 121 of the vector's master key: its key begins with a zero byte. (The search is the restatement's, over the
    indices below 5000, as a check on the index written down here.)"""
    key, chain, want = parents["vector"]
    found = [i for i in range(300) if want[0][i]["key"][1] == 0]
    assert found and found[0] == TOP_ZERO_INDEX < 5000
    (got,) = device_children(ctx, key, chain, TOP_ZERO_INDEX, 1)
    assert got == want[0][TOP_ZERO_INDEX] and got["key"][:2] == b"\0\0"


@pytest.mark.parametrize("name", ["vector", "random 1", "random 2", "short key"])
def test_children_public(ctx, parents, name):
    """Under the neutered parent: the same chain codes, public keys and addresses, and the compressed point as key data."""
    key, chain, want = parents[name]
    pub = hd.neuter(key)
    for first, n in ((0, 300), (H - 32, 32)):
        got = device_children(ctx, pub, chain, first, n)
        assert [first + i for i in range(n) if got[i] != public_of(want[first][i])] == []
    for n in (0, 1, 63, 64, 65, 257):
        assert device_children(ctx, pub, chain, 0, n) == [public_of(c) for c in want[0][:n]]
    assert hd.child(pub, chain, 7) == public_of(want[0][7])     # the restatement's own public derivation agrees


def test_public_parent_has_no_hardened_children(zk, ctx, parents):
    """A range that touches 2^31 is an error return, and no output is written."""
    key, chain, _ = parents["vector"]
    pub = hd.neuter(key)
    L = zk.lib()
    for first, n in ((H - 32, 33), (H, 1), ((1 << 32) - 1, 1)):
        bufs = [ctypes.create_string_buffer(b"\xaa" * (size * n), size * n) for size in (33, 32, 64, 20, 1)]
        rc = L.zkpoa_bip32_children(ctx._h, pub, chain, first, n, *bufs)
        assert rc != zk.PROVER_OK and b"hardened" in L.zkpoa_last_error(ctx._h)
        assert all(b.raw == b"\xaa" * len(b.raw) for b in bufs)
    with pytest.raises(zk.ZkpoaError):
        ctx.bip32_children(pub, chain, H - 1, 2)
    assert device_children(ctx, pub, chain, H - 1, 1)[0]["status"] == hd.OK


def test_children_arguments(zk, ctx, parents):
    key, chain, _ = parents["vector"]
    for bad_first, n in (((1 << 32) - 1, 2), (1 << 32, 1), ((1 << 32) + 5, 0)):
        with pytest.raises(zk.ZkpoaError):
            ctx.bip32_children(key, chain, bad_first, n)
    assert ctx.bip32_children(key, chain, 1 << 32, 0) == (b"", b"", b"", b"", b"")
    off_curve = next(x for x in range(1, 100) if sr.lift_x(x, False) is None)
    for bad_key in (hd.priv_data(0), hd.priv_data(N), b"\4" + key[1:], b"\2" + off_curve.to_bytes(32, "big")):
        with pytest.raises(zk.ZkpoaError):
            ctx.bip32_children(bad_key, chain, 0, 1)
    ctx.bip32_children(key, chain, 0, 64)
    assert ctx.last_ms(8) > 0


# ---- the tweak step at its edges ---------------------------------------------------------------------------------------------
def test_tweak_edges_private(ctx):
    rng = random.Random(5)
    for k in (rng.randrange(1, N), 1, N - 1):
        key = hd.priv_data(k)
        tweaks = [0, 1, N - 1, N, N + 1, (1 << 256) - 1, N - k] + sg.edge_keys() + [rng.randrange(1, N) for _ in range(60)]
        want = [hd.tweak(key, il) for il in tweaks]
        got = device_tweak(ctx, key, tweaks)
        assert [hex(il) for il, g, w in zip(tweaks, got, want) if g != w] == []
        assert [w["status"] for w in want[:7]] == [1, 0 if k != N - 1 else 1, 0 if k != 1 else 1, 1, 1, 1, 1]
        assert got[6] == dict(status=1, key=bytes(33), pub=(0, 0), address=bytes(20))


def test_tweak_edges_public(ctx):
    rng = random.Random(6)
    for k in (rng.randrange(1, N), 1, N - 1):
        pub = hd.neuter(hd.priv_data(k))
        tweaks = [k, N - k, 0, N, N + 1, (1 << 256) - 1, 1, N - 1] + sg.edge_keys() + [rng.randrange(1, N) for _ in range(60)]
        want = [hd.tweak(pub, il) for il in tweaks]
        got = device_tweak(ctx, pub, tweaks)
        assert [hex(il) for il, g, w in zip(tweaks, got, want) if g != w] == []
        # IL = k: IL G = K, the doubling; IL = n - k: the point at infinity
        assert got[0]["status"] == 0 and got[0]["pub"] == sr.mul(2 * k % N, sr.G)
        assert [g["status"] for g in got[1:6]] == [1] * 5
        assert got[1] == dict(status=1, key=bytes(33), pub=(0, 0), address=bytes(20))
    assert ctx.bip32_tweak(pub, b"") == (b"", b"", b"", b"")


# ---- paths -----------------------------------------------------------------------------------------------------------------
def test_path_of_the_development_mnemonic(zk, ctx, vec):
    """mnemonic -> seed -> master key -> m/44'/60'/0'/0 -> children 0..2: the pinned keys and addresses."""
    v = vec["development_mnemonic"]
    key, chain = zk.bip32_master(zk.bip39_seed(v["mnemonic"], v["passphrase"]))
    acct = ctx.bip32_derive_path(key, chain, v["path"])
    assert acct == hd.derive_path(key, chain, v["path"])
    got = device_children(ctx, acct[0], acct[1], 0, 3)
    for c, g in zip(v["children"], got):
        assert g["status"] == 0 and g["key"] == b"\0" + bytes.fromhex(c["key"][2:]) and sr.checksum(g["address"]) == c["address"]
    assert ctx.eth_address(b"".join(be(g["pub"][0]) + be(g["pub"][1]) for g in got))[1] == [c["address"] for c in v["children"]]
    # the spelling with h, the empty path, a public path below the account key
    assert ctx.bip32_derive_path(key, chain, "m/44h/60h/0h/0") == acct
    assert ctx.bip32_derive_path(key, chain, "m") == (key, chain)
    xpub = hd.neuter(acct[0])
    assert ctx.bip32_derive_path(xpub, acct[1], "m/2") == (hd.neuter(got[2]["key"]), got[2]["chain"])
    for bad_key, path in ((xpub, "m/0'"), (xpub, "m/1/2h"), (key, "m/"), (key, "m/2147483648"), (b"\5" + key[1:], "m")):
        with pytest.raises(zk.ZkpoaError):
            ctx.bip32_derive_path(bad_key, chain, path)


# ---- the commands ------------------------------------------------------------------------------------------------------------
def run(argv):
    return subprocess.run([str(a) for a in argv], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def account(vec):
    """The development mnemonic's account key m/44'/60'/0'/0 as the test's own xprv / xpub strings (zero fingerprint), and
    its first children as (key, balance = address mod 1000)."""
    v = vec["development_mnemonic"]
    key, chain = hd.derive_path(*hd.master(hd.bip39_seed(v["mnemonic"])), v["path"])
    kids = [hd.child(key, chain, i) for i in range(5)]
    return dict(xprv=hd.serialize(key, chain, depth=4), xpub=hd.serialize(hd.neuter(key), chain, depth=4),
                keys=[(int.from_bytes(c["key"][1:], "big"), hd.hd_balance(c["address"])) for c in kids],
                addresses=[sr.checksum(c["address"]) for c in kids])


def test_sign_command_from_a_mnemonic(sigs_bin, tmp_path, vec, account):
    v = vec["development_mnemonic"]
    z = (1 << 255) + 12345
    out, keys_out, again = tmp_path / "signatures.json", tmp_path / "keys.txt", tmp_path / "again.json"
    rc = run([sigs_bin, "sign", "--mnemonic", v["mnemonic"], "--hd-count", 3, "--msghash", sr.hex32(z), "--output-path", out, "--write-keys", keys_out])
    assert rc.returncode == 0, rc.stderr
    pinned = [(int(c["key"], 16), int(c["address"], 16) % 1000) for c in v["children"]]
    assert pinned == account["keys"][:3]
    assert out.read_text() == sg.sign_text(pinned, z)
    assert keys_out.read_text() == "".join("0x%064x,%d\n" % kb for kb in pinned)
    rc = run([sigs_bin, "sign", "--keys", keys_out, "--msghash", sr.hex32(z), "--output-path", again])
    assert rc.returncode == 0, rc.stderr
    assert again.read_bytes() == out.read_bytes()
    # the same accounts from the account-level xprv in a file, from the second child on
    (tmp_path / "xprv.txt").write_text(account["xprv"] + "\n")
    rc = run([sigs_bin, "sign", "--hd-key", "@" + str(tmp_path / "xprv.txt"), "--hd-first", 1, "--hd-count", 4, "--msghash", sr.hex32(z), "-o", again])
    assert rc.returncode == 0, rc.stderr
    assert again.read_text() == sg.sign_text(account["keys"][1:5], z)


def test_anon_set_command_from_xpub_and_xprv(sigs_bin, tmp_path, vec, account):
    v = vec["development_mnemonic"]
    a, b, c = tmp_path / "a.csv", tmp_path / "b.csv", tmp_path / "c.csv"
    for key, path in ((account["xpub"], a), (account["xprv"], b)):
        rc = run([sigs_bin, "anon-set", "--hd-key", key, "--hd-count", 5, "--num-addresses", 40, "--output-path", path])
        assert rc.returncode == 0, rc.stderr
    assert a.read_bytes() == b.read_bytes()
    assert a.read_text() == sg.anon_set_text(account["keys"], b"", 40)
    (tmp_path / "words.txt").write_text(v["mnemonic"] + "\n")
    rc = run([sigs_bin, "anon-set", "--mnemonic", "@" + str(tmp_path / "words.txt"), "--hd-count", 5, "-n", 3, "-o", c])
    assert rc.returncode == 0, rc.stderr
    assert c.read_text() == sg.anon_set_text(account["keys"][:3], b"", 3)


def test_hd_list_command(sigs_bin, tmp_path, vec, account):
    v = vec["development_mnemonic"]
    out = tmp_path / "addresses.csv"
    rc = run([sigs_bin, "hd-list", "--hd-key", account["xpub"], "--hd-count", 3, "--output-path", out])
    assert rc.returncode == 0, rc.stderr
    assert out.read_text() == "index,address\n" + "".join("%d,%s\n" % (c["index"], c["address"]) for c in v["children"])
    seed = hd.bip39_seed(v["mnemonic"])
    rc = run([sigs_bin, "hd-list", "--hd-seed", "0x" + seed.hex(), "--hd-first", 3, "--hd-count", 2, "-o", out])
    assert rc.returncode == 0, rc.stderr
    assert out.read_text() == "index,address\n" + "".join("%d,%s\n" % (3 + i, a) for i, a in enumerate(account["addresses"][3:5]))
    rc = run([sigs_bin, "hd-list", "--mnemonic", v["mnemonic"], "--passphrase", "p", "--hd-path", "m/0", "--hd-count", 1, "-o", out])
    assert rc.returncode == 0, rc.stderr
    key, chain = hd.derive_path(*hd.master(hd.bip39_seed(v["mnemonic"], "p")), "m/0")
    assert out.read_text() == "index,address\n0,%s\n" % sr.checksum(hd.child(key, chain, 0)["address"])
