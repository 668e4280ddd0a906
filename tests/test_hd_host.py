"""The host side of the HD-wallet key sources (include/zkpoa_hd_wallet.h) without a GPU: the BIP-39 seed, the master key,
the readers of extended keys and of paths, and the command-line errors of `ecdsa-sigs-parser` that must come before any
device work. Against tests/hd_ref.py and the vectors of tests/golden/hd/vectors.json."""
import hashlib
import json
import os
import subprocess

import pytest

import hd_ref as hd
import secp_ref as sr
from conftest import GOLDEN, ROOT

N, P = sr.N, sr.P


@pytest.fixture(scope="module")
def vec():
    with open(os.path.join(GOLDEN, "hd", "vectors.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("mnemonic,passphrase", [
    ("test test test test test test test test test test test junk", ""),
    ("legal winner thank year wave sausage worth useful legal winner thank yellow", "TREZOR"),
    ("abandon " * 23 + "art", "a passphrase, with a comma"),      # 187 bytes: above the block of SHA-512, so the key is hashed
    ("", ""), ("x" * 128, "y" * 120), ("x" * 129, "")])
def test_bip39_seed(zk, mnemonic, passphrase):
    want = hashlib.pbkdf2_hmac("sha512", mnemonic.encode(), b"mnemonic" + passphrase.encode(), 2048, 64)
    assert zk.bip39_seed(mnemonic, passphrase) == want == hd.bip39_seed(mnemonic, passphrase)


def test_bip39_seed_published_vector(zk):
    """Trezor's vectors for BIP-39, the second: passphrase TREZOR."""
    got = zk.bip39_seed("legal winner thank year wave sausage worth useful legal winner thank yellow", "TREZOR")
    assert got.hex().startswith("2e8905819b8723fe2c1d161860e5ee1830318dbf49a83bd451cfb8440c28bd6f")


def test_bip39_seed_refuses_what_it_cannot_normalise(zk):
    for mnemonic, passphrase in (("café", ""), ("test", "ü"), ("a" * 4097, "")):
        with pytest.raises(zk.ZkpoaError):
            zk.bip39_seed(mnemonic, passphrase)


def test_master_key(zk, vec):
    v = vec["bip32_vector_1"]
    key, chain = zk.bip32_master(bytes.fromhex(v["seed"]))
    assert key == b"\0" + bytes.fromhex(v["key"]) and chain == bytes.fromhex(v["chain"])
    for seed in (bytes(range(16)), bytes(range(33)), bytes(range(64))):
        assert zk.bip32_master(seed) == hd.master(seed)
    for seed in (b"", bytes(15), bytes(65)):
        with pytest.raises(zk.ZkpoaError):
            zk.bip32_master(seed)


def test_parse_key(zk, vec):
    v = vec["bip32_vector_1"]
    key, chain = b"\0" + bytes.fromhex(v["key"]), bytes.fromhex(v["chain"])
    assert zk.bip32_parse_key(v["xprv"]) == (key, chain, 0, 0)
    assert zk.bip32_parse_key(v["xpub"]) == (hd.neuter(key), chain, 0, 0)
    # depth, child index and a fingerprint, which is ignored
    text = hd.serialize(key, chain, depth=5, index=hd.HARDENED + 7, fingerprint=b"\xde\xad\xbe\xef")
    assert zk.bip32_parse_key(text) == (key, chain, 5, hd.HARDENED + 7) == hd.parse_key(text)
    # a key with leading zero bytes, and the largest private key
    for k in (1, N - 1):
        assert zk.bip32_parse_key(hd.serialize(hd.priv_data(k), chain))[0] == hd.priv_data(k)


def broken_keys(vec):
    v = vec["bip32_vector_1"]
    key, chain = b"\0" + bytes.fromhex(v["key"]), bytes.fromhex(v["chain"])
    pub = hd.neuter(key)
    x = next(x for x in range(1, 100) if sr.lift_x(x, False) is None)
    raw = hd.b58decode(v["xprv"])
    flipped = v["xprv"][:50] + ("A" if v["xprv"][50] != "A" else "B") + v["xprv"][51:]
    return {
        "a flipped character": flipped,
        "a character outside base58": v["xprv"][:60] + "0" + v["xprv"][61:],
        "another one": v["xpub"][:20] + "l" + v["xpub"][21:],
        "a wrong version": hd.serialize(key, chain, version=0x04358394),
        "the public version on a private key": hd.serialize(key, chain, version=hd.XPUB),
        "the private version on a public key": hd.serialize(pub, chain, version=hd.XPRV),
        "a private prefix of 1": hd.serialize(b"\1" + key[1:], chain, version=hd.XPRV),
        "a key of 0": hd.serialize(hd.priv_data(0), chain),
        "a key of n": hd.serialize(hd.priv_data(N), chain),
        "a public prefix of 4": hd.serialize(b"\4" + pub[1:], chain, version=hd.XPUB),
        "an x off the curve": hd.serialize(b"\2" + x.to_bytes(32, "big"), chain, version=hd.XPUB),
        "an x of p or more": hd.serialize(b"\2" + (P + 1).to_bytes(32, "big"), chain, version=hd.XPUB),
        "short": hd.b58encode(raw[:77] + hd.checksum4(raw[:77])),
        "long": hd.b58encode(raw[:78] + b"\0" + hd.checksum4(raw[:78] + b"\0")),
        "a character short": v["xprv"][:-1],
        "a character long": v["xprv"] + "1",
        "a leading 1": "1" + v["xprv"],
        "empty": "",
        "very long": v["xprv"] * 3,
    }


def test_parse_key_refuses(zk, vec):
    cases = broken_keys(vec)
    assert len(cases) == 19
    for what, text in cases.items():
        with pytest.raises(zk.ZkpoaError):
            zk.bip32_parse_key(text)
            pytest.fail("accepted: " + what)
        if what not in ("empty",):
            with pytest.raises(ValueError):
                hd.parse_key(text)


def test_parse_path(zk):
    H = hd.HARDENED
    assert zk.bip32_parse_path("m") == []
    assert zk.bip32_parse_path("m/0") == [0]
    assert zk.bip32_parse_path("m/0'/1h") == [H, H + 1]
    assert zk.bip32_parse_path("m/44'/60'/0'/0") == [H + 44, H + 60, H, 0] == hd.parse_path("m/44'/60'/0'/0")
    assert zk.bip32_parse_path("m/2147483647") == [H - 1] and zk.bip32_parse_path("m/2147483647'") == [2 * H - 1]
    assert zk.bip32_parse_path("m" + "/7" * 255) == [7] * 255
    for bad in ("m/2147483648", "m/4294967296", "m/99999999999999999999", "m//1", "m/", "m/1/", "m" + "/7" * 256, "", "M", "n/0", "m0", "/0",
                "m/-1", "m/0''", "m/0'h", "m/ 1", "m/1 ", "m/0x1", "m/1'2"):
        with pytest.raises(zk.ZkpoaError):
            zk.bip32_parse_path(bad)
            pytest.fail("accepted: %r" % bad)


def test_hd_signatures_match_header(zk):
    """zk-proof-of-assets_amd/_abi.py's HD_SIGNATURES against the prototypes of include/zkpoa_hd_wallet.h, as
    tests/test_abi.py::test_signatures_match_header holds the main table against zkpoa_prover.h: count and class of every
    parameter and of the return value, every symbol exported, and lib() has applied the signatures."""
    import re
    from test_abi import _c_class, _ctypes_class
    from zkpoa_amd import _abi
    text = open(os.path.join(ROOT, "include", "zkpoa_hd_wallet.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    protos = {}
    for ret, name, args in re.findall(r"([\w \t*]+?[\s*])(zkpoa_\w+)\s*\(([^()]*)\)\s*;", text):
        assert name not in protos
        protos[name] = (_c_class(ret + " ret"), [_c_class(a.strip().replace("struct ", "")) for a in args.split(",")])
    assert len(protos) == 9 and list(protos) == list(_abi.HD_SIGNATURES)
    assert not set(protos) & (set(_abi.SIGNATURES) | set(_abi.SIGN_SIGNATURES) | set(_abi.LAYER_INPUT_SIGNATURES) | set(_abi.HOOK_SIGNATURES))
    L = zk.lib()
    wrong = []
    for name, (ret, params) in protos.items():
        restype, argtypes = _abi.signature(_abi.HD_SIGNATURES[name])
        if _ctypes_class(restype) != ret:
            wrong.append("%s: returns %s, the table says %s" % (name, ret, _ctypes_class(restype)))
        if len(argtypes) != len(params):
            wrong.append("%s: %d parameters, the table has %d" % (name, len(params), len(argtypes)))
            continue
        wrong += ["%s: parameter %d is %s, the table says %s" % (name, i, c, _ctypes_class(t))
                  for i, (c, t) in enumerate(zip(params, argtypes)) if _ctypes_class(t) != c]
        fn = getattr(L, name)
        assert fn.argtypes is not None and list(fn.argtypes) == argtypes and fn.restype == restype, name
    assert wrong == []
    # the public header takes the new one in by an #include, which is why its own symbol count stands
    main = open(os.path.join(ROOT, "include", "zkpoa_prover.h")).read()
    assert '#include "zkpoa_hd_wallet.h"' in main and "zkpoa_bip32_children(" not in main


# ---- the command line: refused before any device work ------------------------------------------------------------------------
def run(argv):
    return subprocess.run([str(a) for a in argv], capture_output=True, text=True, timeout=120)


MNEMONIC = "test test test test test test test test test test test junk"


@pytest.mark.parametrize("case", ["two key sources", "two hd sources", "sign with an xpub", "hardened path under an xpub", "no count",
                                  "first + count", "hardened range under an xpub", "bad key", "bad path", "bad seed", "non-ascii mnemonic",
                                  "hd option without a source", "passphrase without a mnemonic", "hd-list without a source"])
def test_command_errors(zk, vec, tmp_path, case):
    v = vec["bip32_vector_1"]
    out = tmp_path / "out.file"
    keys = tmp_path / "keys.txt"
    keys.write_text("5\n")
    sign = [zk.SIGS_BIN, "sign", "--message", "m", "--output-path", out]
    anon = [zk.SIGS_BIN, "anon-set", "--num-addresses", "10", "--output-path", out]
    lst = [zk.SIGS_BIN, "hd-list", "--output-path", out]
    argvs, needle = {
        "two key sources": ([sign + ["--keys", keys, "--mnemonic", MNEMONIC, "--hd-count", "3"],
                             anon + ["--generate-keys", "3", "--seed", "s", "--hd-key", v["xpub"], "--hd-count", "3"]], "exactly one of"),
        "two hd sources": ([lst + ["--hd-key", v["xpub"], "--hd-seed", "0x" + v["seed"], "--hd-count", "3"]], "exclude each other"),
        "sign with an xpub": ([sign + ["--hd-key", v["xpub"], "--hd-count", "3"]], "xpub"),
        "hardened path under an xpub": ([anon + ["--hd-key", v["xpub"], "--hd-path", "m/0/1'", "--hd-count", "3"],
                                         lst + ["--hd-key", v["xpub"], "--hd-path", "m/44h", "--hd-count", "3"]], "hardened"),
        "no count": ([sign + ["--mnemonic", MNEMONIC], anon + ["--hd-key", v["xpub"]], lst + ["--hd-key", v["xprv"]]], "--hd-count"),
        "first + count": ([sign + ["--mnemonic", MNEMONIC, "--hd-first", "4294967295", "--hd-count", "2"],
                           lst + ["--hd-key", v["xprv"], "--hd-first", "4294967296", "--hd-count", "1"]], "2^32"),
        "hardened range under an xpub": ([lst + ["--hd-key", v["xpub"], "--hd-first", "2147483647", "--hd-count", "2"]], "2^31"),
        "bad key": ([lst + ["--hd-key", v["xpub"][:-1] + "9", "--hd-count", "1"]], "--hd-key"),
        "bad path": ([lst + ["--hd-key", v["xprv"], "--hd-path", "m/1/", "--hd-count", "1"]], "--hd-path"),
        "bad seed": ([lst + ["--hd-seed", "0x0011", "--hd-count", "1"], lst + ["--hd-seed", v["seed"], "--hd-count", "1"]], "--hd-seed"),
        "non-ascii mnemonic": ([lst + ["--mnemonic", "café", "--hd-count", "1"]], "ASCII"),
        "hd option without a source": ([sign + ["--keys", keys, "--hd-count", "3"], anon + ["--keys", keys, "--hd-path", "m"]], "goes with"),
        "passphrase without a mnemonic": ([lst + ["--hd-key", v["xprv"], "--passphrase", "p", "--hd-count", "1"]], "--passphrase"),
        "hd-list without a source": ([lst], "HD source"),
    }[case]
    for argv in argvs:
        rc = run(argv)
        assert rc.returncode == 2, (argv, rc.stderr)
        first = rc.stderr.splitlines()[0]
        assert first.startswith("error: ") and needle in first and "Usage:" in rc.stderr, rc.stderr
        assert "HIP" not in rc.stderr                       # it never got as far as the device
        assert sorted(p.name for p in tmp_path.iterdir()) == ["keys.txt"]
