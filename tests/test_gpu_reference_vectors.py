"""The device kernels on vectors this project did not make (tests/golden/extract_reference_vectors.py: signatures by noble
and ethers, addresses by ethers, Poseidon paths by the reference's Rust binary and by circomlibjs): zkpoa_ecdsa_star,
zkpoa_eth_address, zkpoa_keccak256 and zkpoa_poseidon2 must give the values the reference committed. Every comparison is
exact and covers every entry; tests/test_reference_vectors.py holds the same fixtures against the oracles."""
import pytest

import secp_ref as sr
from conftest import le
from oracle.py import poseidon as P
from test_gpu_ecdsa_star import be, run
from test_reference_vectors import (HEIGHT, N_PATHS, N_WITH_ADDRESS, circomlibjs_path, height24_paths, keccak_fixture,
                                    keys_of_paths, none_of, signatures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sigs():
    out = signatures()
    assert len(out) == 258 and sum(s["address"] is not None for s in out) == N_WITH_ADDRESS == 130
    return out


@pytest.fixture(scope="module")
def paths():
    out = height24_paths()
    assert len(out) == N_PATHS == 153
    return out


def _ints(b):
    return [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(len(b) // 32)]


def test_ecdsa_star_on_every_reference_signature(ctx, sigs):
    """One call, 258 lanes: r' and the key are the file's; the address derived is the leaf address where the reference
    holds one (status OK), and differs from the twenty zero bytes handed in where it holds none (status ADDRESS)."""
    got = run(ctx, [(s["r"], s["s"], 27 + (s["rprime"] & 1), s["z"], s["address"] or bytes(20)) for s in sigs])
    assert len(got) == 258
    bad, with_address = [], 0
    for s, (status, rprime, pub, addr) in zip(sigs, got):
        if s["address"] is not None:
            with_address += 1
            ok = (status, rprime, pub, addr) == (sr.OK, s["rprime"], s["pub"], s["address"])
        else:
            ok = (status, rprime, pub) == (sr.ADDRESS, s["rprime"], s["pub"]) and addr == sr.eth_address(s["pub"])
        if not ok:
            bad.append((s["source"], status, "%064x" % rprime, "%064x %064x" % pub, addr.hex()))
    none_of(bad, "signatures whose device recovery differs from the record")
    assert with_address == 130


def test_ecdsa_star_with_the_other_v(ctx, sigs):
    """The other root of r: r' = p - r', and another key, so no entry's address matches. Expected: sr.recover."""
    cases = [(s["r"], s["s"], 28 - (s["rprime"] & 1), s["z"], s["address"] or bytes(20)) for s in sigs]
    want = [sr.recover(*c) for c in cases]
    got = run(ctx, cases)
    assert len(got) == 258
    bad = []
    for s, g, w in zip(sigs, got, want):
        assert w[0] == sr.ADDRESS and w[1] == sr.P - s["rprime"] and w[2] != s["pub"], s["source"]
        if g != w or g[1] != sr.P - s["rprime"] or g[2] == s["pub"]:
            bad.append((s["source"], g[0], "%064x" % g[1], "%064x %064x" % g[2], g[3].hex()))
    none_of(bad, "signatures whose device recovery with the other v differs from sr.recover")


def test_eth_address_of_the_reference_keys(ctx, sigs, paths):
    keys = keys_of_paths(paths, sigs)
    assert len(keys) == 153
    addr, text = ctx.eth_address(b"".join(be(x) + be(y) for x, y in keys))
    assert len(addr) == 20 * 153 and len(text) == 153
    bad = [(p["name"], addr[20 * i:20 * i + 20].hex(), text[i]) for i, p in enumerate(paths)
           if addr[20 * i:20 * i + 20] != p["address"].to_bytes(20, "big") or text[i] != sr.checksum(p["address"].to_bytes(20, "big"))]
    none_of(bad, "keys whose device address or EIP-55 text differs")


def test_keccak256_of_the_reference_preimage(ctx):
    msg, digest = keccak_fixture()
    assert ctx.keccak256(msg, len(msg)) == digest


def test_poseidon2_leaves_of_the_reference_paths(ctx, paths):
    got = _ints(ctx.poseidon2(b"".join(le(p["address"]) for p in paths), b"".join(le(p["balance"]) for p in paths)))
    assert len(got) == 153
    bad = [p["name"] for p, g in zip(paths, got) if g != P.poseidon([p["address"], p["balance"]])]
    none_of(bad, "leaves whose device hash differs from the oracle")


def test_poseidon2_folds_every_reference_path_to_its_root(ctx, paths):
    """24 calls, one per level, each over the 153 height-24 paths and the circomlibjs path (which starts from its raw
    leaf): every path ends at the root its own file holds. Level 0 is compared with the oracle as well."""
    every = paths + [circomlibjs_path()]
    assert len(every) == 154 and all(len(p["elements"]) == HEIGHT == 24 for p in every)
    nodes = _ints(ctx.poseidon2(b"".join(le(p["address"]) for p in paths), b"".join(le(p["balance"]) for p in paths)))
    nodes.append(every[-1]["leaf"])
    for lvl in range(HEIGHT):
        left = [p["elements"][lvl] if p["bits"][lvl] else nd for p, nd in zip(every, nodes)]
        right = [nd if p["bits"][lvl] else p["elements"][lvl] for p, nd in zip(every, nodes)]
        nodes = _ints(ctx.poseidon2(b"".join(le(x) for x in left), b"".join(le(x) for x in right)))
        assert len(nodes) == 154
        if lvl == 0:
            bad = [p["name"] for p, l, r, nd in zip(every, left, right, nodes) if nd != P.poseidon([l, r])]
            none_of(bad, "paths whose level-0 device hash differs from the oracle")
    bad = [p["name"] for p, nd in zip(every, nodes) if nd != p["root"]]
    none_of(bad, "paths that the device does not fold to their root")
