"""The reference's own vectors (tests/golden/extract_reference_vectors.py; made by noble, ethers, circomlibjs, the Rust
Poseidon of its Merkle binary and py_ecc) against this project's oracles and host code, without a GPU: signatures,
public key -> address, Keccak, the height-24 Merkle paths and the py_ecc sanitiser's output. The device runs the same
fixtures in tests/test_gpu_reference_vectors.py; a failure there that does not show here is the kernel's."""
import json
import os

import secp_ref as sr
from conftest import GOLDEN
from oracle.py import bn254 as bn
from oracle.py import groth16 as g16
from oracle.py import poseidon as P

N_EXPERIMENTS, N_TESTS, N_WITH_ADDRESS = 128, 130, 130      # distinct signatures; those first met in tests/old/N_sigs
N_PATHS, HEIGHT, N_SIBLINGS = 153, 24, 979
SET_SIZES = [2, 7, 16, 128]


def none_of(bad, what):
    """Fails with every entry of bad written out (a plain `bad == []` shortens a long list)."""
    assert not bad, "%d %s: %s" % (len(bad), what, "; ".join(str(b) for b in bad))


def _json(*parts):
    with open(os.path.join(GOLDEN, *parts)) as f:
        return json.load(f)


def _text(*parts):
    with open(os.path.join(GOLDEN, *parts)) as f:
        return f.read()


def signatures():
    """Every reference signature once: dicts of source, r, s, rprime, z, pub (x, y), address (20 bytes or None)."""
    out = []
    for name in ("reference_ecdsa_star_experiments.json", "reference_ecdsa_star_tests.json"):
        for rec in _json("sigs", name):
            assert set(rec) == {"source", "r", "s", "rprime", "msghash", "pubkey_x", "pubkey_y", "address"}, rec["source"]
            assert all(len(rec[k]) == 64 for k in ("r", "s", "rprime", "msghash", "pubkey_x", "pubkey_y")), rec["source"]
            assert rec["address"] is None or len(rec["address"]) == 40, rec["source"]
            out.append(dict(source=rec["source"], r=int(rec["r"], 16), s=int(rec["s"], 16), rprime=int(rec["rprime"], 16),
                            z=int(rec["msghash"], 16), pub=(int(rec["pubkey_x"], 16), int(rec["pubkey_y"], 16)),
                            address=None if rec["address"] is None else bytes.fromhex(rec["address"])))
    return out


def height24_paths():
    """The 153 paths: dicts of name (source file and position), address, balance, root, elements, bits."""
    d = _json("ref", "merkle", "height24_paths.json")
    sib = [int(x) for x in d["siblings"]]
    out = []
    for s in d["sets"]:
        for i in range(len(s["leaf_addresses"])):
            out.append(dict(name="%s path %d" % (s["source"], i), address=int(s["leaf_addresses"][i]),
                            balance=int(s["leaf_balances"][i]), root=int(s["merkle_root"]),
                            elements=[sib[k] for k in s["path_elements"][i]], bits=[int(b) for b in s["path_indices"][i]]))
    return out


def circomlibjs_path():
    """The circomlibjs path in the same form; its `leaf` is a node value, not an (address, balance) pair."""
    d = _json("ref", "merkle", "circomlibjs_path.json")
    return dict(name="circomlibjs_path.json", leaf=int(d["leaf"]), root=int(d["root"]),
                elements=[int(x) for x in d["pathElements"]], bits=[int(b) for b in d["pathIndices"]])


def keys_of_paths(paths, sigs):
    """The public key of every path's leaf: tests/old/N_sigs/layer_two_input.json lists the keys of that directory's
    layer-one file in its order, and the signature records of those files carry that file's leaf address."""
    by_address = {s["address"]: s["pub"] for s in sigs if s["address"] is not None}
    missing = [p["name"] for p in paths if p["address"].to_bytes(20, "big") not in by_address]
    none_of(missing, "paths whose leaf address no signature record has")
    return [by_address[p["address"].to_bytes(20, "big")] for p in paths]


def keccak_fixture():
    """(preimage bytes, hash bytes) of keccak_inputs.json: bits as strings, least significant bit of each byte first."""
    d = _json("sigs", "keccak_inputs.json")
    unbits = lambda bits: bytes(sum(int(b) << k for k, b in enumerate(bits[i:i + 8])) for i in range(0, len(bits), 8))
    return unbits(d["preimagebits"]), unbits(d["hashbits"])


def fold(p, node, hash2=lambda l, r: P.poseidon([l, r])):
    for e, bit in zip(p["elements"], p["bits"]):
        node = hash2(e, node) if bit else hash2(node, e)
    return node


# ---- the fixtures' shape -------------------------------------------------------------------------------------------------
def test_fixture_shape():
    sigs = signatures()
    assert len(sigs) == N_EXPERIMENTS + N_TESTS >= 256
    assert len({(s["r"], s["s"], s["z"]) for s in sigs}) == len(sigs)
    assert sum(s["address"] is not None for s in sigs) == N_WITH_ADDRESS
    assert {s["rprime"] & 1 for s in sigs} == {0, 1}
    assert {s["z"] for s in sigs if "experiments/" in s["source"]} == {1234}
    assert len({s["z"] for s in sigs if s["source"].startswith("tests/")}) == 2
    for s in sigs:
        assert 0 < s["r"] < sr.N and 0 < s["s"] <= sr.N // 2, s["source"]
    paths = height24_paths()
    assert len(paths) == N_PATHS
    assert [sum(p["name"].startswith("tests/old/%d_sigs/" % n) for p in paths) for n in SET_SIZES] == SET_SIZES
    assert all(len(p["elements"]) == HEIGHT and len(p["bits"]) == HEIGHT and set(p["bits"]) <= {0, 1} for p in paths)
    assert len({e for p in paths for e in p["elements"]}) >= N_SIBLINGS
    assert len(_json("ref", "merkle", "height24_paths.json")["siblings"]) == N_SIBLINGS       # no value twice in the table
    c = circomlibjs_path()
    assert len(c["elements"]) == HEIGHT and c["bits"] == [1] * HEIGHT
    assert len(keys_of_paths(paths, sigs)) == N_PATHS


def test_no_fixture_outgrows_the_largest():
    limit = os.path.getsize(os.path.join(GOLDEN, "gen", "vectors.json"))
    for parts in (("sigs", "reference_ecdsa_star_experiments.json"), ("sigs", "reference_ecdsa_star_tests.json"),
                  ("ref", "merkle", "height24_paths.json")):
        assert os.path.getsize(os.path.join(GOLDEN, *parts)) <= limit, parts


# ---- oracles on the fixtures ---------------------------------------------------------------------------------------------
def test_recover_gives_the_reference_rprime_and_key():
    bad = []
    for s in signatures():
        want = (sr.OK if s["address"] is not None else sr.ADDRESS, s["rprime"], s["pub"])
        got = sr.recover(s["r"], s["s"], 27 + (s["rprime"] & 1), s["z"], s["address"] or bytes(20))
        if got[:3] != want or s["address"] not in (None, got[3]):
            bad.append(s["source"])
    none_of(bad, "signatures whose recovery differs from the record")


def test_addresses_of_the_reference_keys():
    paths = height24_paths()
    keys = keys_of_paths(paths, signatures())
    none_of([p["name"] for p, pub in zip(paths, keys) if sr.eth_address(pub) != p["address"].to_bytes(20, "big")],
            "keys whose address is not the leaf address")


def test_keccak_of_the_reference_preimage():
    msg, digest = keccak_fixture()
    assert msg == b"test" and len(digest) == 32
    assert sr.keccak256(msg) == digest


def test_height24_paths_fold_to_their_roots():
    none_of([p["name"] for p in height24_paths() if fold(p, P.poseidon([p["address"], p["balance"]])) != p["root"]],
            "paths that do not fold to their root")
    c = circomlibjs_path()
    assert fold(c, c["leaf"]) == c["root"], c["name"]


def _limbs43(v):
    assert len(v) == 6 and all(0 <= int(x) < 1 << 43 for x in v)
    return sum(int(x) << (43 * i) for i, x in enumerate(v))


def _g1(v):
    return (_limbs43(v[0]), _limbs43(v[1]))


def _g2(v):
    return ((_limbs43(v[0][0]), _limbs43(v[0][1])), (_limbs43(v[1][0]), _limbs43(v[1][1])))


def test_py_ecc_sanitiser_output_recombines_to_the_snarkjs_files():
    s = _json("ref", "snarkjs_style", "full-circom-input.json")
    vkey, proof, public = (_json("ref", "snarkjs_style", n) for n in ("vkey.json", "proof.json", "public.json"))
    assert _g1(s["negpa"]) == bn.ec_neg(g16.g1_from_obj(proof["pi_a"]), bn.FQ)
    assert _g2(s["pb"]) == g16.g2_from_obj(proof["pi_b"])
    assert _g1(s["pc"]) == g16.g1_from_obj(proof["pi_c"])
    assert _g2(s["gamma2"]) == g16.g2_from_obj(vkey["vk_gamma_2"])
    assert _g2(s["delta2"]) == g16.g2_from_obj(vkey["vk_delta_2"])
    assert len(s["IC"]) == 6 and [_g1(p) for p in s["IC"]] == [g16.g1_from_obj(p) for p in vkey["IC"]]
    assert len(public) == 5 and s["pubInput"] == [int(v) for v in public]
    from test_oracle_fixtures import _fq12_from_sanitized
    e_neg = bn.pairing(g16.g2_from_obj(vkey["vk_beta_2"]), bn.ec_neg(g16.g1_from_obj(vkey["vk_alpha_1"]), bn.FQ))
    assert bn.FQ12.eq(e_neg, _fq12_from_sanitized(s["negalfa1xbeta2"]))
    assert g16.verify(vkey, public, proof) is True


# ---- the product's host code ---------------------------------------------------------------------------------------------
def test_verifier_accepts_the_snarkjs_style_proof(zk):
    """Five public inputs, six IC points, snarkjs layout: the reference's sixth verifier vector."""
    vkey, public, proof = (_text("ref", "snarkjs_style", n) for n in ("vkey.json", "public.json", "proof.json"))
    assert zk.groth16_verify(vkey, public, proof) is True
    for i in range(5):
        pub = json.loads(public)
        pub[i] = str(int(pub[i]) + 1)
        assert zk.groth16_verify(vkey, json.dumps(pub), proof) is False, i
    pr = json.loads(proof)
    pr["pi_a"], pr["pi_c"] = pr["pi_c"], pr["pi_a"]
    assert zk.groth16_verify(vkey, public, json.dumps(pr)) is False


def _ints(v):
    return [_ints(x) for x in v] if isinstance(v, list) else int(v)


def test_sanitiser_equals_py_ecc_on_the_snarkjs_style_proof(zk):
    want = _json("ref", "snarkjs_style", "full-circom-input.json")
    got = json.loads(zk.sanitize_proof(*(_text("ref", "snarkjs_style", n) for n in ("vkey.json", "public.json", "proof.json"))))
    assert set(got) == set(want)
    for k in want:
        assert _ints(got[k]) == _ints(want[k]), k
