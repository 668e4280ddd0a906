"""tests/secp_ref.py pinned before anything is measured against it (no GPU): its Keccak permutation against the standard
library, its recovery against the reference's committed data, its generator against its own recovery, and the host-only
mode of the command against the one output file the reference committed."""
import hashlib
import json
import os
import random
import subprocess

import pytest

import secp_ref as sr
from conftest import GOLDEN

# the reference's three data files of this step; not under golden/ref/, every directory of which is a proof fixture
SIGS = os.path.join(GOLDEN, "sigs")


def fixture_text(name):
    with open(os.path.join(SIGS, name)) as f:
        return f.read()


def from_limbs(limbs):
    return sum(int(v) << (64 * i) for i, v in enumerate(limbs))


@pytest.fixture(scope="module")
def sigs_bin(zk):
    """The executable; the session fixture does not know it, so a tree built before it existed is built again."""
    if not os.path.exists(zk.SIGS_BIN):
        import __graft_entry__ as entry
        entry.build()
    return zk.SIGS_BIN


@pytest.mark.parametrize("length", [0, 1, 135, 136, 137, 272])
def test_sponge_with_the_sha3_pad_is_sha3_256(length):
    msg = bytes(random.Random(length).randrange(256) for _ in range(length))
    assert sr.sponge256(msg, 0x06) == hashlib.sha3_256(msg).digest()


def test_keccak256_of_the_empty_message():
    assert sr.keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"


def test_reference_vector():
    (entry,) = json.loads(fixture_text("signatures_1.json"))
    want = json.loads(fixture_text("layer_one_input.json"))
    sig = entry["signature"]
    r, s, z = int(sig["r"], 16), int(sig["s"], 16), int(sig["msghash"], 16)
    status, rprime, pub, addr = sr.recover(r, s, sig["v"], z, bytes.fromhex(entry["address"][2:]))
    assert status == sr.OK
    assert sr.limbs64(rprime) == want["rprime"][0]
    assert [sr.limbs64(pub[0]), sr.limbs64(pub[1])] == want["pubkey"][0]
    assert sr.limbs64(r) == want["r"][0] and sr.limbs64(s) == want["s"][0] and sr.limbs64(z) == want["msghash"][0]
    assert sr.checksum(addr) == entry["address"] == "0x668e97bfD9851AF354C0508D6C180dDc68244826"
    assert sr.verify(r, s, z, pub)
    # both texts of the command, through the restatement alone
    assert sr.layer_one_text(sr.parser_output_text(fixture_text("signatures_1.json"))) == fixture_text("layer_one_input.json")


def test_verification_vector():
    v = json.loads(fixture_text("ecdsa_verification_inputs.json"))
    pub = (from_limbs(v["pubkey"][0]), from_limbs(v["pubkey"][1]))
    assert sr.on_curve(pub)
    assert sr.verify(from_limbs(v["signatureR"]), from_limbs(v["signatureS"]), from_limbs(v["msghash"]), pub)
    assert not sr.verify(from_limbs(v["signatureR"]), from_limbs(v["signatureS"]), from_limbs(v["msghash"]) ^ 1, pub)


def test_generator_agrees_with_recover():
    entries = sr.generate(64, seed=7)
    for e in entries:
        assert sr.on_curve(e["pub"]) and e["s"] < 1 << 255
        assert sr.recover(e["r"], e["s"], e["v"], e["z"], e["address"]) == (sr.OK, e["rprime"], e["pub"], e["address"])
    # without the replacement of a high s some entries carry one, and recovery refuses exactly those
    raw = sr.generate(64, seed=7, low_s=False)
    high = [e for e in raw if e["s"] >= 1 << 255]
    assert high and len(high) < 64
    for e in raw:
        status = sr.recover(e["r"], e["s"], e["v"], e["z"], e["address"])[0]
        assert status == (sr.HIGH_S if e["s"] >= 1 << 255 else sr.OK)


def test_layer_one_input_mode(sigs_bin, tmp_path):
    """Host only: the parser's output as the restatement writes it -> the reference's committed layer_one_input.json."""
    parsed = tmp_path / "parsed.json"
    parsed.write_text(sr.parser_output_text(fixture_text("signatures_1.json")))
    out = tmp_path / "layer_one_input.json"
    rc = subprocess.run([sigs_bin, "layer-one-input", "--poa-input-data", str(parsed), "--write-layer-one-data-to", str(out)],
                        capture_output=True, text=True, timeout=120)
    assert rc.returncode == 0, rc.stderr
    assert out.read_text() == fixture_text("layer_one_input.json")
    assert "Batch contains all input data i.e. there is only 1 batch" in rc.stdout
    # a range of a longer file, short options
    many = sr.parser_output_text(sr.signatures_json(sr.generate(5, seed=3)))
    parsed.write_text(many)
    rc = subprocess.run([sigs_bin, "layer-one-input", "-i", str(parsed), "-o", str(out), "-s", "1", "-e", "4"],
                        capture_output=True, text=True, timeout=120)
    assert rc.returncode == 0, rc.stderr
    assert out.read_text() == sr.layer_one_text(many, 1, 4)
    # the reference's index-range error, and no file
    out.unlink()
    rc = subprocess.run([sigs_bin, "layer-one-input", "-i", str(parsed), "-o", str(out), "-s", "3", "-e", "3"],
                        capture_output=True, text=True, timeout=120)
    assert rc.returncode == 1
    assert "startIndex 3 must be less than endIndex 3" in rc.stderr
    assert not out.exists()
