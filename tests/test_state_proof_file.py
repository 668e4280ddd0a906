"""csrc/state_proof_file.hpp, the reader of the proofs file, on the CPU and under a sanitizer: tools/state_proof_file_check.cpp
is a stand-alone program (g++ -fsanitize=address,undefined, its own main; nothing is loaded into Python, nothing touches
the GPU). Good files must give exactly the addresses and nodes that tests/mpt_ref.py wrote, whatever the slab limits; bad
files a clean error that names the line; neither a sanitizer report."""
import json
import os
import random
import subprocess

import pytest

import mpt_ref as m
from conftest import ROOT
from secp_ref import keccak256

CSRC = os.path.join(ROOT, "zk-proof-of-assets_amd", "csrc")


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("spf") / "state_proof_file_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, os.path.join(ROOT, "tools", "state_proof_file_check.cpp"), "-o", out], check=True,
                   capture_output=True, text=True)
    return out


def run(check_bin, path, items=1 << 16, text=1 << 28):
    rc = subprocess.run([check_bin, str(path), str(items), str(text)], capture_output=True, text=True, timeout=120)
    assert rc.stderr == "" and rc.returncode in (0, 1), rc.stderr[-3000:]           # a sanitizer report would be on stderr
    assert (rc.returncode == 1) == rc.stdout.startswith("error: ")
    return rc.returncode, rc.stdout


@pytest.fixture(scope="module")
def proofs():
    rng = random.Random(11)
    accounts = {keccak256(b"holder %d" % i)[:20]: m.account(i, rng.randrange(1 << 90)) for i in range(40)}
    trie = m.account_trie(accounts)
    return [(a, trie.prove(keccak256(a))) for a in accounts] + [(bytes(20), []), (b"\xAB" * 20, [b"", b"\x80", b"x" * 9])]


def want_text(proofs):
    return "".join("%s %s\n" % (a.hex(), ",".join(n.hex() for n in p)) for a, p in proofs)


def test_good_files_in_any_slabs(check_bin, proofs, tmp_path):
    lines = [m.proof_json(a, p, envelope=i % 3 == 1, balance=i) for i, (a, p) in enumerate(proofs)]
    lines[2] = lines[2].replace("0x", "0X", 1)                                    # the address's prefix in capitals ...
    lines[3] = json.dumps(dict(json.loads(lines[3]), address="0x" + proofs[3][0].hex().upper()))     # ... and its digits
    path = tmp_path / "good.jsonl"
    path.write_text("\n\n  \n" + "\n".join(l + ("\r" if i % 5 == 0 else "") + ("\n" if i % 7 == 0 else "")
                                          for i, l in enumerate(lines)))          # blank lines, CR LF, no final newline
    for items, text in ((1 << 16, 1 << 28), (1, 1 << 28), (7, 1 << 28), (1 << 16, 1), (1 << 16, 5000)):
        assert run(check_bin, path, items, text) == (0, want_text(proofs)), (items, text)
    rc = subprocess.run([check_bin, str(path), "65536", "268435456"], capture_output=True, text=True, timeout=120,
                        env=dict(os.environ, ZKPOA_SETUP_THREADS="5"))
    assert (rc.returncode, rc.stdout, rc.stderr) == (0, want_text(proofs), "")


def test_an_empty_file_and_a_blank_one(check_bin, tmp_path):
    for text in ("", "\n\n \r\n"):
        path = tmp_path / "empty.jsonl"
        path.write_text(text)
        assert run(check_bin, path) == (0, "")


def test_bad_files_are_clean_errors_that_name_the_line(check_bin, proofs, tmp_path):
    a, p = proofs[0]
    good = m.proof_json(a, p)
    obj = json.loads(good)
    bad = {
        "truncated": good[:len(good) // 2],
        "truncated inside the envelope": m.proof_json(a, p, envelope=True)[:-1],
        "odd-length hex": json.dumps(dict(obj, accountProof=[obj["accountProof"][0] + "a"])),
        "no hex digit": json.dumps(dict(obj, accountProof=["0xzz"])),
        "no prefix": json.dumps(dict(obj, accountProof=["abcd"])),
        "an envelope without result": json.dumps({"jsonrpc": "2.0", "id": 1, "error": {"code": -32000, "message": "missing trie node"}}),
        "result is null": json.dumps({"jsonrpc": "2.0", "id": 1, "result": None}),
        "no address": json.dumps({k: v for k, v in obj.items() if k != "address"}),
        "no proof": json.dumps({k: v for k, v in obj.items() if k != "accountProof"}),
        "a short address": json.dumps(dict(obj, address="0x1234")),
        "an address that is a number": json.dumps(dict(obj, address=5)),
        "a proof that is no array": json.dumps(dict(obj, accountProof="0x80")),
        "a node that is a number": json.dumps(dict(obj, accountProof=[1, 2])),
        "text after the object": good + " x",
        "an array": "[" + good + "]",
        "nesting too deep": json.dumps(dict(obj, storageProof=eval("[" * 40 + "]" * 40))),
    }
    for name, line in bad.items():
        path = tmp_path / "bad.jsonl"
        path.write_text(good + "\n\n" + line + "\n" + good + "\n")
        rc, out = run(check_bin, path)
        assert rc == 1 and "line 3: " in out, (name, out)
        rc, out = run(check_bin, path, 1, 1)                                      # the slab before it is read first: still line 3
        assert rc == 1 and "line 3: " in out, (name, out)


def test_a_huge_array(check_bin, tmp_path):
    """100000 small nodes in one proof, and one node of a megabyte: read; a node above 2^20 bytes: refused."""
    nodes = ["0x%04x" % (i & 0xffff) for i in range(100000)]
    path = tmp_path / "huge.jsonl"
    path.write_text(json.dumps({"address": "0x" + "11" * 20, "accountProof": nodes}) + "\n")
    rc, out = run(check_bin, path)
    assert rc == 0 and out == "%s %s\n" % ("11" * 20, ",".join(n[2:] for n in nodes))
    path.write_text(json.dumps({"address": "0x" + "11" * 20, "accountProof": ["0x" + "ab" * (1 << 20)]}) + "\n")
    assert run(check_bin, path)[0] == 0
    path.write_text(json.dumps({"address": "0x" + "11" * 20, "accountProof": ["0x" + "ab" * ((1 << 20) + 1)]}) + "\n")
    rc, out = run(check_bin, path)
    assert rc == 1 and "line 1: " in out and "2^20" in out
