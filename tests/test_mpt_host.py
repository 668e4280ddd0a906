"""csrc/mpt.hip.h on the CPU: the word-wise Keccak absorb, the walk and the account parser are host-and-device functions,
and tools/mpt_host_check.hip runs them over the proofs of tests/mpt_cases.py under AddressSanitizer and
UndefinedBehaviorSanitizer -- a stand-alone program with its own main, nothing loaded into Python, no GPU. Every status,
`where` and value span must be what tests/mpt_ref.py says; every node's word-wise digest must equal the byte-wise one."""
import os
import struct
import subprocess

import pytest

import mpt_cases as cases
import mpt_ref as m
from conftest import ROOT


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mpt") / "mpt_host_check")
    subprocess.run(["hipcc", "-O1", "-g", "-std=c++17", "--offload-host-only", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "zk-proof-of-assets_amd", "csrc"),
                    os.path.join(ROOT, "tools", "mpt_host_check.hip"), "-o", out], check=True, capture_output=True, text=True)
    return out


def packed(g, key_kind=0, account=0):
    blob, offsets, lengths, first = m.layout(g["proofs"])
    n, t = len(g["keys"]), len(offsets)
    return (struct.pack("<5Q", n, t, len(blob), key_kind, account) + g["root"] + b"".join(g["keys"]) +
            struct.pack("<%dQ" % (n + 1), *first) + struct.pack("<%dQ" % t, *offsets) + struct.pack("<%dI" % t, *lengths) + blob)


def run(check_bin, tmp_path, g, **kw):
    path = tmp_path / "case.bin"
    path.write_bytes(packed(g, **kw))
    rc = subprocess.run([check_bin, str(path)], capture_output=True, text=True, timeout=120)
    assert rc.returncode == 0 and rc.stderr == "", (g["name"], rc.stdout[-500:], rc.stderr[-2000:])
    return [line.split() for line in rc.stdout.splitlines()]


def test_the_walk_gives_what_the_restatement_gives(check_bin, tmp_path):
    groups = list(cases.raw_groups()) + [cases.keccak_edges_group(), cases.lanes_group(65)] + cases.mutation_groups()
    seen = set()
    for g in groups:
        want = cases.expected(g)
        got = [tuple(int(v) for v in line) for line in run(check_bin, tmp_path, g)]
        assert got == want, g["name"]
        seen |= {w[0] for w in want}
    assert seen == {m.PRESENT, m.ABSENT, m.NO_NODES, m.HASH, m.RLP, m.CHILD, m.SHORT, m.LONG, m.HEX_PREFIX}


def test_accounts(check_bin, tmp_path):
    g, want = cases.account_group()
    got = run(check_bin, tmp_path, g, key_kind=1, account=1)
    for line, w in zip(got, want):
        assert (int(line[4]), int(line[5]), line[6], line[7], line[8]) == w
