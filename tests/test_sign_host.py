"""The signing path of zk-proof-of-assets_amd/csrc/secp256k1.hip.h and csrc/sha256.hip.h on the CPU:
tools/sign_host_check.cpp includes the headers' own text, hipcc compiles it for the host alone with AddressSanitizer and
UndefinedBehaviorSanitizer, and every answer is compared with tests/sign_ref.py. A stand-alone program: nothing is loaded
into Python, and no GPU is involved. Any sanitizer report ends the program with a non-zero status."""
import hashlib
import os
import random
import shutil
import subprocess

import pytest

import secp_ref as sr
import sign_ref as sg
from conftest import ROOT

N = sr.N
h32 = lambda v: "%064x" % v


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """One build and one run: name -> answer line, for every case of this file."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc to compile the host check with")
    exe = str(tmp_path_factory.mktemp("sign_host") / "sign_host_check")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-O0", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "zk-proof-of-assets_amd", "csrc"),
                           os.path.join(ROOT, "tools", "sign_host_check.cpp"), "-o", exe])
    lines = []
    for name, (op, args) in CASES.items():
        lines.append(" ".join([op] + [a if isinstance(a, str) else (str(a) if op in ("nonce", "key") and i == len(args) - 1 else h32(a))
                                      for i, a in enumerate(args)]))
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr == ""
    out = run.stdout.splitlines()
    assert len(out) == len(CASES)
    return dict(zip(CASES, out))


def build_cases():
    rng = random.Random(7)
    cases = {}
    for d in sg.edge_keys():
        cases["pub %x" % d] = ("pub", (d,))
        for z in sg.edge_hashes(rng):
            cases["sign %x %x" % (d, z)] = ("sign", (d, z))
    for d in sg.INVALID_KEYS:
        cases["pub %x" % d] = ("pub", (d,))
        cases["sign %x 5" % d] = ("sign", (d, 5))
    for d in (1, N - 1, rng.randrange(1, N)):
        for z in (0, N - 1, N, N + 1, (1 << 256) - 1, rng.getrandbits(256)):
            for skip in (0, 1, 2):
                cases["nonce %x %x %d" % (d, z, skip)] = ("nonce", (d, z, skip))
    for length in (0, 1, 55, 56, 63, 64, 65, 119, 120, 128):
        msg = bytes(rng.randrange(256) for _ in range(length))
        cases["sha %d" % length] = ("sha", (msg.hex() or "-",))
    for seed in (b"", b"seed", bytes(range(60))):
        for i in (0, 1, 255, 256, (1 << 40) + 3):
            cases["key %s %d" % (seed.hex(), i)] = ("key", (seed.hex() or "-", i))
    cases["sign vector"] = ("sign", (1, int.from_bytes(hashlib.sha256(b"Satoshi Nakamoto").digest(), "big")))
    return cases


CASES = build_cases()


def test_signatures(answers):
    checked = 0
    for name, (op, args) in CASES.items():
        if op != "sign":
            continue
        g = sg.sign(*args)
        want = "%d %s %s %d %s %s %s" % (g["status"], h32(g["r"]), h32(g["s"]), g["v"], h32(g["pub"][0]), h32(g["pub"][1]), g["address"].hex())
        assert answers[name] == want, name
        checked += 1
    assert checked == 4 * len(sg.edge_keys()) + len(sg.INVALID_KEYS) + 1 and len(sg.edge_keys()) == 21
    assert answers["sign vector"].split()[1] == "934b1ea10a4b3c1757e2b0c017d0b6143ce3c9a7e6a4a49860d7a6ab210ee3d8"


def test_public_keys(answers):
    for name, (op, args) in CASES.items():
        if op == "pub":
            g = sg.public_key(*args)
            assert answers[name] == "%d %s %s %s" % (g["status"], h32(g["pub"][0]), h32(g["pub"][1]), g["address"].hex()), name


def test_nonces(answers):
    for name, (op, args) in CASES.items():
        if op == "nonce":
            assert answers[name] == h32(sg.nonce(*args)), name


def test_sha256_and_derived_keys(answers):
    for name, (op, args) in CASES.items():
        if op == "sha":
            msg = b"" if args[0] == "-" else bytes.fromhex(args[0])
            assert answers[name] == hashlib.sha256(msg).hexdigest(), name
        elif op == "key":
            seed = b"" if args[0] == "-" else bytes.fromhex(args[0])
            assert answers[name] == h32(sg.derive_key(seed, args[1])), name
