"""zk-proof-of-assets_amd/csrc/host_text.hpp on the CPU: tools/host_text_check.cpp includes the header's own text (and
host_files.hpp, and mini_json.hpp for the nesting cap the two JSON readers share), g++ compiles it without HIP, and what
it answers is compared with Python's own int and json. HOST_TEXT_CHECK_FLAGS adds compiler flags (a sanitizer build)."""
import json
import os
import random
import shlex
import subprocess

import pytest

import secp_ref as sr
from conftest import ROOT

N_RANDOM = 10000
DIGITS = set("0123456789")
HEX_DIGITS = set("0123456789abcdefABCDEF")


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_text") / "host_text_check")
    subprocess.run(["g++", "-O2", "-std=c++17"] + shlex.split(os.environ.get("HOST_TEXT_CHECK_FLAGS", "")) +
                   ["-I", os.path.join(ROOT, "zk-proof-of-assets_amd", "csrc"),
                    os.path.join(ROOT, "tools", "host_text_check.cpp"), "-o", out], check=True, capture_output=True, text=True)
    return out


def lines(check_bin, op, texts):
    assert not any("\n" in t for t in texts)
    rc = subprocess.run([check_bin] + op.split(), input="".join(t + "\n" for t in texts), capture_output=True, text=True,
                        timeout=300)
    assert rc.returncode == 0, rc.stderr
    got = rc.stdout.split("\n")
    assert got[-1] == "" and len(got) == len(texts) + 1
    return got[:-1]


def document(check_bin, op, text):
    """(exit status, the lines of stdout); a run that ends on a signal has a negative status and fails here"""
    rc = subprocess.run([check_bin, op], input=text, capture_output=True, text=True, timeout=300)
    assert rc.returncode in (0, 1), (rc.returncode, rc.stderr[-2000:])
    assert (rc.stdout == "" or rc.stdout.endswith("\n")) and rc.stderr == ""
    out = rc.stdout.split("\n")[:-1]
    if rc.returncode == 1:
        assert len(out) == 1 and out[0].startswith("error: ")
    return rc.returncode, out


def want_dec(t):
    return str(int(t)) if t and set(t) <= DIGITS and int(t) < 1 << 256 else "!"


def want_hex(t):
    return str(int(t, 16)) if t and set(t) <= HEX_DIGITS and int(t, 16) < 1 << 256 else "!"


def want_num(t):
    return want_hex(t[2:]) if t[:2] in ("0x", "0X") else want_dec(t)


def random_values(rng, count):
    """bit length uniform over 0..256"""
    out = []
    for _ in range(count):
        bits = rng.randrange(257)
        out.append(rng.getrandbits(bits) | 1 << (bits - 1) if bits else 0)
    return out


# ---- 256-bit integers ---------------------------------------------------------------------------------------------------
def test_decimal_parse_and_print(check_bin):
    values = [0, 1, 2 ** 64 - 1, 2 ** 64, 2 ** 128 - 1, 2 ** 128 + 1, 2 ** 256 - 1]
    for chunk in (19, 38, 57):                                          # the borders of the 19-digit steps
        values += [10 ** chunk - 1, 10 ** chunk, 10 ** chunk + 1]
    accepted = [str(v) for v in values] + ["0" * 100 + "1234567890123456789012", "0" * 100, "00"]
    refused = [str(2 ** 256), str(2 ** 256 + 1), str(10 ** 78 - 1), "1" + "0" * 78, "", "-1", "+1", "12 34", " 1", "1 ", "1\t",
               "12a4", "a", "0x10", "1" * 200, "0" * 100 + str(2 ** 256)]
    assert len(refused[3]) == 79
    for t in accepted:
        assert want_dec(t) != "!", t
    for t in refused:
        assert want_dec(t) == "!", t
    texts = accepted + refused + [str(v) for v in random_values(random.Random(256), N_RANDOM)]
    got = lines(check_bin, "dec", texts)
    assert got == [want_dec(t) for t in texts]
    assert lines(check_bin, "dec", got[:len(accepted)]) == got[:len(accepted)]      # what is printed parses to itself


def test_hex_and_either_form(check_bin):
    rng = random.Random(16)
    values = [0, 1, 0xabcdef, 2 ** 64, 2 ** 256 - 1] + random_values(rng, 1000)
    texts = ["%x" % v for v in values] + ["%X" % v for v in values] + ["aBcDeF", "f" * 64, "0" + "f" * 64, "0" * 40 + "1"]
    texts += ["1" + "0" * 64, "f" * 65, "", "g", "12g4", "0x12", " 1", "1 ", "-1"]
    got = lines(check_bin, "hex", texts)
    assert got == [want_hex(t) for t in texts]
    assert got[len(texts) - 9:] == ["!"] * 9 and "!" not in got[:len(texts) - 9]
    both = ["0x%x" % v for v in values] + ["0X%X" % v for v in values] + [str(v) for v in values]
    both += ["0x", "0X", "x", "0x12g", "00x1", "1x2", "0x1,", "0x" + "f" * 64, "0x1" + "0" * 64, str(2 ** 256), "12a", ""]
    got = lines(check_bin, "num", both)
    assert got == [want_num(t) for t in both]
    assert got[3 * len(values):] == ["!"] * 7 + [str(2 ** 256 - 1)] + ["!"] * 4


def test_fixed_width_hex_bytes(check_bin):
    rng = random.Random(20)
    good = ["0x" + bytes(rng.randrange(256) for _ in range(20)).hex() for _ in range(50)] + ["0x" + "aB" * 20]
    bad = ["0x" + "ab" * 19, "0x" + "ab" * 21, "0x" + "ab" * 19 + "a", "0X" + "ab" * 20, "ab" * 21, "0x" + "ab" * 19 + "ag", ""]
    got = lines(check_bin, "hexbytes 20", good + bad)
    assert got == [t[2:].lower() for t in good] + ["!"] * len(bad)


def test_byte_order(check_bin):
    rng = random.Random(32)
    raw = [bytes(32), bytes([1] + [0] * 31), bytes([0] * 31 + [1]), bytes(range(1, 33)), b"\xff" * 32]
    raw += [bytes(rng.randrange(256) for _ in range(32)) for _ in range(1000)]
    texts = ["0x" + b.hex() for b in raw]
    assert lines(check_bin, "be", texts) == [str(int.from_bytes(b, "big")) for b in raw]
    assert lines(check_bin, "le", texts) == [str(int.from_bytes(b, "little")) for b in raw]


# ---- the pull parser ----------------------------------------------------------------------------------------------------
def bigints(value):
    """what the tool's walk prints"""
    out = []
    if isinstance(value, dict):
        for k, v in value.items():
            if k == "__bigint__":
                out.append(str(v))
            elif not k.startswith("extra"):
                out += bigints(v)
    elif isinstance(value, list):
        for v in value:
            out += bigints(v)
    return out


@pytest.fixture(scope="module")
def parsed_documents():
    entries = sr.generate(50, seed=50)
    return [json.loads(sr.parser_output_text(sr.signatures_json(entries[:n]), known=entries[:n])) for n in (0, 1, 50)]


def test_pull_parser_finds_the_bigints(check_bin, parsed_documents):
    for doc in parsed_documents:
        n = len(doc["accountAttestations"])
        assert len(bigints(doc)) == 7 * n
        for d in (doc, sr.with_unknown_members(doc), sr.with_unknown_members(doc, bare=n - 1)):
            want = bigints(d)
            assert len(want) == 7 * n                                   # none of those under an "extra" key
            assert json.loads(json.dumps(d)) == d
            for indent in (None, 2):
                assert document(check_bin, "bigints", json.dumps(d, indent=indent)) == (0, want)
    # as a string and as a bare number
    assert document(check_bin, "bigints", '[{"__bigint__": "12"}, {"__bigint__": 12}, {"__bigint__":-1.5e3}]') == (0, ["12", "12", "-1.5e3"])


def test_every_truncation_is_an_error(check_bin):
    small = {"accountAttestations": [{"signature": {"r": {"__bigint__": "11"}},
                                       "accountData": {"address": {"__bigint__": "123"}, "balance": {"__bigint__": "45"}}}]}
    text = json.dumps(sr.with_unknown_members(small), separators=(",", ":"))
    assert 300 < len(text) < 1000
    assert document(check_bin, "bigints", text) == (0, ["123", "45", "11"])
    refused = 0
    for cut in range(len(text)):
        status, out = document(check_bin, "bigints", text[:cut])
        assert status == 1, (cut, out)
        refused += 1
    assert refused == len(text)


def test_nesting_cap_is_one_for_both_readers(check_bin):
    depth = int(subprocess.run([check_bin, "depth"], capture_output=True, text=True, check=True).stdout)
    assert depth == 32
    for op in ("bigints", "tree"):
        for text in ('{"extra": ' + "[" * 100000, "[" * 100000, '{"a":' * 100000):
            status, out = document(check_bin, op, text)
            assert status == 1 and "nesting too deep" in out[0]

    def nested(opener, closer, levels, inner=""):
        return opener * levels + inner + closer * levels
    # objects and arrays nested exactly `depth` deep are read by both readers, one more by neither
    cases = [(nested("[", "]", depth), True, True), (nested("[", "]", depth + 1), False, False),
             (nested('{"a":', "}", depth - 1, "[]"), True, True), (nested('{"a":', "}", depth, "[]"), False, False),
             ('{"extra": ' + nested("[", "]", depth - 1) + "}", True, True), ('{"extra": ' + nested("[", "]", depth) + "}", False, False),
             ('{"extra": ' + nested('{"a":', "}", depth - 1, "1") + "}", True, False),
             ('{"extra": ' + nested('{"a":', "}", depth, "1") + "}", False, False),
             # the tree reader counts a scalar or a key as one more level, as it always did; the pull parser does not
             (nested("[", "]", depth - 1, "1"), True, True), (nested("[", "]", depth, "1"), True, False),
             (nested('{"a":', "}", depth - 1, '"s"'), True, True), (nested('{"a":', "}", depth, '"s"'), True, False)]
    for text, pulled, tree in cases:
        for op, accepted in (("bigints", pulled), ("tree", tree)):
            status, out = document(check_bin, op, text)
            assert (status == 0) == accepted, (op, text[:20], out)
            assert accepted or "nesting too deep" in out[0]
