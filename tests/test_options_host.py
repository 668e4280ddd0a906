"""zk-proof-of-assets_amd/csrc/options.hpp on the CPU: the one table of the ZKPOA_* variables. tools/options_check.cpp
includes the header's own text, g++ compiles it without HIP, and what its typed accessors answer for every row is compared
with a rule written here over the table's own listing (never with the accessors' own idea of a value).
OPTIONS_CHECK_FLAGS adds compiler flags (a sanitizer build).

ZKPOA_DEVICES is a text row: its list parser and its messages stay in select_devices (multi_device.hip.h, HIP code) and
are exercised by tests/test_gpu_prove.py; the other strict messages are compared here byte for byte."""
import collections
import os
import re
import shlex
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "zk-proof-of-assets_amd", "csrc")
Row = collections.namedtuple("Row", "name kind lo hi words dflt strict latched hook own_message meaning")


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("options") / "options_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread"] + shlex.split(os.environ.get("OPTIONS_CHECK_FLAGS", "")) +
                   ["-I", CSRC, os.path.join(ROOT, "tools", "options_check.cpp"), "-o", out], check=True, capture_output=True, text=True)
    return out


def run(check_bin, args, env):
    """stdout lines of `options_check args` in an environment that holds the ZKPOA_* variables of `env` and no others"""
    base = {k: v for k, v in os.environ.items() if not k.startswith("ZKPOA_")}
    rc = subprocess.run([check_bin] + args, env=dict(base, **env), capture_output=True, text=True, timeout=120)
    assert rc.returncode == 0 and rc.stderr == "", (rc.returncode, rc.stderr[-2000:])
    assert rc.stdout.endswith("\n")
    return rc.stdout.split("\n")[:-1]


@pytest.fixture(scope="module")
def rows(check_bin):
    out = []
    for line in run(check_bin, ["list"], {}):
        f = line.split("\t")
        assert len(f) == 11 and f[1] in ("flag", "int", "choice", "text") and f[6] in ("strict", "lenient"), line
        assert f[7] in ("every", "latched") and f[8] in ("knob", "hook") and f[10], line
        out.append(Row(f[0], f[1], int(f[2]), int(f[3]), f[4].split("|") if f[1] == "choice" else None, int(f[5]),
                       f[6] == "strict", f[7] == "latched", f[8] == "hook", None if f[9] == "-" else f[9], f[10]))
    assert len({r.name for r in out}) == len(out) >= 40 and all(r.name.startswith("ZKPOA_") for r in out)
    return out


def bad_message(row, value):
    if row.own_message:
        return row.own_message % value
    assert row.kind == "int"
    return "%s='%s' is not an integer in [%d, %d]" % (row.name, value, row.lo, row.hi)


def want(row, value):
    """The rule, restated: what the typed accessor must answer for `value` (None = unset)."""
    if row.kind == "text":
        return "null" if value is None else "=" + value
    if value is None or value == "":
        return str(row.dflt)
    if row.kind == "flag":
        return "0" if value == "0" else "1"
    if row.kind == "choice" and value in row.words:
        return str(row.words.index(value))
    # strtol's whole-string rule: optional white space, optional sign, decimal digits, nothing after them
    if row.kind == "int" and re.fullmatch(r"[ \t\n\v\f\r]*[+-]?[0-9]+", value) and row.lo <= int(value) <= row.hi:
        return str(int(value))
    return "error: " + bad_message(row, value) if row.strict else str(row.dflt)


def get(check_bin, env, args=("get",)):
    got = collections.OrderedDict(line.split("\t", 1) for line in run(check_bin, list(args), env))
    return got


def test_every_read_goes_through_the_table():
    reads, gone = re.compile(r'getenv\s*\(\s*"ZKPOA_'), re.compile(r"\b(req_getenv|env_long)\b")
    seen = 0
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".h", ".hpp")):
            continue
        seen += 1
        text = open(os.path.join(CSRC, name)).read()
        assert not gone.search(text), name
        assert name == "options.hpp" or not reads.search(text), name
    assert seen > 50
    table = open(os.path.join(CSRC, "options.hpp")).read()
    assert 'getenv(opt_row(id).name)' in table and len(re.findall(r"\bgetenv\s*\(", table)) == 1   # the one read


def test_the_table_is_well_formed(rows):
    by_name = {r.name: r for r in rows}
    for r in rows:
        if r.kind == "flag":
            assert r.dflt in (0, 1)
        if r.kind == "choice":
            assert len(r.words) >= 2 and len(set(r.words)) == len(r.words) and 0 <= r.dflt < len(r.words) and "" not in r.words
        if r.kind == "int":
            assert r.lo <= r.hi < 2 ** 62 and -2 ** 62 < r.lo
        if r.own_message:
            assert r.strict and r.own_message.count("%") == 1 and "%s" in r.own_message and r.name in r.own_message
    strict = {r.name for r in rows if r.strict and r.kind != "text"}
    assert strict == {"ZKPOA_DEVICE", "ZKPOA_SHARD_BLOCK_LOG", "ZKPOA_MULTI_MIN_POWER", "ZKPOA_LANE_WORKSPACE_MAX_MB",
                      "ZKPOA_GPU_LOCK_WAIT_S", "ZKPOA_MERKLE_THREADS"}
    assert by_name["ZKPOA_DEVICES"].kind == "text" and by_name["ZKPOA_DEVICES"].strict
    for name in ("ZKPOA_R", "ZKPOA_S", "ZKPOA_DELTA", "ZKPOA_PHASE1_S", "ZKPOA_PHASE2_S"):   # secrets and test scalars
        assert by_name[name].kind == "text" and by_name[name].hook
    for name in ("ZKPOA_R", "ZKPOA_S", "ZKPOA_KEY_CACHE", "ZKPOA_SELFCHECK", "ZKPOA_OVERLAP", "ZKPOA_NO_DENSITY"):
        assert not by_name[name].latched                                   # tests change these between calls
    for name in ("ZKPOA_SCAN", "ZKPOA_NO_SPARSE", "ZKPOA_NTT_TILE", "ZKPOA_EXCHANGE"):
        assert by_name[name].latched
    # the workspace guard and its self-test: off unless asked for, hooks, and read at every use (tests set them per case)
    guard, clobber = by_name["ZKPOA_WS_GUARD"], by_name["ZKPOA_TEST_WS_CLOBBER"]
    assert (guard.kind, guard.dflt, guard.hook, guard.latched, guard.strict) == ("flag", 0, True, False, False)
    assert (clobber.kind, clobber.dflt, clobber.lo, clobber.hook, clobber.latched, clobber.strict) == ("int", 0, 0, True, False, False)
    assert clobber.hi >= 64 and want(clobber, "1") == "1" and want(clobber, "-1") == "0" and want(guard, "1") == "1"
    assert by_name["ZKPOA_OVERLAP"].dflt == 1 and by_name["ZKPOA_UPLOAD_AFFINITY"].words == ["gpu", "off"]
    assert by_name["ZKPOA_DETACH_EXIT"].words == ["auto", "0", "always"]
    # the values that documents, tests, tools and bench.py use keep their meaning
    assert want(by_name["ZKPOA_SCAN"], "3") == "1" and want(by_name["ZKPOA_SELFCHECK"], "all") == "3"
    assert want(by_name["ZKPOA_PRECOMP"], "eager") == "3" and want(by_name["ZKPOA_EXCHANGE"], "copy") == "1"
    assert want(by_name["ZKPOA_JSON"], "snarkjs") == "1" and want(by_name["ZKPOA_NTT_TILE"], "10") == "10"


def test_every_row_reads_every_value_by_the_rule(check_bin, rows):
    names = [r.name for r in rows]
    cases = [{}]                                                          # unset
    for text in ("", "0", "1", "12abc", " 5", "+5", "-0", "99999999999999999999", "5 ", "0x10", "true", "yes", "1|3"):
        cases.append({r.name: text for r in rows})
    for pick in (lambda r: r.lo, lambda r: r.hi, lambda r: r.lo - 1, lambda r: r.hi + 1):
        cases.append({r.name: str(pick(r)) for r in rows if r.kind == "int"})
    for k in range(max(len(r.words) for r in rows if r.kind == "choice")):
        cases.append({r.name: r.words[k] for r in rows if r.kind == "choice" and k < len(r.words)})
    cases.append({r.name: "no-such-word" for r in rows if r.kind == "choice"})
    errors = 0
    for env in cases:
        got = get(check_bin, env)
        assert list(got) == names
        for r in rows:
            value = env.get(r.name)
            assert got[r.name] == want(r, value), (r.name, value)
            if got[r.name].startswith("error: "):
                errors += 1
                assert r.strict and r.name in got[r.name] and value in got[r.name]
    assert errors > 40
    # the deliberate rule for flags: unset, empty or "0" is off; anything else is on
    by_name = {r.name: r for r in rows}
    for name, value, on in (("ZKPOA_VERBOSE", "0", "0"), ("ZKPOA_VERBOSE", "", "0"), ("ZKPOA_NO_SPARSE", "true", "1"),
                            ("ZKPOA_SERVER_KILL_WEDGED", "yes", "1"), ("ZKPOA_OVERLAP", "0", "0"), ("ZKPOA_OVERLAP", "1", "1")):
        assert by_name[name].kind == "flag" and get(check_bin, {name: value})[name] == on


def test_strict_messages_are_the_parent_commits(check_bin):
    """the texts env_long, zkpoa_context_create, device_from_env and merkle-tree's reader produced before the table"""
    for name, value, text in (
            ("ZKPOA_SHARD_BLOCK_LOG", "25", "ZKPOA_SHARD_BLOCK_LOG='25' is not an integer in [0, 24]"),
            ("ZKPOA_MULTI_MIN_POWER", "x", "ZKPOA_MULTI_MIN_POWER='x' is not an integer in [0, 64]"),
            ("ZKPOA_GPU_LOCK_WAIT_S", "-1", "ZKPOA_GPU_LOCK_WAIT_S='-1' is not an integer in [0, 86400]"),
            ("ZKPOA_LANE_WORKSPACE_MAX_MB", "lots", "ZKPOA_LANE_WORKSPACE_MAX_MB='lots' is not a number of MiB"),
            ("ZKPOA_LANE_WORKSPACE_MAX_MB", "1048577", "ZKPOA_LANE_WORKSPACE_MAX_MB='1048577' is not a number of MiB"),
            ("ZKPOA_DEVICE", "7x", "ZKPOA_DEVICE: not a device index: 7x"),
            ("ZKPOA_DEVICE", "1024", "ZKPOA_DEVICE: not a device index: 1024"),
            ("ZKPOA_MERKLE_THREADS", "0", "ZKPOA_MERKLE_THREADS must be 1..256, not '0'")):
        assert get(check_bin, {name: value})[name] == "error: " + text
    # the prover holds ZKPOA_DEVICE to the device count it finds
    for value, count, text in (("7x", 8, "ZKPOA_DEVICE='7x' is not an integer in [0, 7]"),
                               ("-1", 1, "ZKPOA_DEVICE='-1' is not an integer in [0, 0]"),
                               ("99", 8, "ZKPOA_DEVICE='99' is not an integer in [0, 7]")):
        assert run(check_bin, ["device", "0", str(count - 1)], {"ZKPOA_DEVICE": value}) == ["error: " + text]
    assert run(check_bin, ["device", "0", "7"], {"ZKPOA_DEVICE": "7"}) == ["7"]
    assert run(check_bin, ["device", "0", "7"], {}) == ["0"]


def test_latched_rows_keep_their_first_value(check_bin, rows):
    first = {r.name: r.words[-1] if r.kind == "choice" else str(r.hi) for r in rows if r.kind != "text"}
    got = get(check_bin, first, ("get-twice", "0"))
    for r in rows:
        if r.kind != "text":
            assert got[r.name] == want(r, first[r.name] if r.latched else "0"), r.name
            assert not r.latched or want(r, first[r.name]) != want(r, "0")          # the case can tell the two apart


def test_overlay_is_per_thread_and_wins_over_the_environment(check_bin):
    env = {"ZKPOA_R": "11", "ZKPOA_S": "22", "ZKPOA_JSON": "snarkjs", "ZKPOA_VERBOSE": "1", "ZKPOA_KEY_CACHE": "5"}
    from_env = "R =11 S =22 JSON 1 VERBOSE 1 KEY_CACHE 5"
    overlaid = "R =7 S null JSON 0 VERBOSE 0 KEY_CACHE 5"   # a set field wins, an empty one reads as unset; other rows: the environment
    assert run(check_bin, ["overlay"], env) == ["second " + from_env, "task " + overlaid, "first " + overlaid, "cleared " + from_env]
    assert run(check_bin, ["overlay"], {}) == ["second R null S null JSON 0 VERBOSE 0 KEY_CACHE 2",
                                               "task R =7 S null JSON 0 VERBOSE 0 KEY_CACHE 2",
                                               "first R =7 S null JSON 0 VERBOSE 0 KEY_CACHE 2",
                                               "cleared R null S null JSON 0 VERBOSE 0 KEY_CACHE 2"]


def test_vlog_follows_the_verbose_row(check_bin):
    base = {k: v for k, v in os.environ.items() if not k.startswith("ZKPOA_")}
    for value, text in ((None, ""), ("", ""), ("0", ""), ("1", "check 7\n"), ("yes", "check 7\n")):
        env = base if value is None else dict(base, ZKPOA_VERBOSE=value)
        rc = subprocess.run([check_bin, "vlog"], env=env, capture_output=True, text=True, timeout=60)
        assert (rc.returncode, rc.stdout, rc.stderr) == (0, "", text), value


def test_integration_md_lists_the_table(rows):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    begin, end = "<!-- options table: begin -->", "<!-- options table: end -->"
    assert text.count(begin) == 1 and text.count(end) == 1
    listed = {}
    for line in text.split(begin)[1].split(end)[0].strip().split("\n")[2:]:
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        assert len(cells) == 5 and re.fullmatch(r"`ZKPOA_[A-Z0-9_]+`", cells[0]) and cells[0] not in listed, line
        listed[cells[0].strip("`")] = cells
    assert set(listed) == {r.name for r in rows}
    for r in rows:
        _, kind, dflt, policy, meaning = listed[r.name]
        want_default = {"flag": lambda: "on" if r.dflt else "off", "int": lambda: str(r.dflt), "choice": lambda: r.words[r.dflt],
                        "text": lambda: "unset"}[r.kind]()
        assert dflt.strip("`") == want_default, r.name
        assert kind.startswith(r.kind) and policy.startswith("strict" if r.strict else "lenient"), r.name
        assert ("latched" in policy) == r.latched and meaning.startswith("(test hook)") == r.hook, r.name
