"""zkpoa_assets_verify and the `zkpoa-audit` executable: the verifier's whole check, pinned on the reference's own files.

The reference commits no run that has csv, proof and verification key together: 1_sigs_1_batches_5_height has the csv and
the layer-three proof but no layer-three vkey, 4_sigs_2_batches_12_height has vkey and proof but no csv. Every check
runs whatever the others found, so both runs pin something: the 1_sigs files under the (4_sigs) key fail only the proof,
the 4_sigs files over the 1_sigs set fail only the root."""
import json
import os
import subprocess

import pytest

import layer_inputs_ref as ref
from conftest import GOLDEN, le
from test_pedersen_decode import compress, decode
from test_poseidon_oracle import REF_ROOT, anon_set

pytestmark = pytest.mark.gpu

CSV = os.path.join(GOLDEN, "ref", "merkle", "anonymity_set_10.csv")
VKEY = os.path.join(GOLDEN, "ref", "layer_three_vkey.json")
RUN_1 = os.path.join(GOLDEN, "ref", "1_sigs_1_batches_5_height__layer_three")
RUN_4 = os.path.join(GOLDEN, "ref", "4_sigs_2_batches_12_height__layer_three")
COMMITMENT_1 = compress(ref.pedersen_commitment(354, 2))     # tests/test_pedersen_decode.py pins this on the fixture


def text(path):
    with open(path) as f:
        return f.read()


def set_bytes(addr, bal):
    return b"".join(le(a) for a in addr), b"".join(le(b) for b in bal)


@pytest.fixture(scope="module")
def audit_bin(zk):
    if not os.path.exists(zk.AUDIT_BIN):
        import __graft_entry__ as entry
        entry.build()
    return zk.AUDIT_BIN


def run(audit_bin, csv_path, run_dir, vkey=VKEY, extra=(), public=None, proof=None):
    return subprocess.run([audit_bin, "--anon-set", str(csv_path), "--vkey", str(vkey), "--public",
                           str(public or os.path.join(run_dir, "public.json")), "--proof",
                           str(proof or os.path.join(run_dir, "proof.json")), *extra], capture_output=True, text=True, timeout=120)


def test_one_sig_run_under_the_other_runs_key_fails_only_the_proof(zk, ctx):
    a, b = set_bytes(*anon_set())
    failed, rep = ctx.assets_verify(a, b, text(VKEY), text(os.path.join(RUN_1, "public.json")), text(os.path.join(RUN_1, "proof.json")))
    assert failed == zk.ASSETS_PROOF
    assert rep == {"root": REF_ROOT, "commitment": COMMITMENT_1, "rows": 10, "duplicate_rows": 0, "first_dup": None,
                   "ascending": True}
    assert sorted(anon_set()[0]) == anon_set()[0]
    # with the commitment the auditor expects: still only the proof; with one bit of it flipped: the commitment too
    failed, _ = ctx.assets_verify(a, b, text(VKEY), text(os.path.join(RUN_1, "public.json")), text(os.path.join(RUN_1, "proof.json")),
                                  expected_commitment=COMMITMENT_1)
    assert failed == zk.ASSETS_PROOF
    flipped = bytes([COMMITMENT_1[0] ^ 1]) + COMMITMENT_1[1:]
    failed, rep = ctx.assets_verify(a, b, text(VKEY), text(os.path.join(RUN_1, "public.json")), text(os.path.join(RUN_1, "proof.json")),
                                    expected_commitment=flipped)
    assert failed == zk.ASSETS_PROOF | zk.ASSETS_COMMITMENT and rep["commitment"] == COMMITMENT_1


def test_four_sig_run_over_the_other_runs_set_fails_only_the_root(zk, ctx):
    a, b = set_bytes(*anon_set())
    public = text(os.path.join(RUN_4, "public.json"))
    failed, rep = ctx.assets_verify(a, b, text(VKEY), public, text(os.path.join(RUN_4, "proof.json")))
    assert failed == zk.ASSETS_ROOT                      # the proof verifies, the commitment is a point
    assert rep["root"] == REF_ROOT != int(json.loads(public)[12])
    assert rep["commitment"] == decode([int(v) for v in json.loads(public)])
    assert zk.groth16_verify(text(VKEY), public, text(os.path.join(RUN_4, "proof.json")))


def test_a_repeated_address_with_another_balance(zk, ctx):
    addr, bal = anon_set()
    addr, bal = addr + [addr[3]], bal + [bal[3] + 10 ** 6]          # row 10 repeats row 3 with an inflated balance
    a, b = set_bytes(addr, bal)
    failed, rep = ctx.assets_verify(a, b, text(VKEY), text(os.path.join(RUN_1, "public.json")), text(os.path.join(RUN_1, "proof.json")))
    assert failed == zk.ASSETS_SET | zk.ASSETS_ROOT | zk.ASSETS_PROOF   # (the proof: the key is the other run's, as above)
    assert (rep["rows"], rep["duplicate_rows"], rep["first_dup"], rep["ascending"]) == (11, 1, (3, 10), False)
    assert rep["root"] != REF_ROOT
    failed, rep = ctx.assets_verify(a, b, text(VKEY), text(os.path.join(RUN_4, "public.json")), text(os.path.join(RUN_4, "proof.json")))
    assert failed == zk.ASSETS_SET | zk.ASSETS_ROOT and rep["first_dup"] == (3, 10)


def test_every_check_runs_on_input_that_fails_them_all(zk, ctx):
    """An empty set, twelve signals that spell no point and a thirteenth that is no root, under a key of another run."""
    public = json.dumps(["0"] * 13)
    failed, rep = ctx.assets_verify(b"", b"", text(VKEY), public, text(os.path.join(RUN_1, "proof.json")))
    assert failed == zk.ASSETS_SET | zk.ASSETS_ROOT | zk.ASSETS_COMMITMENT | zk.ASSETS_PROOF
    assert rep["rows"] == 0 and rep["commitment"] == bytes(32)
    a, b = set_bytes(*anon_set())
    twelve = json.dumps(json.loads(text(os.path.join(RUN_1, "public.json")))[:12])
    failed, rep = ctx.assets_verify(a, b, text(VKEY), twelve, text(os.path.join(RUN_1, "proof.json")))
    assert failed == zk.ASSETS_ROOT | zk.ASSETS_PROOF and rep["root"] == REF_ROOT and rep["commitment"] == COMMITMENT_1


def test_malformed_input_is_an_error_not_a_verdict(zk, ctx):
    a, b = set_bytes(*anon_set())
    good = [text(VKEY), text(os.path.join(RUN_1, "public.json")), text(os.path.join(RUN_1, "proof.json"))]
    for k in range(3):
        args = list(good)
        args[k] = "not json"
        with pytest.raises(zk.ZkpoaError):
            ctx.assets_verify(a, b, *args)
    with pytest.raises(zk.ZkpoaError, match="row 2"):
        ctx.assets_verify(a[:64] + le(ref.R) + a[96:], b, *good)
    with pytest.raises(zk.ZkpoaError, match="balance of row 9"):
        ctx.assets_verify(a, b[:288] + b"\xff" * 32, *good)


def test_executable_verdicts_and_exit_codes(zk, audit_bin, tmp_path):
    rc = run(audit_bin, CSV, RUN_1)
    lines = rc.stdout.splitlines()
    assert rc.returncode == 1 and lines[-1] == "AUDIT FAILED: proof", rc.stdout + rc.stderr
    assert lines[0].startswith("rows: 10") and lines[1] == "duplicates: none"
    assert lines[2].startswith("root: %d " % REF_ROOT) and "as in" in lines[2]
    assert lines[3].startswith("commitment: " + COMMITMENT_1.hex()) and lines[4] == "proof: Invalid proof" and len(lines) == 6
    rc = run(audit_bin, CSV, RUN_4)
    lines = rc.stdout.splitlines()
    assert rc.returncode == 1 and lines[-1] == "AUDIT FAILED: root" and lines[4] == "proof: OK" and "DIFFERS" in lines[2]
    rc = run(audit_bin, CSV, RUN_1, extra=["--commitment", COMMITMENT_1.hex()])
    assert rc.returncode == 1 and rc.stdout.splitlines()[-1] == "AUDIT FAILED: proof" and "as expected" in rc.stdout
    flipped = bytes([COMMITMENT_1[0] ^ 1]) + COMMITMENT_1[1:]
    rc = run(audit_bin, CSV, RUN_1, extra=["--commitment=" + flipped.hex()])
    assert rc.returncode == 1 and rc.stdout.splitlines()[-1] == "AUDIT FAILED: commitment proof" and "DIFFERS from --commitment" in rc.stdout
    # the set with one row repeated under another balance
    rows = text(CSV).splitlines()
    dup = tmp_path / "dup.csv"
    dup.write_text("\n".join(rows + [rows[4].split(",")[0] + ",1000414"]) + "\n")
    rc = run(audit_bin, dup, RUN_4)
    lines = rc.stdout.splitlines()
    assert rc.returncode == 1 and lines[-1] == "AUDIT FAILED: set root"
    assert lines[0] == "rows: 11" and "rows 3 and 10" in lines[1] and rows[4].split(",")[0][-40:].lower() in lines[1]


def test_executable_usage_and_malformed_input(zk, audit_bin, tmp_path):
    """Exit 2 and an empty stdout. (Exit 0 with a verdict needs a set whose root a committed proof names, which the
    reference does not commit; the mask of the C ABI is what AUDIT OK is printed from, and --help is the 0 seen here.)"""
    rc = subprocess.run([audit_bin, "--help"], capture_output=True, text=True, timeout=60)
    assert rc.returncode == 0 and "Usage: zkpoa-audit" in rc.stdout
    rc = subprocess.run([audit_bin, "--anon-set", CSV], capture_output=True, text=True, timeout=60)
    assert rc.returncode == 2 and rc.stdout == "" and "required arguments" in rc.stderr
    rc = subprocess.run([audit_bin, "--bogus"], capture_output=True, text=True, timeout=60)
    assert rc.returncode == 2 and rc.stdout == ""
    junk = tmp_path / "junk.json"
    junk.write_text("this is not JSON")
    for kw in ({"vkey": junk}, {"public": junk}, {"proof": junk}):
        rc = run(audit_bin, CSV, RUN_1, **kw)
        assert rc.returncode == 2 and rc.stdout == "" and rc.stderr.startswith("Error: "), (kw, rc.stdout, rc.stderr)
    rc = run(audit_bin, tmp_path / "missing.csv", RUN_1)
    assert rc.returncode == 2 and rc.stdout == ""
    rc = run(audit_bin, CSV, RUN_1, extra=["--commitment", "abcd"])
    assert rc.returncode == 2 and rc.stdout == "" and "64 hex digits" in rc.stderr
