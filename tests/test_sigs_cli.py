"""The command line of `ecdsa-sigs-parser` where no other test pins it, without a GPU: what the parser mode and
layer-one-input answer to help, to no arguments and to bad ones (they do not answer as the five later modes do), the
`--name=value` spelling, and layer-one-input's output for an empty batch and for slices of a five-entry file."""
import json

import pytest

import secp_ref as sr
from test_layer_inputs import run, sigs_bin  # noqa: F401  (sigs_bin is a fixture)
from test_secp_ref import fixture_text

FIELDS = ("r", "s", "rprime", "pubkey", "msghash")


def stderr_of(sigs_bin, argv, status):
    rc = run([sigs_bin] + argv)
    assert rc.returncode == status, (argv, rc.returncode, rc.stderr)
    return rc.stderr


@pytest.mark.parametrize("argv", [["--help"], ["layer-one-input", "-h"], ["-h"], ["layer-one-input", "--help", "--frobnicate"]])
def test_help_is_the_usage_on_stdout(sigs_bin, argv):
    rc = run([sigs_bin] + argv)
    assert rc.returncode == 0 and rc.stderr == ""
    assert rc.stdout.startswith("Usage: ecdsa-sigs-parser --signatures <in.json> --output-path <out.json>\n")
    assert rc.stdout.endswith("--blindingFactor <decimal or 0x-hex>\n") and len(rc.stdout.splitlines()) == 16


def test_missing_files_are_exit_two_with_one_line(sigs_bin):
    assert stderr_of(sigs_bin, [], 2) == "error: --signatures <FILE> and --output-path <FILE> are required\n"
    assert stderr_of(sigs_bin, ["--signatures", "x"], 2) == "error: --signatures <FILE> and --output-path <FILE> are required\n"
    want = "error: layer-one-input needs --poa-input-data <FILE> and --write-layer-one-data-to <FILE>\n"
    assert stderr_of(sigs_bin, ["layer-one-input"], 2) == want
    assert stderr_of(sigs_bin, ["layer-one-input", "-o", "x", "-s", "1"], 2) == want


def test_bad_arguments_are_exit_one_with_one_line(sigs_bin):
    assert stderr_of(sigs_bin, ["--frobnicate", "1"], 1) == "Error: unknown argument --frobnicate\n"
    assert stderr_of(sigs_bin, ["-o", "x", "--signatures"], 1) == "Error: option --signatures needs a value\n"
    assert stderr_of(sigs_bin, ["layer-one-input", "-e"], 1) == "Error: option -e needs a value\n"
    # the parser mode has no index options, and layer-one-input does not know --signatures
    assert stderr_of(sigs_bin, ["-e", "1"], 1) == "Error: unknown argument -e\n"
    assert stderr_of(sigs_bin, ["layer-one-input", "--signatures", "x"], 1) == "Error: unknown argument --signatures\n"
    assert stderr_of(sigs_bin, ["layer-one-input", "-i", "a", "-o", "b", "-s", "x"], 1) == "Error: --account-start-index is not an integer\n"
    assert stderr_of(sigs_bin, ["layer-one-input", "-i", "a", "-o", "b", "--account-end-index=4x"], 1) == \
        "Error: --account-end-index is not an integer\n"


def test_sign_has_no_help_option(sigs_bin):
    err = stderr_of(sigs_bin, ["sign", "-h"], 2)
    assert err.startswith("error: unknown argument -h\nUsage: ecdsa-sigs-parser --signatures") and len(err.splitlines()) == 17


def test_the_equals_form_is_read(sigs_bin, tmp_path):
    missing, out = tmp_path / "missing.json", tmp_path / "out.json"
    rc = run([sigs_bin, "layer-one-input", "--poa-input-data=%s" % missing, "--write-layer-one-data-to=%s" % out])
    assert rc.returncode == 1 and rc.stderr == "Error: cannot open %s\n" % missing
    assert "- System input: %s\n" % missing in rc.stdout and "Path to write processed data to: %s\n" % out in rc.stdout
    assert list(tmp_path.iterdir()) == []


def layer_one(sigs_bin, tmp_path, parsed_text, extra):
    parsed, out = tmp_path / "parsed.json", tmp_path / "layer_one_input.json"
    parsed.write_text(parsed_text)
    rc = run([sigs_bin, "layer-one-input", "-i", parsed, "-o", out] + extra)
    assert rc.returncode == 0, rc.stderr
    return out.read_text(), rc.stdout


def test_layer_one_input_of_an_empty_batch(sigs_bin, tmp_path):
    """A slice past the end of the one-signature file: five empty arrays, each written as []."""
    text, _ = layer_one(sigs_bin, tmp_path, sr.parser_output_text(fixture_text("signatures_1.json")), ["-s", "5", "-e", "100"])
    assert text == '{\n  "r": [],\n  "s": [],\n  "rprime": [],\n  "pubkey": [],\n  "msghash": []\n}'


def five_entries():
    big = lambda v: {"__bigint__": str(v)}
    atts = [{"signature": {"r": big(3 ** (40 + i)), "s": big(5 ** (30 + i)), "r_prime": big((1 << 256) - 1 - i),
                           "pubkey": {"x": big(7 ** (60 + i)), "y": big(i)},
                           "msghash": {"__uint8array__": [(37 * i + k) % 256 for k in range(32)]}},
             "accountData": {"address": big(1000 + i), "balance": big(i)}} for i in range(5)]
    return json.dumps({"accountAttestations": atts}, indent=2)


# -e -1 is "to the end" (the reference's one special case), so -s -3 -e -1 is the last three entries
@pytest.mark.parametrize("extra,lo,hi,whole", [(["-s", "-3", "-e", "-1"], 2, 5, True), (["-s", "1", "-e", "4"], 1, 4, False),
                                               (["--account-start-index=-4", "--account-end-index", "-2"], 1, 3, False)])
def test_layer_one_input_slices_of_five_entries(sigs_bin, tmp_path, extra, lo, hi, whole):
    parsed = five_entries()
    text, stdout = layer_one(sigs_bin, tmp_path, parsed, extra)
    got, every = json.loads(text), json.loads(sr.layer_one_text(parsed))
    assert list(got) == list(FIELDS)
    for name in FIELDS:
        assert len(every[name]) == 5 and got[name] == every[name][lo:hi], name
    assert text == json.dumps(got, indent=2)
    assert ("Batch contains all input data" in stdout) == whole
