"""`ecdsa-sigs-parser layer-two-input | layer-three-input | pedersen-check` and the four host-only entry points behind
them (include/zkpoa_layer_inputs.h), without a GPU: first tests/layer_inputs_ref.py is pinned by the files the reference
commits (tests/golden/layer_inputs/), then the library and the commands are compared with those files byte for byte
and with the restatement where the reference has no file."""
import ctypes
import json
import os
import random
import re
import subprocess

import pytest

import layer_inputs_ref as ref
from conftest import GOLDEN, ROOT

# not under golden/ref/: every directory there is a proof fixture (tests/test_oracle_fixtures.py)
FIX = os.path.join(GOLDEN, "layer_inputs")
BLINDING_4 = 57896044618658097711785492504343953926634992332820282019728792003956564819948   # tests/4_sigs_2_batches_12_height.sh:12
CASES = {"1_sigs": ("1_sigs_1_batches_5_height", 2, [0]), "4_sigs": ("4_sigs_2_batches_12_height", BLINDING_4, [0, 1])}
# the order in which the reference's run handed the layer-two proofs to layer three: its file has balances [1582, 632]
LAYER_THREE_ORDER = {"1_sigs": [0], "4_sigs": [1, 0]}


def text(path):
    with open(path) as f:
        return f.read()


def ref_dir(case, layer, batch=None):
    return os.path.join(GOLDEN, "ref", "%s__%s" % (CASES[case][0], layer) + ("" if batch is None else "__batch_%d" % batch))


def layer_two_fixture(case, batch):
    return text(os.path.join(FIX, "%s__layer_two_batch_%d_input.json" % (case, batch)))


@pytest.fixture(scope="module")
def hash_cases():
    return [([int(v) for v in c["x_limbs"]], int(c["pubkey_x_coord_hash"]), c["file"])
            for c in json.loads(text(os.path.join(FIX, "x_coord_hashes.json")))]


@pytest.fixture(scope="module")
def sigs_bin(zk):
    if not os.path.exists(zk.SIGS_BIN):
        import __graft_entry__ as entry
        entry.build()
    return zk.SIGS_BIN


def run(argv, **kw):
    return subprocess.run([str(a) for a in argv], capture_output=True, text=True, timeout=60, **kw)


# ---- the restatements against the reference's files ----------------------------------------------------------------
def test_restated_sponge_gives_the_eleven_committed_hashes(hash_cases):
    assert len(hash_cases) == 11 and sorted({len(x) for x, _, _ in hash_cases}) == [4, 8, 28, 64, 512]
    for x, want, name in hash_cases:
        assert ref.poseidon_sponge(x) == want, name
    # the 7-signature file holds only with the last round's offset rule: reading at 16 gives another hash
    x, want, _ = next(c for c in hash_cases if len(c[0]) == 28)
    assert ref.poseidon(x[16:28], ref.poseidon(x[:16])[0], 2)[1] != want


def test_restated_width_three_is_the_oracles_poseidon():
    """Two generators written apart (the oracle's steps bit by bit, this one 18 bits at a time) agree where both exist."""
    from oracle.py import poseidon as op
    C, M = ref.poseidon_params(3)
    assert (C, [list(row) for row in M]) == (op.params(3)[0], [list(row) for row in op.params(3)[1]])
    assert ref.poseidon([1, 2]) == [op.poseidon([1, 2])]
    assert op.poseidon([1, 2]) == 7853200120776062878684798364095072458815029376092732009249414926327459813530   # circomlib's own test vector


@pytest.mark.parametrize("case", ["1_sigs", "4_sigs"])
def test_restated_commitment_is_the_committed_public_signals(case):
    _, blinding, batches = CASES[case]
    balances = [int(b) for k in batches for b in json.loads(layer_two_fixture(case, k))["leaf_balances"]]
    assert sum(balances) == {"1_sigs": 354, "4_sigs": 1582 + 632}[case]
    signals = json.loads(text(os.path.join(ref_dir(case, "layer_three"), "public.json")))
    assert ref.point_equal(ref.pedersen_commitment(sum(balances), blinding), ref.dechunk_to_point(signals[:12]))
    assert not ref.point_equal(ref.pedersen_commitment(sum(balances) + 1, blinding), ref.dechunk_to_point(signals[:12]))
    want = json.loads(text(os.path.join(FIX, "%s__layer_three_input.json" % case)))
    assert want["ped_com_blinding_factor"] == ref.format_scalar_power(blinding)
    assert want["ped_com_generator_g"] == [ref.chunks85(v) for v in ref.GEN_G]
    assert want["ped_com_generator_h"] == [ref.chunks85(v) for v in ref.GEN_H]


# ---- the C ABI -----------------------------------------------------------------------------------------------------
def test_new_header_matches_the_binding_table(zk):
    """include/zkpoa_layer_inputs.h against _abi.LAYER_INPUT_SIGNATURES, as tests/test_abi.py does for the main header, and
    the main header includes it."""
    from zkpoa_amd import _abi
    import test_abi
    src = text(os.path.join(ROOT, "include", "zkpoa_layer_inputs.h"))
    src = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.M)
    protos = re.findall(r"([\w \t*]+?[\s*])(zkpoa_\w+)\s*\(([^()]*)\)\s*;", src)
    assert sorted(n for _, n, _ in protos) == sorted(_abi.LAYER_INPUT_SIGNATURES) and len(protos) == 4
    L = zk.lib()
    for ret, name, args in protos:
        restype, argtypes = _abi.signature(_abi.LAYER_INPUT_SIGNATURES[name])
        assert test_abi._ctypes_class(restype) == test_abi._c_class(ret + " ret"), name
        assert [test_abi._ctypes_class(t) for t in argtypes] == [test_abi._c_class(a.strip()) for a in args.split(",")], name
        assert list(getattr(L, name).argtypes) == argtypes
    assert '#include "zkpoa_layer_inputs.h"' in text(os.path.join(ROOT, "include", "zkpoa_prover.h"))
    assert not set(_abi.LAYER_INPUT_SIGNATURES) & (set(_abi.SIGNATURES) | set(_abi.HOOK_SIGNATURES))


def test_sponge_through_the_abi_gives_the_eleven_committed_hashes(zk, hash_cases):
    for x, want, name in hash_cases:
        assert zk.poseidon_sponge(x) == want, name


@pytest.mark.parametrize("n", [1, 4, 15, 16, 17, 20, 32, 33, 60, 64])
def test_sponge_at_the_edges_of_the_offset_rule(zk, n):
    rng = random.Random(n)
    x = [rng.randrange(ref.R) for _ in range(n)]
    assert zk.poseidon_sponge(x) == ref.poseidon_sponge(x)


def test_sponge_refuses_no_input_and_values_outside_the_field(zk):
    out = ctypes.create_string_buffer(32)
    assert zk.lib().zkpoa_poseidon_sponge(b"\0" * 32, 0, out) == zk.PROVER_ERROR
    with pytest.raises(zk.ZkpoaError):
        zk.poseidon_sponge([])
    with pytest.raises(zk.ZkpoaError):
        zk.poseidon_sponge([ref.R])
    assert zk.poseidon_sponge([ref.R - 1]) == ref.poseidon_sponge([ref.R - 1])


@pytest.mark.parametrize("t", range(2, 18))
def test_poseidon_hash_at_every_width(zk, t):
    rng = random.Random(100 + t)
    x, init = [rng.randrange(ref.R) for _ in range(t - 1)], rng.randrange(1, ref.R)
    state = ref.poseidon(x, init, t)
    assert zk.poseidon_hash(x, init, t) == state
    assert zk.poseidon_hash(x, init, 1) == state[:1]
    for bad_inputs, n_out in ((x, 0), (x, t + 1), ([], 1), (x + [1] * (17 - len(x)), 1)):
        with pytest.raises(zk.ZkpoaError):
            zk.poseidon_hash(bad_inputs, init, n_out)


def test_width_three_parameters_did_not_move(zk):
    """The generator now takes (t, R_P): what it makes at (3, 57) is what the restatement's own generator makes."""
    C, M = zk.poseidon_params()
    assert (C, M) == ref.poseidon_params(3)


@pytest.mark.parametrize("secret,blinding", [(0, 0), (0, 5), (7, 0), (354, 2), (1582 + 632, BLINDING_4), (2 ** 64 + 3, 2 ** 255 - 1)])
def test_commitment_through_the_abi(zk, secret, blinding):
    want = ref.pedersen_commitment(secret, blinding)
    assert zk.pedersen_commit(secret, blinding) == want
    signals = [int(c) for v in want for c in ref.chunks85(v)]
    assert zk.pedersen_check(secret, blinding, signals)
    assert not zk.pedersen_check(secret + 1, blinding, signals)
    assert not zk.pedersen_check(secret, blinding + 1, signals)
    # another projective form of the same point, and chunks that are not reduced
    scaled = [v * 12345 % ref.P for v in want]
    assert zk.pedersen_check(secret, blinding, [int(c) for v in scaled for c in ref.chunks85(v)])
    loose = list(signals)
    loose[0], loose[1] = loose[0] + (1 << 85), loose[1] - 1 if loose[1] else loose[1]
    assert zk.pedersen_check(secret, blinding, loose) == ref.point_equal(want, ref.dechunk_to_point(loose))
    if (secret, blinding) == (0, 0):
        assert want == (0, 4, 4, 0)                                             # pointAdd of two identities (0, 1, 1, 0)


# ---- files for the commands ------------------------------------------------------------------------------------------
def big(v):
    return {"__bigint__": str(v)}


def parsed_text(accounts):
    """A parsed-signatures file with the fields these steps read and no others: accounts = [(x, y, address, balance)]."""
    return json.dumps({"accountAttestations": [
        {"signature": {"pubkey": {"x": big(x), "y": big(y)}}, "accountData": {"address": big(a), "balance": big(b)}}
        for x, y, a, b in accounts]}, indent=2)


def proofs_text(addresses, balances, elements, indices):
    return json.dumps({"leaves": [{"address": big(a), "balance": big(b), "hash": big(0)} for a, b in zip(addresses, balances)],
                       "path_elements": [[big(e) for e in row] for row in elements], "path_indices": indices}, indent=2)


def from_limbs(limbs):
    return sum(int(v) << (64 * i) for i, v in enumerate(limbs))


def layer_two_inputs(tmp_path, fixtures):
    """parsed.json, merkle_root.json and merkle_proofs.json made of the fields of the reference's layer-two inputs."""
    d = [json.loads(f) for f in fixtures]
    accounts = [(from_limbs(k[0]), from_limbs(k[1]), int(a), int(b))
                for f in d for k, a, b in zip(f["pubkey"], f["leaf_addresses"], f["leaf_balances"])]
    (tmp_path / "parsed.json").write_text(parsed_text(accounts))
    (tmp_path / "merkle_root.json").write_text(json.dumps(big(d[0]["merkle_root"]), indent=2))
    (tmp_path / "merkle_proofs.json").write_text(proofs_text(
        [a[2] for a in accounts], [a[3] for a in accounts], [row for f in d for row in f["path_elements"]],
        [row for f in d for row in f["path_indices"]]))
    return accounts


def layer_two_argv(sigs_bin, tmp_path, proof, short=False, **replace):
    names = (("--poa-input-data", "-i"), ("--merkle-root", "-t"), ("--merkle-proofs", "-p"), ("--write-x-coords-hash-to", "-h"),
             ("--layer-one-sanitized-proof", "-d"), ("--write-layer-two-data-to", "-o"))
    values = [tmp_path / "parsed.json", tmp_path / "merkle_root.json", tmp_path / "merkle_proofs.json", tmp_path / "hash.txt",
              proof, tmp_path / "layer_two_input.json"]
    argv = [sigs_bin, "layer-two-input"]
    for (long_name, short_name), v in zip(names, values):
        if replace.get(long_name, v) is not None:
            argv += [short_name if short else long_name, replace.get(long_name, v)]
    return argv


# ---- layer-two-input -----------------------------------------------------------------------------------------------
def test_layer_two_input_of_the_one_signature_test(sigs_bin, tmp_path):
    want = layer_two_fixture("1_sigs", 0)
    layer_two_inputs(tmp_path, [want])
    proof = os.path.join(ref_dir("1_sigs", "layer_one", 0), "sanitized_proof.json")
    rc = run(layer_two_argv(sigs_bin, tmp_path, proof) + ["--account-end-index", "-1"])
    assert rc.returncode == 0, rc.stderr
    assert (tmp_path / "layer_two_input.json").read_text() == want
    assert (tmp_path / "hash.txt").read_text() == json.loads(want)["pubkey_x_coord_hash"]
    assert rc.stdout.splitlines() == [
        "Preparing input for layer 2 using the following data:", "- System input: %s" % (tmp_path / "parsed.json"),
        "- Start index for batch: 0", "- End index for batch: -1", "- Merkle proofs path: %s" % (tmp_path / "merkle_proofs.json"),
        "- Merkle root path: %s" % (tmp_path / "merkle_root.json"), "Path to write processed data to: %s" % (tmp_path / "layer_two_input.json"),
        "Path to write public keys hash to: %s" % (tmp_path / "hash.txt"), "",
        "Batch contains all input data i.e. there is only 1 batch",
        "Hash of public keys x-coords: %s" % json.loads(want)["pubkey_x_coord_hash"],
        "Checking that the order of addresses in input data & Merkle proofs is the same.."]
    assert sorted(os.listdir(tmp_path)) == ["hash.txt", "layer_two_input.json", "merkle_proofs.json", "merkle_root.json", "parsed.json"]


@pytest.mark.parametrize("batch", [0, 1])
def test_layer_two_input_of_a_batch_of_the_four_signature_test(sigs_bin, tmp_path, batch):
    want = [layer_two_fixture("4_sigs", k) for k in (0, 1)]
    layer_two_inputs(tmp_path, want)
    proof = os.path.join(ref_dir("4_sigs", "layer_one", batch), "sanitized_proof.json")
    rc = run(layer_two_argv(sigs_bin, tmp_path, proof, short=True) + ["-s", 2 * batch, "-e", 2 * batch + 2])
    assert rc.returncode == 0, rc.stderr
    assert (tmp_path / "layer_two_input.json").read_text() == want[batch]
    assert (tmp_path / "hash.txt").read_text() == json.loads(want[batch])["pubkey_x_coord_hash"]
    assert "only 1 batch" not in rc.stdout


def seven_accounts(hash_cases):
    x, want, _ = next(c for c in hash_cases if len(c[0]) == 28)
    return [(from_limbs(x[4 * i:4 * i + 4]), 1000 + i, 500 + 3 * i, 10 * i) for i in range(7)], want


def write_seven(tmp_path, accounts, leaves=None):
    (tmp_path / "parsed.json").write_text(parsed_text(accounts))
    (tmp_path / "merkle_root.json").write_text(json.dumps(big(77), indent=2))
    leaves = [a[2] for a in accounts] if leaves is None else leaves
    (tmp_path / "merkle_proofs.json").write_text(proofs_text(leaves, [0] * len(leaves), [[5, 6]] * len(leaves), [[0, 1]] * len(leaves)))


def test_layer_two_input_of_seven_accounts_has_the_reference_hash(sigs_bin, tmp_path, hash_cases):
    accounts, want = seven_accounts(hash_cases)
    write_seven(tmp_path, accounts)
    proof = os.path.join(ref_dir("1_sigs", "layer_one", 0), "sanitized_proof.json")
    rc = run(layer_two_argv(sigs_bin, tmp_path, proof))
    assert rc.returncode == 0, rc.stderr
    assert (tmp_path / "hash.txt").read_text() == str(want)
    got = json.loads((tmp_path / "layer_two_input.json").read_text())
    assert got["pubkey_x_coord_hash"] == str(want) and got["leaf_addresses"] == [str(a[2]) for a in accounts]
    assert got["path_elements"] == [["5", "6"]] * 7 and got["path_indices"] == [[0, 1]] * 7 and got["merkle_root"] == "77"
    assert list(got)[:7] == ["gamma2", "delta2", "negalfa1xbeta2", "IC", "negpa", "pb", "pc"] and "pubInput" not in got
    # slices with negative indices are Array.prototype.slice's: the last three accounts, all but the last two, an end past the array
    for extra, lo, hi in ((["-s", "-3", "-e", "7"], 4, 7), (["-s", "-7", "-e", "-2"], 0, 5), (["-s", "5", "-e", "100"], 5, 7)):
        rc = run(layer_two_argv(sigs_bin, tmp_path, proof) + extra)
        assert rc.returncode == 0, rc.stderr
        got = json.loads((tmp_path / "layer_two_input.json").read_text())
        assert got["leaf_addresses"] == [str(a[2]) for a in accounts[lo:hi]] and len(got["path_indices"]) == hi - lo
        assert got["pubkey_x_coord_hash"] == str(ref.poseidon_sponge([v for a in accounts[lo:hi] for v in ref.x_limbs(a[0])]))


def layer_two_error_cases(accounts):
    addr = [a[2] for a in accounts]
    swapped = list(accounts)
    swapped[3], swapped[4] = swapped[4], swapped[3]
    twice = list(accounts)
    twice[5] = twice[5][:2] + (twice[4][2],) + twice[5][3:]
    return {
        "length": (accounts, addr[:6], [], "Length of input data array 7 should equal length of merkle proofs array 6"),
        "mismatch": (accounts, addr[:2] + [addr[2] + 1] + addr[3:], [],
                     "[i = 2] Address in input data array %d should equal address in merkle proofs array %d" % (addr[2], addr[2] + 1)),
        "descending": (swapped, None, [], "Addresses must be in ascending order, but address at i=4 (%d) is less than the previous address (%d)"
                       % (addr[3], addr[4])),
        "duplicate": (twice, None, [], "Cannot have duplicate addresses, but address at i=5 (%d) is the same as the previous address (%d)"
                      % (addr[4], addr[4])),
        "range": (accounts, None, ["-s", "3", "-e", "3"], "startIndex 3 must be less than endIndex 3"),
    }


@pytest.mark.parametrize("case", ["length", "mismatch", "descending", "duplicate", "range", "missing option", "truncated"])
def test_layer_two_input_errors_leave_no_output(sigs_bin, tmp_path, hash_cases, case):
    accounts, _ = seven_accounts(hash_cases)
    proof = os.path.join(ref_dir("1_sigs", "layer_one", 0), "sanitized_proof.json")
    replace = {}
    if case == "missing option":
        write_seven(tmp_path, accounts)
        extra, message, replace = [], "layer-two-input needs --merkle-root <value>", {"--merkle-root": None}
    elif case == "truncated":
        write_seven(tmp_path, accounts)
        whole = (tmp_path / "merkle_proofs.json").read_text()
        (tmp_path / "merkle_proofs.json").write_text(whole[:len(whole) // 2])
        extra, message = [], "malformed JSON"
    else:
        acc, leaves, extra, message = layer_two_error_cases(accounts)[case]
        write_seven(tmp_path, acc, leaves)
    out, hash_out = tmp_path / "layer_two_input.json", tmp_path / "hash.txt"
    for existing in (False, True):
        if existing:
            out.write_text("an earlier output")
            hash_out.write_text("an earlier hash")
        rc = run(layer_two_argv(sigs_bin, tmp_path, proof, **replace) + extra)
        assert rc.returncode == 1 and rc.stderr.startswith("Error: ") and message in rc.stderr, (rc.returncode, rc.stderr)
        assert len(rc.stderr.strip().splitlines()) == 1
        if existing:
            assert out.read_text() == "an earlier output" and hash_out.read_text() == "an earlier hash"
        assert sorted(os.listdir(tmp_path)) == sorted(["parsed.json", "merkle_root.json", "merkle_proofs.json"] +
                                                      (["layer_two_input.json", "hash.txt"] if existing else []))


def test_bad_arguments_are_exit_two_with_the_usage(sigs_bin, tmp_path):
    for argv in (["layer-two-input", "--no-such-option", "1"], ["layer-two-input", "-s", "x"], ["layer-three-input", "-o"],
                 ["pedersen-check", "--poa-input-data"]):
        rc = run([sigs_bin] + argv)
        assert rc.returncode == 2 and "Usage: ecdsa-sigs-parser" in rc.stderr and "layer-three-input" in rc.stderr, rc.stderr


# ---- layer-three-input ---------------------------------------------------------------------------------------------
def layer_three_argv(sigs_bin, tmp_path, proofs, blinding, short=False):
    (tmp_path / "merkle_root.json").write_text(json.dumps(big(json.loads(text(proofs[0]))["pubInput"][1]), indent=2))
    names = ("-m", "-p", "-o") if short else ("--merkle-root-path", "--layer-two-sanitized-proof-paths", "--write-layer-three-data-to")
    return [sigs_bin, "layer-three-input", names[0], tmp_path / "merkle_root.json", names[1], ",".join(str(p) for p in proofs),
            names[2], tmp_path / "layer_three_input.json", "--blindingFactor", blinding]


@pytest.mark.parametrize("case", ["1_sigs", "4_sigs"])
def test_layer_three_input_is_the_reference_file(sigs_bin, tmp_path, case):
    blinding = CASES[case][1]
    proofs = [os.path.join(ref_dir(case, "layer_two", k), "sanitized_proof.json") for k in LAYER_THREE_ORDER[case]]
    rc = run(layer_three_argv(sigs_bin, tmp_path, proofs, blinding, short=case == "4_sigs"))
    assert rc.returncode == 0, rc.stderr
    want = text(os.path.join(FIX, "%s__layer_three_input.json" % case))
    assert (tmp_path / "layer_three_input.json").read_text() == want
    d = json.loads(want)
    assert rc.stdout.splitlines() == [
        "Preparing input for layer 3 using the following data:", "- Merkle root: %s" % d["merkle_root"], "- Blinding factor: %d" % blinding,
        "- Balances (layer 2 output): %s" % ",".join(str(b) for b in d["balances"]),
        "Path to write processed data to: %s" % (tmp_path / "layer_three_input.json"), ""]
    if case == "4_sigs":                                                        # the order given is the order written
        rc = run(layer_three_argv(sigs_bin, tmp_path, proofs[::-1], hex(blinding)))
        assert rc.returncode == 0, rc.stderr
        got = json.loads((tmp_path / "layer_three_input.json").read_text())
        assert got["balances"] == d["balances"][::-1] and got["pc"] == d["pc"][::-1] and got["IC"] == d["IC"][::-1]
        assert got["ped_com_blinding_factor"] == d["ped_com_blinding_factor"]


@pytest.mark.parametrize("blinding", [0, 255, 256, 2 ** 248, 2 ** 255 - 1])
def test_layer_three_blinding_factor_bits(sigs_bin, tmp_path, blinding):
    proofs = [os.path.join(ref_dir("1_sigs", "layer_two", 0), "sanitized_proof.json")]
    rc = run(layer_three_argv(sigs_bin, tmp_path, proofs, blinding))
    assert rc.returncode == 0, rc.stderr
    got = json.loads((tmp_path / "layer_three_input.json").read_text())
    assert got["ped_com_blinding_factor"] == ref.format_scalar_power(blinding) and len(got["ped_com_blinding_factor"]) == 255


def test_layer_three_refusals(sigs_bin, tmp_path):
    good = os.path.join(ref_dir("1_sigs", "layer_two", 0), "sanitized_proof.json")
    out = tmp_path / "layer_three_input.json"
    rc = run(layer_three_argv(sigs_bin, tmp_path, [good], 2 ** 255))
    assert rc.returncode == 1 and "is not below 2^255" in rc.stderr and not out.exists()
    proof = json.loads(text(good))
    for value, refused in ((2 ** 53, True), (2 ** 53 - 1, False), (1.5, True), (-1, True)):
        proof["pubInput"][0] = value
        (tmp_path / "big.json").write_text(json.dumps(proof))
        rc = run(layer_three_argv(sigs_bin, tmp_path, [tmp_path / "big.json"], 2))
        if refused:
            assert rc.returncode == 1 and "pubInput[0] = %s is not an integer below 2^53" % json.dumps(value) in rc.stderr and not out.exists()
        else:
            assert rc.returncode == 0 and json.loads(out.read_text())["balances"] == [value]
            out.unlink()
    (tmp_path / "dir.json").mkdir()
    rc = run(layer_three_argv(sigs_bin, tmp_path, [good, tmp_path / "dir.json"], 2))
    assert rc.returncode == 1 and "Expected %s to be a path to a file" % (tmp_path / "dir.json") in rc.stderr and not out.exists()
    (tmp_path / "proof.txt").write_text(text(good))
    rc = run(layer_three_argv(sigs_bin, tmp_path, [tmp_path / "proof.txt"], 2))
    assert rc.returncode == 1 and "Expected %s to be a path to a json file" % (tmp_path / "proof.txt") in rc.stderr and not out.exists()
    rc = run(layer_three_argv(sigs_bin, tmp_path, [good], 2)[:-2])
    assert rc.returncode == 1 and "layer-three-input needs --blindingFactor" in rc.stderr and not out.exists()


# ---- pedersen-check --------------------------------------------------------------------------------------------------
def pedersen_files(tmp_path, case):
    _, blinding, batches = CASES[case]
    d = [json.loads(layer_two_fixture(case, k)) for k in batches]
    accounts = [(1, 2, int(a), int(b)) for f in d for a, b in zip(f["leaf_addresses"], f["leaf_balances"])]
    (tmp_path / "parsed.json").write_text(parsed_text(accounts))
    signals = json.loads(text(os.path.join(ref_dir(case, "layer_three"), "public.json")))
    (tmp_path / "public.json").write_text(json.dumps(signals, indent=1))
    return accounts, signals, blinding


def pedersen_argv(sigs_bin, tmp_path, blinding, short=False):
    names = ("-i", "-p") if short else ("--poa-input-data", "--layer-three-public-inputs")
    return [sigs_bin, "pedersen-check", names[0], tmp_path / "parsed.json", names[1], tmp_path / "public.json", "--blindingFactor", blinding]


@pytest.mark.parametrize("case", ["1_sigs", "4_sigs"])
def test_pedersen_check(sigs_bin, tmp_path, case):
    accounts, signals, blinding = pedersen_files(tmp_path, case)
    total = sum(a[3] for a in accounts)
    rc = run(pedersen_argv(sigs_bin, tmp_path, blinding, short=case == "4_sigs"))
    assert rc.returncode == 0, rc.stderr
    assert rc.stdout.splitlines() == ["Balance sum calculated from input data: %d" % total, "Blinding factor given: %d" % blinding]
    assert rc.stderr == ""
    # another blinding factor
    rc = run(pedersen_argv(sigs_bin, tmp_path, blinding + 1))
    assert rc.returncode == 1 and rc.stderr.startswith("Error: the Pedersen commitment") and len(rc.stderr.strip().splitlines()) == 1
    # one altered signal
    (tmp_path / "public.json").write_text(json.dumps([str(int(signals[0]) ^ 1)] + signals[1:]))
    assert run(pedersen_argv(sigs_bin, tmp_path, blinding)).returncode == 1
    # eleven signals
    (tmp_path / "public.json").write_text(json.dumps(signals[:11]))
    rc = run(pedersen_argv(sigs_bin, tmp_path, blinding))
    assert rc.returncode == 1 and "holds 11 public signals" in rc.stderr
    # one balance more
    (tmp_path / "public.json").write_text(json.dumps(signals))
    assert run(pedersen_argv(sigs_bin, tmp_path, blinding)).returncode == 0
    accounts[-1] = accounts[-1][:3] + (accounts[-1][3] + 1,)
    (tmp_path / "parsed.json").write_text(parsed_text(accounts))
    rc = run(pedersen_argv(sigs_bin, tmp_path, blinding))
    assert rc.returncode == 1 and "Balance sum calculated from input data: %d" % (total + 1) in rc.stdout


# ---- the modes' header compiled alone (and, with LAYER_INPUTS_CHECK_FLAGS, under a sanitizer) --------------------------
def test_modes_compiled_alone(tmp_path):
    """tools/layer_inputs_check.cpp: g++ compiles csrc/layer_inputs.hpp without HIP and without the library, and the three
    modes give the reference's files from there too."""
    import shlex
    check = tmp_path / "layer_inputs_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread"] + shlex.split(os.environ.get("LAYER_INPUTS_CHECK_FLAGS", "")) +
                   ["-I", os.path.join(ROOT, "zk-proof-of-assets_amd", "csrc"), os.path.join(ROOT, "tools", "layer_inputs_check.cpp"),
                    "-o", str(check)], check=True, capture_output=True, text=True)
    want = [layer_two_fixture("4_sigs", k) for k in (0, 1)]
    layer_two_inputs(tmp_path, want)
    for batch in (0, 1):
        rc = run([check, "two", tmp_path / "parsed.json", tmp_path / "merkle_root.json", tmp_path / "merkle_proofs.json", tmp_path / "hash.txt",
                  os.path.join(ref_dir("4_sigs", "layer_one", batch), "sanitized_proof.json"), tmp_path / "two.json", 2 * batch, 2 * batch + 2])
        assert rc.returncode == 0 and rc.stderr == "", rc.stderr
        assert (tmp_path / "two.json").read_text() == want[batch]
    rc = run([check, "two", tmp_path / "parsed.json", tmp_path / "merkle_root.json", tmp_path / "merkle_proofs.json", tmp_path / "hash.txt",
              os.path.join(ref_dir("4_sigs", "layer_one", 0), "sanitized_proof.json"), tmp_path / "two.json", 3, 2])
    assert rc.returncode == 1 and rc.stderr == "Error: startIndex 3 must be less than endIndex 2\n"
    proofs = ",".join(os.path.join(ref_dir("4_sigs", "layer_two", k), "sanitized_proof.json") for k in LAYER_THREE_ORDER["4_sigs"])
    rc = run([check, "three", tmp_path / "merkle_root.json", proofs, tmp_path / "three.json", BLINDING_4])
    assert rc.returncode == 0 and rc.stderr == "", rc.stderr
    assert (tmp_path / "three.json").read_text() == text(os.path.join(FIX, "4_sigs__layer_three_input.json"))
    public = os.path.join(ref_dir("4_sigs", "layer_three"), "public.json")
    rc = run([check, "pedersen", tmp_path / "parsed.json", public, BLINDING_4])
    assert rc.returncode == 0 and rc.stderr == "", rc.stderr
    rc = run([check, "pedersen", tmp_path / "parsed.json", public, BLINDING_4 - 1])
    assert rc.returncode == 1 and rc.stderr.startswith("Error: the Pedersen commitment")
