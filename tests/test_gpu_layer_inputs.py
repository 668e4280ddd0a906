"""The chain from signatures.json to the Pedersen check as scripts/full_workflow.sh runs it, through the two GPU commands
that feed the host-only input steps: every file a step reads is the one the step before wrote (the proofs between the
layers are the reference's committed ones), and what comes out is the reference's committed file, byte for byte."""
import os
import subprocess

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

REF = os.path.join(GOLDEN, "ref")


def text(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_signatures_to_pedersen_check(zk, tmp_path):
    def step(argv, timeout):
        rc = subprocess.run([str(a) for a in argv], capture_output=True, text=True, timeout=timeout)
        assert rc.returncode == 0, (argv[:2], rc.returncode, rc.stderr)      # the first failure ends the chain
        return rc
    parsed, tree = tmp_path / "parsed.json", tmp_path / "tree"
    tree.mkdir()
    step([zk.SIGS_BIN, "--signatures", os.path.join(GOLDEN, "sigs", "signatures_1.json"), "--output-path", parsed], 60)
    step([zk.MERKLE_BIN, "--anon-set", os.path.join(REF, "merkle", "anonymity_set_10.csv"), "--poa-input-data", parsed,
          "--output-dir", tree], 60)
    two, hash_path, three = tmp_path / "layer_two_input.json", tmp_path / "hash.txt", tmp_path / "layer_three_input.json"
    step([zk.SIGS_BIN, "layer-two-input", "--poa-input-data", parsed, "--merkle-root", tree / "merkle_root.json",
          "--merkle-proofs", tree / "merkle_proofs.json", "--write-x-coords-hash-to", hash_path, "--layer-one-sanitized-proof",
          os.path.join(REF, "1_sigs_1_batches_5_height__layer_one__batch_0", "sanitized_proof.json"),
          "--write-layer-two-data-to", two], 30)
    assert two.read_text() == text(GOLDEN, "layer_inputs", "1_sigs__layer_two_batch_0_input.json")
    assert hash_path.read_text() in two.read_text()
    step([zk.SIGS_BIN, "layer-three-input", "--merkle-root-path", tree / "merkle_root.json", "--layer-two-sanitized-proof-paths",
          os.path.join(REF, "1_sigs_1_batches_5_height__layer_two__batch_0", "sanitized_proof.json"),
          "--write-layer-three-data-to", three, "--blindingFactor", "2"], 30)
    assert three.read_text() == text(GOLDEN, "layer_inputs", "1_sigs__layer_three_input.json")
    rc = step([zk.SIGS_BIN, "pedersen-check", "--poa-input-data", parsed, "--layer-three-public-inputs",
               os.path.join(REF, "1_sigs_1_batches_5_height__layer_three", "public.json"), "--blindingFactor", "2"], 30)
    assert rc.stdout.splitlines() == ["Balance sum calculated from input data: 354", "Blinding factor given: 2"]
