"""Makes tests/golden/layer_inputs/ (data only) from a checkout of the reference, given as the one argument:
the three layer_two_batch_*_input.json and the two layer_three_input.json files the reference's tests commit, copied byte
for byte, and x_coord_hashes.json: the x limbs (`pubkey[i][0]`) and `pubkey_x_coord_hash` of every committed layer-two
input, eleven files in all."""
import json
import os
import shutil
import sys

REF = os.path.join(sys.argv[1], "tests")
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "layer_inputs")
COPIES = {
    "1_sigs_1_batches_5_height/layer_two/batch_0/layer_two_batch_0_input.json": "1_sigs__layer_two_batch_0_input.json",
    "4_sigs_2_batches_12_height/layer_two/batch_0/layer_two_batch_0_input.json": "4_sigs__layer_two_batch_0_input.json",
    "4_sigs_2_batches_12_height/layer_two/batch_1/layer_two_batch_1_input.json": "4_sigs__layer_two_batch_1_input.json",
    "1_sigs_1_batches_5_height/layer_three/layer_three_input.json": "1_sigs__layer_three_input.json",
    "4_sigs_2_batches_12_height/layer_three/layer_three_input.json": "4_sigs__layer_three_input.json",
}
HASHED = list(COPIES)[:3] + [
    "1_sigs_1_batches_5_height/layer_two_input.json",
    "old/2_sigs/layer_two_input.json",
    "old/6_sigs_parallel/layer_two_input_0.json",
    "old/6_sigs_parallel/layer_two_input_1.json",
    "old/6_sigs_parallel/layer_two_input_2.json",
    "old/7_sigs/layer_two_input.json",
    "old/16_sigs/layer_two_input.json",
    "old/128_sigs/layer_two_input.json",
]
os.makedirs(HERE, exist_ok=True)
for src, dst in COPIES.items():
    shutil.copyfile(os.path.join(REF, src), os.path.join(HERE, dst))
cases = []
for src in HASHED:
    d = json.load(open(os.path.join(REF, src)))
    cases.append({"file": "tests/" + src, "x_limbs": [limb for key in d["pubkey"] for limb in key[0]],
                  "pubkey_x_coord_hash": d["pubkey_x_coord_hash"]})
with open(os.path.join(HERE, "x_coord_hashes.json"), "w") as f:
    json.dump(cases, f, indent=1)
    f.write("\n")
