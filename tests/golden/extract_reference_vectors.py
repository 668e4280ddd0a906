"""Makes the reference-vector fixtures (data only) from a checkout of the reference, given as the one argument:
  sigs/reference_ecdsa_star_experiments.json  the ECDSA* tuples of experiments/scripts/batch_ecdsa_input_prep/input_N.json
  sigs/reference_ecdsa_star_tests.json        those of the layer-one inputs under tests/old/ and tests/4_sigs_2_batches_12_height/
  ref/merkle/height24_paths.json              the five Merkle fields of tests/old/{2,7,16,128}_sigs/layer_two_input.json
and three byte-for-byte copies (COPIES below). tests/golden/sigs/README.txt and tests/golden/ref/merkle/README.txt say
what each holds. Every record is one (r, s, msghash) once: a tuple that a later file repeats keeps its first source."""
import json
import os
import shutil
import sys

REF = sys.argv[1]
HERE = os.path.dirname(os.path.abspath(__file__))
EXPERIMENTS = "experiments/scripts/batch_ecdsa_input_prep"
WITH_LAYER_TWO = ["tests/old/%d_sigs" % n for n in (2, 7, 16, 128)]      # layer_one_input.json + layer_two_input.json
LAYER_ONE_ONLY = ["tests/old/6_sigs_parallel/layer_one_input_%d.json" % i for i in (0, 1, 2)] + \
                 ["tests/4_sigs_2_batches_12_height/layer_one/batch_%d/layer_one_batch_%d_input.json" % (b, b) for b in (0, 1)]
COPIES = {
    "experiments/scripts/merkle_inputs.json": "ref/merkle/circomlibjs_path.json",
    "experiments/scripts/keccak_inputs.json": "sigs/keccak_inputs.json",
    "experiments/scripts/groth16_input_prep/full-circom-input.json": "ref/snarkjs_style/full-circom-input.json",
}


def load(rel):
    with open(os.path.join(REF, rel)) as f:
        return json.load(f)


def limbs(v):
    return sum(int(x) << (64 * i) for i, x in enumerate(v))


def tuples(d):
    """The file's entries as (r, s, rprime, msghash, x, y) integers."""
    n = len(d["r"])
    assert all(len(d[k]) == n for k in ("s", "rprime", "msghash", "pubkey"))
    return [(limbs(d["r"][i]), limbs(d["s"][i]), limbs(d["rprime"][i]), limbs(d["msghash"][i]),
             limbs(d["pubkey"][i][0]), limbs(d["pubkey"][i][1])) for i in range(n)]


class Records:
    def __init__(self):
        self.out, self.seen = [], set()

    def add(self, rel, entries, addresses=None):
        for i, (r, s, rprime, z, x, y) in enumerate(entries):
            if (r, s, z) in self.seen:
                continue
            self.seen.add((r, s, z))
            rec = {"source": "%s#%d" % (rel, i)}
            rec.update((k, "%064x" % v) for k, v in (("r", r), ("s", s), ("rprime", rprime), ("msghash", z),
                                                     ("pubkey_x", x), ("pubkey_y", y)))
            rec["address"] = "%040x" % int(addresses[i]) if addresses else None
            self.out.append(rec)

    def write(self, name):
        with open(os.path.join(HERE, "sigs", name), "w") as f:
            json.dump(self.out, f, indent=1)
            f.write("\n")


# ---- experiments: input_128.json first; every smaller file must repeat its start, and what does not is kept as well
exp = Records()
sizes = sorted(int(n[len("input_"):-len(".json")]) for n in os.listdir(os.path.join(REF, EXPERIMENTS))
               if n.startswith("input_") and n.endswith(".json"))
assert sizes[-1] == 128
full = tuples(load("%s/input_128.json" % EXPERIMENTS))
exp.add("%s/input_128.json" % EXPERIMENTS, full)
total = 0
for n in sizes:
    part = tuples(load("%s/input_%d.json" % (EXPERIMENTS, n)))
    total += len(part)
    assert len(part) == n and part == full[:n], "input_%d.json is no prefix of input_128.json" % n
    exp.add("%s/input_%d.json" % (EXPERIMENTS, n), part)
exp.write("reference_ecdsa_star_experiments.json")

# ---- tests: the four directories with a layer-two file first, so that a repeated tuple keeps the record with an address
tests = Records()
paths = {"siblings": [], "sets": []}
index_of = {}
for d in WITH_LAYER_TWO:
    one, two = load(d + "/layer_one_input.json"), load(d + "/layer_two_input.json")
    assert one["pubkey"] == two["pubkey"] and len(two["leaf_addresses"]) == len(one["r"])
    total += len(one["r"])
    tests.add(d + "/layer_one_input.json", tuples(one), two["leaf_addresses"])
    elems = []
    for path in two["path_elements"]:
        elems.append([index_of.setdefault(e, len(index_of)) for e in path])
    paths["sets"].append({"source": d + "/layer_two_input.json",
                          "leaf_addresses": two["leaf_addresses"], "leaf_balances": two["leaf_balances"],
                          "merkle_root": two["merkle_root"], "path_elements": elems, "path_indices": two["path_indices"]})
for rel in LAYER_ONE_ONLY:
    one = load(rel)
    total += len(one["r"])
    tests.add(rel, tuples(one))
tests.write("reference_ecdsa_star_tests.json")
paths["siblings"] = sorted(index_of, key=index_of.get)


def rows(items):
    """A JSON list with one item per line."""
    return "[\n" + ",\n".join(json.dumps(x, separators=(",", ":")) for x in items) + "\n]"


with open(os.path.join(HERE, "ref", "merkle", "height24_paths.json"), "w") as f:
    f.write('{"siblings": %s,\n"sets": [\n' % rows(paths["siblings"]))
    for k, s in enumerate(paths["sets"]):
        f.write('{"source": %s,\n' % json.dumps(s["source"]))
        for key in ("leaf_addresses", "leaf_balances"):
            f.write('"%s": %s,\n' % (key, rows(s[key])))
        f.write('"merkle_root": %s,\n' % json.dumps(s["merkle_root"]))
        f.write('"path_elements": %s,\n"path_indices": %s}%s\n' % (rows(s["path_elements"]), rows(s["path_indices"]),
                                                                 "," if k + 1 < len(paths["sets"]) else ""))
    f.write("]}\n")

for src, dst in COPIES.items():
    shutil.copyfile(os.path.join(REF, src), os.path.join(HERE, dst))
print("%d tuples read: %d + %d distinct; %d paths, %d distinct siblings" % (
    total, len(exp.out), len(tests.out), sum(len(s["leaf_addresses"]) for s in paths["sets"]), len(paths["siblings"])))
