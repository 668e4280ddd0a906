"""The time slots of zkpoa_last_ms: csrc/zkpoa_internal.hpp's enum MsSlot against the ids that the comment in
include/zkpoa_prover.h documents. The ids are ABI: the enum counts exactly the documented ones, and the enumerator of
every id is the one listed here, so a slot inserted in the middle or two slots swapped fail. No GPU."""
import os
import re

from conftest import ROOT

# id -> enumerator. An id keeps its meaning for good: a new slot is appended here, in the enum and in the header comment.
SLOTS = ["kMsMsm", "kMsMsmAccum", "kMsNtt", "kMsChain", "kMsMsmPhase", "kMsProve", "kMsSelfCheck", "kMsMerkleBuild",
         "kMsLaneBatch", "kMsAnonIndex", "kMsAnonFind"]


def enumerators():
    src = open(os.path.join(ROOT, "zk-proof-of-assets_amd", "csrc", "zkpoa_internal.hpp")).read()
    body = re.sub(r"//.*", "", re.search(r"enum MsSlot : int \{(.*?)\};", src, flags=re.S).group(1))
    assert "=" not in body                                                             # no explicit values: position is the id
    return [name.strip() for name in body.split(",") if name.strip()], src


def documented_ids():
    src = open(os.path.join(ROOT, "include", "zkpoa_prover.h")).read()
    text = re.search(r"/\* Timings \(ms, HIP events.*?\n \* Also:", src, flags=re.S).group(0)
    return [int(v) for v in re.findall(r"\b(\d+) = ", text)]


def test_the_enum_counts_the_documented_ids():
    names, src = enumerators()
    assert documented_ids() == list(range(11))
    assert names[-1] == "kMsCount" and len(names) - 1 == len(documented_ids())
    assert "float ms[zkpoa::kMsCount]" in src
    api = open(os.path.join(ROOT, "zk-proof-of-assets_amd", "csrc", "zkpoa_api.hip")).read()
    assert re.search(r"zkpoa_last_ms\(const zkpoa_context\* ctx, int id\) \{\s*if \(!ctx \|\| id < 0 \|\| id >= kMsCount\)", api)


def test_the_enumerators_are_in_id_order():
    names, _ = enumerators()
    assert names[:-1] == SLOTS


def test_every_id_answers_minus_one_without_a_context(zk):
    for ident in documented_ids() + [-1, len(documented_ids())]:
        assert zk.lib().zkpoa_last_ms(None, ident) == -1.0
