"""Which request (csrc/msm_plan.hpp MsmRequest) each of the prover's five MSMs is planned with, pinned through the only
run-time observable the library has: a lane's count of mixed additions (last_ms_lane(lane, 2): the non-zero digits of
its scalars, deterministic for a witness, a form and a window width). The table of call sites (csrc/prover.hip
stage_request, DESIGN.md "MSM plans") says who plans with the witness's digit density and who does not; a call site that
changed sides would take another window width and show another count. The constants were recorded on the commit before
the density became an argument (it was a thread-local hint then) and that commit passes this test.

Shape: k = 12, m = 3000 (that of test_sparse_first_pass_extreme_witnesses) is the smallest tried, and there the default
and ZKPOA_NO_DENSITY=1 already differ on the A, B1 and C lanes."""
import random

import pytest

from oracle.py.bn254 import R

pytestmark = pytest.mark.gpu

K, M = 12, 3000
CHUNK = 700          # msm_max_points below the B query's length: no shared sort, B1 and B2 each run their own MSMs

# H, A, B1, B2, C: mixed additions of one proof
COUNTS = {
    "classic": [117159, 22848, 18655, 18655, 24696],
    "chunked": [148998, 26629, 22087, 16877, 29198],      # B1 with the density, B2 without: the known mismatch
    "no_density": [117159, 17782, 14508, 14508, 19217],
    "tables": [81871, 16124, 13175, 13175, 17427],
}


def lane_adds(ctx):
    return [int(round(ctx.last_ms_lane(lane, 2) * 1e6)) for lane in range(5)]


def test_each_stage_is_planned_with_its_own_request(ctx, zk, monkeypatch):
    from zkpoa_amd.synthetic import SyntheticCircuit
    monkeypatch.delenv("ZKPOA_NO_DENSITY", raising=False)
    circ = SyntheticCircuit(zk, ctx, K, M, n_public=2, seed=5, witness_like=True)
    got = {}
    try:
        rng = random.Random(8)
        r_, s_ = rng.randrange(R), rng.randrange(R)
        want, _ = circ.prove(r_, s_)
        got["classic"] = lane_adds(ctx)
        ctx.set_option("msm_max_points", CHUNK)
        try:
            assert circ.prove(r_, s_)[0] == want
            got["chunked"] = lane_adds(ctx)
        finally:
            ctx.set_option("msm_max_points", 0)
        monkeypatch.setenv("ZKPOA_NO_DENSITY", "1")      # (read at every proof)
        assert circ.prove(r_, s_)[0] == want
        got["no_density"] = lane_adds(ctx)
        monkeypatch.delenv("ZKPOA_NO_DENSITY")
        assert circ.key.precompute() > 0
        assert circ.prove(r_, s_)[0] == want
        got["tables"] = lane_adds(ctx)
    finally:
        circ.close()
    for case in COUNTS:
        print("mixed additions H, A, B1, B2, C, %-10s: %s" % (case, got[case]))
    # the density must matter at this shape, or the equalities below could not tell the call sites apart
    assert got["classic"] != got["no_density"]
    assert got["classic"][0] == got["no_density"][0]     # H never takes it
    # B2's own MSM is planned without the density, B1's own with it (the known mismatch: DESIGN.md "MSM plans")
    assert got["chunked"][2] != got["chunked"][3] and got["classic"][2] == got["classic"][3]
    assert got == COUNTS
