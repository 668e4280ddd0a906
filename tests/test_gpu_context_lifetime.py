"""A context gives back what it took when it is closed, and one that cannot come up says why instead of ending the
process."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

_CHILD = """
import sys
sys.path.insert(0, %r)
import __graft_entry__ as entry
zk = entry.load_package()
try:
    zk.Context(0)
except zk.ZkpoaError as e:
    assert "ZKPOA_LANE_WORKSPACE_MAX_MB" in str(e), str(e)
    print("refused: " + str(e))
    sys.exit(0)
sys.exit(3)
"""


def test_a_context_that_cannot_come_up_returns_its_error(zk):
    """zkpoa_context_create reads the strict ZKPOA_LANE_WORKSPACE_MAX_MB after the device context, with its background
    thread, is up: a malformed value must come back as ZkpoaError naming the variable, and the half-built context must go
    without taking the process with it. In a child: a process that ended in std::terminate could not report anything."""
    rc = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _CHILD % ROOT],
                        env=dict(os.environ, ZKPOA_LANE_WORKSPACE_MAX_MB="lots"), capture_output=True, text=True)
    assert rc.returncode == 0, (rc.returncode, rc.stdout, rc.stderr)
    assert "refused: zkpoa_context_create: " in rc.stdout and "terminate called" not in rc.stderr


N_POINTS = 1 << 16   # by 0.6 to 0.9 KB of lane workspace per point: 39 MB or more for the one MSM of a cycle
WARM_UP, CYCLES = 2, 6
# Free HBM may fall by less than this over CYCLES cycles. Measured on the parent commit (profiles/context_lifetime.txt):
# a fall of 0 bytes over six cycles, so twice that, raised to the floor of 1 MiB -- a fortieth of one lost workspace.
MAX_FALL = 1 << 20


def test_closed_contexts_give_back_their_device_memory(zk):
    """Create a context, run a G1 MSM over 2^16 device-generated bases (a lane workspace, scan scratch, the pinned
    read-back), eight Poseidon pairs (the parameter tables) and an NTT at log_n = 10 (a plan's tables), close it. After
    two warm-up cycles six more may not lower the free HBM the driver reports by as much as MAX_FALL: one lost
    arena would be 39 MB a cycle. Results are pinned by other tests; here the MSM of one more cycle only has to give the
    first cycle's bytes."""
    import torch
    nr = np.random.default_rng(7)
    limbs = nr.integers(0, 1 << 63, size=(N_POINTS, 4), dtype=np.uint64)
    limbs[:, 3] &= np.uint64((1 << 60) - 1)
    d_scalars = torch.from_numpy(limbs.view(np.uint8).reshape(-1)).cuda()
    small = nr.integers(0, 1 << 62, size=(16 + 1024, 4), dtype=np.uint64)
    small[:, 3] &= np.uint64((1 << 60) - 1)
    left, right, coeffs = small[:8].tobytes(), small[8:16].tobytes(), small[16:].tobytes()
    d_bases = torch.empty(N_POINTS * 64, dtype=torch.uint8, device="cuda")

    def cycle():
        c = zk.Context(0)
        try:
            c.gen_bases_g1_device(12345, 67890, 0, N_POINTS, d_bases.data_ptr())
            got = c.msm_g1_device(d_bases.data_ptr(), d_scalars.data_ptr(), N_POINTS)
            assert len(c.poseidon2(left, right)) == 8 * 32
            assert len(c.ntt(coeffs, 10)) == 1024 * 32
        finally:
            c.close()
        return got

    def free_hbm():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    first = cycle()
    for _ in range(WARM_UP - 1):
        cycle()
    before = free_hbm()
    for _ in range(CYCLES):
        cycle()
    fall = before - free_hbm()
    print("free HBM fell by %d bytes over %d cycles" % (fall, CYCLES))
    assert fall < MAX_FALL, "free HBM fell by %d bytes over %d create/close cycles" % (fall, CYCLES)
    assert cycle() == first
