"""A proving-key handle gives back the device memory it took, on every path that makes or ends one."""
import ctypes
import json

import pytest

from conftest import golden_case
from oracle.py import bn254 as bn
from oracle.py import groth16 as g16

pytestmark = pytest.mark.gpu

ROUNDS = 8
# Rounds before the first reading. One is enough in a fresh process. Behind other tests it is not: the lanes' grow-only
# MSM workspaces are then still sized for those tests' keys, so the first round's proofs up to its first precompute (which
# gives the workspaces back) grow nothing, and it is the second round that sizes them for this key. Measured in the
# suite's order, with and without the owning members: one step of 2 MiB in the second round, flat for the seven after.
WARM_UP = 2


def _free_hbm(ctx):
    import torch
    ctx.synchronize()
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_key_handles_give_back_their_device_memory(ctx, zk, monkeypatch):
    """Every way a key handle comes and goes -- file load, block-cyclic split shards, device sections lent by the
    caller (whole and split), re-sharding a resident key + prove + fixed-base tables, the one-shot staged prove, a load
    that fails with its sections already resident -- run ROUNDS times after the warm-up rounds (lane workspaces, NTT
    tables, scan scratch, the one-shot entry point's own context): the free HBM the driver reports afterwards equals the
    reading before, to the byte. hipMalloc / hipFree hand out and take back whole allocations, so anything a handle
    kept, or freed twice, shows. Lent sections must come through untouched: a borrowed pointer is never freed."""
    import torch
    from zkpoa_amd.sharding import shard_range
    g = golden_case("n128")
    zkey, wtns, rs = g["circuit.zkey"], g["witness.wtns"], json.loads(g["rs.json"])
    r_, s_ = int(rs["r"]), int(rs["s"])
    monkeypatch.setenv("ZKPOA_R", rs["r"])
    monkeypatch.setenv("ZKPOA_S", rs["s"])
    monkeypatch.setenv("ZKPOA_KEY_CACHE", "0")
    monkeypatch.delenv("ZKPOA_OVERLAP", raising=False)
    secs = g16.read_binfile(zkey, "zkey", 2)
    sec = {sid: zkey[secs[sid][0][0]:secs[sid][0][0] + secs[sid][0][1]] for sid in (4, 5, 6, 7, 8, 9)}
    p5, _ = secs[5][0]
    bad = bytearray(zkey)
    bad[p5 + 32:p5 + 64] = bn.Q.to_bytes(32, "little")       # (test_out_of_range_field_elements_are_rejected's input)
    bad = bytes(bad)

    full = ctx.load_zkey(zkey)
    n_vars, n_public, domain, n_coefs = full.info()
    header = full.header()
    want, _ = ctx.prove(full, wtns, r_, s_)
    full.close()
    assert zk.proof_to_json(want) == g["proof_rapidsnark.json"]
    log_domain = domain.bit_length() - 1
    n_c = n_vars - n_public - 1

    def dev(b):
        return torch.frombuffer(bytearray(b if b else b"\0"), dtype=torch.uint8).cuda()

    # what a caller of zkpoa_zkey_load_device_shard holds: (rank, world, split) -> its ranges of sections 5-9, as tensors
    recs = dev(sec[4][4:])
    lent = {}
    for rank, world, split in ((0, 1, False), (0, 2, True), (1, 2, True)):
        (wlo, whi), (clo, chi) = shard_range(n_vars, rank, world), shard_range(n_c, rank, world)
        h = b"".join(sec[9][64 * t:64 * t + 64] for t in range(rank, domain, world)) if split else sec[9]
        host = [sec[5][64 * wlo:64 * whi], sec[6][64 * wlo:64 * whi], sec[7][128 * wlo:128 * whi], sec[8][64 * clo:64 * chi], h]
        lent[(rank, world, split)] = (host, [dev(b) for b in host])

    def one_shot(image):
        psz, usz = ctypes.c_ulong(1 << 12), ctypes.c_ulong(1 << 16)
        proof, public, err = (ctypes.create_string_buffer(psz.value), ctypes.create_string_buffer(usz.value),
                              ctypes.create_string_buffer(1024))
        rc = zk.lib().groth16_prover(image, len(image), wtns, len(wtns), proof, ctypes.byref(psz), public,
                                     ctypes.byref(usz), err, 1024)
        return rc, proof.value.decode(), err.value.decode()

    def one_round():
        ctx.load_zkey(zkey).close()
        for rank in range(2):
            ctx.load_zkey_shard_ex(zkey, rank, 2, split=True, block_log=4).close()
        for (rank, world, split), (host, tensors) in lent.items():
            key = ctx.load_zkey_device_shard(n_vars, n_public, log_domain, rank, world, split,
                                             *[t.data_ptr() for t in tensors], recs.data_ptr(), n_coefs, header)
            if world == 1:
                assert ctx.prove(key, wtns, r_, s_)[0] == want
            key.close()
            torch.cuda.synchronize()
            assert all(bytes(t.cpu().numpy()) == (b if b else b"\0") for b, t in zip(host, tensors)), \
                "a key handle wrote to, or freed, sections its caller lent it"
        key = ctx.load_zkey(zkey)
        key.set_shard_split(0, 2)
        assert key.precompute() > 0           # (a table over the cyclic H shard, which the next line replaces)
        key.set_shard_split(1, 2)
        key.set_shard(0, 1)                   # a whole key again
        assert ctx.prove(key, wtns, r_, s_)[0] == want
        assert key.precompute() > 0
        assert ctx.prove(key, wtns, r_, s_)[0] == want
        key.close()
        rc, proof, err = one_shot(zkey)
        assert rc == 0 and proof == g["proof_rapidsnark.json"], err
        rc, _, err = one_shot(bad)            # the staged load fails after the proof, every section resident
        assert rc == 1 and "coordinate is not a field element" in err
        with pytest.raises(zk.ZkpoaError, match="coordinate is not a field element"):
            ctx.load_zkey(bad)                # the plain load fails with sections 5-9 resident

    for _ in range(WARM_UP):
        one_round()
    before = _free_hbm(ctx)
    for _ in range(ROUNDS):
        one_round()
    after = _free_hbm(ctx)
    print("free HBM before %d, after %d rounds %d: delta %d bytes" % (before, ROUNDS, after, before - after))
    assert after == before
