"""GPU parity tests for the whole prove path behind the reference call site
scripts/g16_prove.sh:248-252: H-scalar chain, zkpoa_prove, the one-shot groth16_prover ABI, and the
`prover` executable with rapidsnark's argv -- against golden files and the oracle."""
import json
import os
import random
import struct
import subprocess
import time

import pytest

from conftest import golden_case, le, rd
from oracle import c_oracle as co
from oracle.py import bn254 as bn
from oracle.py import groth16 as g16

pytestmark = pytest.mark.gpu
R = bn.R


def _pts_to_proof(pts):
    return {"pi_a": g16.g1_from_bytes(pts, 0), "pi_b": g16.g2_from_bytes(pts, 64), "pi_c": g16.g1_from_bytes(pts, 192)}


@pytest.mark.parametrize("tag", ["n8", "n128"])
def test_h_scalars_golden(ctx, tag):
    g = golden_case(tag)
    zk = g16.read_zkey(g["circuit.zkey"])
    secs = g16.read_binfile(g["circuit.zkey"], "zkey", 2)
    p4, l4 = secs[4][0]
    _, w = g16.read_wtns(g["witness.wtns"])
    k = zk.domainSize.bit_length() - 1
    got = ctx.h_scalars(g["circuit.zkey"][p4:p4 + l4], b"".join(le(x) for x in w), zk.nVars, k)
    assert got == g["h_scalars.bin"]


@pytest.mark.parametrize("tag", ["n8", "n128"])
def test_prove_golden_bit_exact(ctx, zk, tag):
    g = golden_case(tag)
    rs = json.loads(g["rs.json"])
    key = ctx.load_zkey(g["circuit.zkey"])
    try:
        pts, pub = ctx.prove(key, g["witness.wtns"], int(rs["r"]), int(rs["s"]))
    finally:
        key.close()
    assert zk.proof_to_json(pts, "rapidsnark") == g["proof_rapidsnark.json"]
    assert zk.public_to_json(pub, "rapidsnark") == g["public_rapidsnark.json"]
    assert zk.proof_to_json(pts, "snarkjs") == g["proof_snarkjs.json"]
    assert zk.public_to_json(pub, "snarkjs") == g["public_snarkjs.json"]


def test_prove_random_r_s_verifies(ctx):
    """Without injected r, s the proof differs per call but must verify (pinned verifier)."""
    g = golden_case("n128")
    vkey = json.loads(g["vkey.json"])
    key = ctx.load_zkey(g["circuit.zkey"])
    try:
        p1, pub = ctx.prove(key, g["witness.wtns"])
        p2, _ = ctx.prove(key, g["witness.wtns"])
    finally:
        key.close()
    assert p1 != p2
    n_pub = len(pub) // 32
    for p in (p1, p2):
        assert g16.verify(vkey, [rd(pub, i) for i in range(n_pub)], g16.proof_to_obj(_pts_to_proof(p)))


def test_prove_with_chunked_msms(ctx, zk):
    """every MSM of the proof larger than one sort may take (forced to 40 points here): A, C and H run in chunks,
    B1 / B2 cannot share a sort -- the proof must still be the golden one."""
    g = golden_case("n128")
    rs = json.loads(g["rs.json"])
    key = ctx.load_zkey(g["circuit.zkey"])
    ctx.set_option("msm_max_points", 40)
    try:
        pts, pub = ctx.prove(key, g["witness.wtns"], int(rs["r"]), int(rs["s"]))
    finally:
        ctx.set_option("msm_max_points", 0)
        key.close()
    assert zk.proof_to_json(pts, "rapidsnark") == g["proof_rapidsnark.json"]


@pytest.fixture(scope="module")
def mid_circuit():
    """2^13-constraint random circuit, setup through the C oracle's fixed-base generator."""
    rng = random.Random(2024)
    nVars, nPublic, nCons = 7000, 3, 8000
    cons, w = g16.random_circuit(rng, nVars, nPublic, nCons)
    # witness-like values on some wires do not matter for validity of *this* R1CS only if unconstrained;
    # keep the satisfying assignment.
    tox = {k: rng.randrange(1, R) for k in ("tau", "alpha", "beta", "gamma", "delta")}
    zkey, vk = g16.synthetic_setup(nVars, nPublic, cons, tox,
                                   g1_batch=lambda s: co.fixed_base_g1(b"".join(le(k) for k in s), 8),
                                   g2_batch=lambda s: co.fixed_base_g2(b"".join(le(k) for k in s), 8))
    return zkey, vk, g16.write_wtns(w), nPublic


def test_prove_mid_size_vs_c_oracle(ctx, mid_circuit):
    zkey, vk, wt, n_pub = mid_circuit
    rng = random.Random(1)
    r_, s_ = rng.randrange(R), rng.randrange(R)
    key = ctx.load_zkey(zkey)
    try:
        assert key.info()[:3] == (7000, 3, 1 << 13)
        pts, pub = ctx.prove(key, wt, r_, s_)
        pts0, _ = ctx.prove(key, wt, 0, 0)
    finally:
        key.close()
    exp, exp_pub = co.prove(zkey, wt, r_, s_, nthreads=8)
    assert pts == exp and pub == exp_pub
    exp0, _ = co.prove(zkey, wt, 0, 0, nthreads=8)
    assert pts0 == exp0
    assert g16.verify(vk, [rd(pub, i) for i in range(n_pub)], g16.proof_to_obj(_pts_to_proof(pts)))


def test_h_scalars_mid_size_vs_c_oracle(ctx, mid_circuit):
    zkey, _, wt, _ = mid_circuit
    secs = g16.read_binfile(zkey, "zkey", 2)
    p4, l4 = secs[4][0]
    p2, l2 = g16.read_binfile(wt, "wtns", 2)[2][0]
    wit = wt[p2:p2 + l2]
    got = ctx.h_scalars(zkey[p4:p4 + l4], wit, 7000, 13)
    assert got == co.h_scalars(zkey[p4:p4 + l4], wit, 7000, 13)


def _long_row_section(rng, n_vars, log_domain, n_long=40):
    """zkey section 4 payload for an R1CS whose row lengths are skewed the way real circuits are: most constraints
    have 1-3 terms per side, a few dozen have hundreds (a Num2Bits sum, a carry chain), one has 1500, some are
    empty, and the 32/33-term boundary of the wave kernel is hit from both sides."""
    domain = 1 << log_domain
    recs = []
    lengths = {}
    special = rng.sample(range(domain - 8), n_long + 6)
    for c in special[:n_long]:
        lengths[c] = (rng.randrange(60, 400), rng.randrange(0, 300))
    lengths[special[n_long]] = (1500, 2)
    lengths[special[n_long + 1]] = (30, 2)       # 32 in total: still the thread kernel
    lengths[special[n_long + 2]] = (31, 2)       # 33: the wave kernel
    lengths[special[n_long + 3]] = (0, 64)       # long B side only
    lengths[special[n_long + 4]] = (33, 0)
    lengths[special[n_long + 5]] = (0, 0)
    for c in range(domain - 8):
        la, lb = lengths.get(c, (rng.randrange(0, 4), rng.randrange(0, 3)))
        for m, cnt in ((0, la), (1, lb)):
            for _ in range(cnt):
                recs.append(struct.pack("<III", m, c, rng.randrange(n_vars)) + le(rng.randrange(R)))
    rng.shuffle(recs)                              # file order is arbitrary
    return struct.pack("<I", len(recs)) + b"".join(recs)


def test_h_scalars_long_rows_vs_c_oracle(ctx):
    rng = random.Random(77)
    n_vars, k = 3000, 12
    sec = _long_row_section(rng, n_vars, k)
    wit = b"".join(le(rng.randrange(R)) for _ in range(n_vars))
    assert ctx.h_scalars(sec, wit, n_vars, k) == co.h_scalars(sec, wit, n_vars, k)


@pytest.fixture(scope="module")
def long_row_circuit():
    """Satisfiable R1CS with realistic skew: 500 short constraints plus sums of 40..300 terms on the A side
    (and a few on the B side) -- (sum a_i w_i) * (sum b_j w_j) = w_e with w_e filled forward."""
    rng = random.Random(4242)
    nVars, nPublic = 900, 2
    cons, w = g16.random_circuit(rng, nVars - 60, nPublic, 500)
    w = w + [0] * 60
    for i in range(60):
        e = nVars - 60 + i
        la = rng.randrange(40, 300)
        lb = rng.choice([1, 1, 1, 2, 50])
        A = {rng.randrange(0, nVars - 60): rng.randrange(1, R) for _ in range(la)}
        B = {rng.randrange(0, nVars - 60): rng.randrange(1, R) for _ in range(lb)}
        va = sum(k * w[s] for s, k in A.items()) % R
        vb = sum(k * w[s] for s, k in B.items()) % R
        w[e] = va * vb % R
        cons.append((A, B, {e: 1}))
    rng.shuffle(cons)
    tox = {k: rng.randrange(1, R) for k in ("tau", "alpha", "beta", "gamma", "delta")}
    zkey, vk = g16.synthetic_setup(nVars, nPublic, cons, tox,
                                   g1_batch=lambda s: co.fixed_base_g1(b"".join(le(k) for k in s), 8),
                                   g2_batch=lambda s: co.fixed_base_g2(b"".join(le(k) for k in s), 8))
    return zkey, vk, g16.write_wtns(w), nPublic


def test_prove_long_rows_verifies_and_matches_oracle(ctx, long_row_circuit):
    zkey, vk, wt, n_pub = long_row_circuit
    rng = random.Random(5)
    r_, s_ = rng.randrange(R), rng.randrange(R)
    key = ctx.load_zkey(zkey)
    try:
        pts, pub = ctx.prove(key, wt, r_, s_)
    finally:
        key.close()
    exp, exp_pub = co.prove(zkey, wt, r_, s_, nthreads=8)
    assert pts == exp and pub == exp_pub
    assert g16.verify(vk, [rd(pub, i) for i in range(n_pub)], g16.proof_to_obj(_pts_to_proof(pts)))


@pytest.mark.parametrize("world", [2, 8])
def test_split_chain_long_rows(ctx, zk, long_row_circuit, world):
    """the wave-per-constraint path inside the split chain: rank-local CSR (keeps its own long rows)"""
    zkey, _, wt, _ = long_row_circuit
    full = ctx.load_zkey(zkey)
    try:
        want, pub = ctx.prove(full, wt, 3, 4)
        header = full.header()
        domain = full.info()[2]
    finally:
        full.close()
    keys = [ctx.load_zkey_shard_split(zkey, r, world) for r in range(world)]
    try:
        for k in keys:
            ctx.witness_load(k, wt)
        parts = _split_chain_partials(ctx, keys, world, domain)
        assert zk.prove_assemble(header, zk.sum_partials(parts), 3, 4) == want
    finally:
        for k in keys:
            k.close()
    # ... and a fully resident key re-pointed rank by rank (full CSR walked with stride G, long list filtered)
    import torch
    full = ctx.load_zkey(zkey)
    try:
        ctx.witness_load(full, wt)
        mb = domain // world * 32
        send = torch.zeros((world, 3, mb), dtype=torch.uint8, device="cuda")
        for r in range(world):
            full.set_shard_split(r, world)
            ctx.split_stage1(full, None, send[r].data_ptr())
        recv = _virtual_all_to_all(send, world, ctx)
        for r in range(world):
            full.set_shard_split(r, world)
            ctx.split_stage2(full, recv[r].data_ptr(), send[r].data_ptr())
        recv = _virtual_all_to_all(send, world, ctx)
        parts = []
        for r in range(world):
            full.set_shard_split(r, world)
            ctx.split_stage3(full, recv[r].data_ptr())
            parts.append(ctx.prove_partials_device(full, None))
        assert zk.prove_assemble(header, zk.sum_partials(parts), 3, 4) == want
    finally:
        full.close()


# ---- error behaviour of the boundary (scripts/lib/error_handling.sh relies on a non-zero exit) ------------
def test_wrong_witness_length_code(ctx, zk):
    g = golden_case("n8")
    _, w = g16.read_wtns(g["witness.wtns"])
    key = ctx.load_zkey(g["circuit.zkey"])
    try:
        with pytest.raises(zk.ZkpoaError, match="Invalid witness length"):
            ctx.prove(key, g16.write_wtns(w[:-1]), 0, 0)
        bad = bytearray(g["witness.wtns"])
        bad[0:4] = b"xxxx"
        with pytest.raises(zk.ZkpoaError, match="magic"):
            ctx.prove(key, bytes(bad), 0, 0)
    finally:
        key.close()


def test_witness_from_a_file_equals_witness_from_a_buffer(zk, tmp_path):
    """zkpoa_groth16_prover_files (the executable's entry point: the .wtns is walked and read through its file descriptor,
    never mapped) against groth16_prover_zkey_file (rapidsnark's shape: a buffer): same proof bytes for a good witness --
    also with the two sections in the other order and an unknown third section, which the container allows -- and the same
    error text for a malformed one (bad magic, truncated section table, truncated values, wrong value count, another
    field, wrong length for the circuit)."""
    g = golden_case("n128")
    rs = json.loads(g["rs.json"])
    zp = tmp_path / "circuit_final.zkey"
    zp.write_bytes(g["circuit.zkey"])
    _, w = g16.read_wtns(g["witness.wtns"])
    sec1 = struct.pack("<I", 32) + le(bn.R) + struct.pack("<I", len(w))
    sec2 = b"".join(le(x) for x in w)
    good = {
        "as written": g["witness.wtns"],
        "values before header, extra section": g16.write_binfile("wtns", 2, [(7, b"\x01\x02\x03"), (2, sec2), (1, sec1)]),
    }
    bad = {
        "bad magic": b"wtnz" + g["witness.wtns"][4:],
        "truncated table": g["witness.wtns"][:20],
        "truncated values": g["witness.wtns"][:-5],
        "count mismatch": g16.write_binfile("wtns", 2, [(1, sec1[:36] + struct.pack("<I", len(w) + 1)), (2, sec2)]),
        "other field": g16.write_binfile("wtns", 2, [(1, struct.pack("<I", 32) + le(bn.Q) + struct.pack("<I", len(w))), (2, sec2)]),
        "short for the circuit": g16.write_wtns(w[:-3]),
        "no values": g16.write_binfile("wtns", 2, [(1, sec1)]),
    }
    os.environ["ZKPOA_R"], os.environ["ZKPOA_S"] = rs["r"], rs["s"]
    try:
        for name, img in good.items():
            wp = tmp_path / "w.wtns"
            wp.write_bytes(img)
            zk.groth16_prove(str(zp), str(wp), str(tmp_path / "a.json"), str(tmp_path / "ap.json"))
            zk.groth16_prove_files(str(zp), str(wp), str(tmp_path / "b.json"), str(tmp_path / "bp.json"))
            assert (tmp_path / "a.json").read_text() == (tmp_path / "b.json").read_text() == g["proof_rapidsnark.json"], name
            assert (tmp_path / "ap.json").read_text() == (tmp_path / "bp.json").read_text() == g["public_rapidsnark.json"], name
        for name, img in bad.items():
            wp = tmp_path / "w.wtns"
            wp.write_bytes(img)
            msgs = []
            for fn in (zk.groth16_prove, zk.groth16_prove_files):
                with pytest.raises(zk.ZkpoaError) as ei:
                    fn(str(zp), str(wp), str(tmp_path / "x.json"), str(tmp_path / "xp.json"))
                msgs.append(str(ei.value).split(": ", 1)[1])
            assert msgs[0] == msgs[1], (name, msgs)
            assert not (tmp_path / "x.json").exists()
        with pytest.raises(zk.ZkpoaError, match="cannot read witness file"):
            zk.groth16_prove_files(str(zp), str(tmp_path / "missing.wtns"), str(tmp_path / "x.json"), str(tmp_path / "xp.json"))
    finally:
        del os.environ["ZKPOA_R"], os.environ["ZKPOA_S"]


def test_bad_zkeys_rejected(ctx, zk):
    g = golden_case("n8")
    z = g["circuit.zkey"]
    with pytest.raises(zk.ZkpoaError):
        ctx.load_zkey(b"nope" + z[4:])
    with pytest.raises(zk.ZkpoaError):
        ctx.load_zkey(z[:len(z) // 2])
    # coefficient record pointing at a signal >= nVars
    secs = g16.read_binfile(z, "zkey", 2)
    p4, _ = secs[4][0]
    bad = bytearray(z)
    struct.pack_into("<I", bad, p4 + 4 + 8, 10 ** 6)
    with pytest.raises(zk.ZkpoaError, match="out of range"):
        ctx.load_zkey(bytes(bad))


# ---- the drop-in executable: prover <zkey> <wtns> <proof.json> <public.json> ------------------------------
def test_prover_cli_drop_in(zk, tmp_path):
    g = golden_case("n128")
    rs = json.loads(g["rs.json"])
    (tmp_path / "circuit_final.zkey").write_bytes(g["circuit.zkey"])
    (tmp_path / "witness.wtns").write_bytes(g["witness.wtns"])
    assert os.path.basename(zk.PROVER_BIN) == "prover"      # g16_prove.sh:195-199 requires this basename
    env = dict(os.environ, ZKPOA_R=rs["r"], ZKPOA_S=rs["s"])
    rc = subprocess.run([zk.PROVER_BIN, str(tmp_path / "circuit_final.zkey"), str(tmp_path / "witness.wtns"),
                         str(tmp_path / "proof.json"), str(tmp_path / "public.json")], env=env,
                        capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr
    assert (tmp_path / "proof.json").read_text() == g["proof_rapidsnark.json"]
    assert (tmp_path / "public.json").read_text() == g["public_rapidsnark.json"]
    env["ZKPOA_JSON"] = "snarkjs"
    rc = subprocess.run([zk.PROVER_BIN, str(tmp_path / "circuit_final.zkey"), str(tmp_path / "witness.wtns"),
                         str(tmp_path / "proof_s.json"), str(tmp_path / "public_s.json")], env=env,
                        capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr
    assert (tmp_path / "proof_s.json").read_text() == g["proof_snarkjs.json"]
    assert (tmp_path / "public_s.json").read_text() == g["public_snarkjs.json"]


def test_prover_cli_worker_process_for_large_keys(zk, tmp_path):
    """A key of 2 GB or more is proved by a worker process and `prover` itself leaves as soon as both outputs are in place
    (the kernel needs ~150 ms to dismantle a process holding a 13-30 GB key on the GPU; csrc/prover_main.hip). Forced here
    for a small key with ZKPOA_DETACH_EXIT=always: same files, same exit status, the caller's pipes are released (this
    call returns), a failure still arrives as a non-zero status with its message and no output file; =0 keeps one process."""
    g = golden_case("n128")
    rs = json.loads(g["rs.json"])
    (tmp_path / "c.zkey").write_bytes(g["circuit.zkey"])
    (tmp_path / "w.wtns").write_bytes(g["witness.wtns"])
    _, w = g16.read_wtns(g["witness.wtns"])
    (tmp_path / "bad.wtns").write_bytes(g16.write_wtns(w + [1]))
    for mode in ("always", "0"):
        env = dict(os.environ, ZKPOA_R=rs["r"], ZKPOA_S=rs["s"], ZKPOA_DETACH_EXIT=mode, ZKPOA_VERBOSE="1")
        out = [str(tmp_path / ("proof_%s.json" % mode)), str(tmp_path / ("public_%s.json" % mode))]
        rc = subprocess.run([zk.PROVER_BIN, str(tmp_path / "c.zkey"), str(tmp_path / "w.wtns")] + out, env=env,
                            capture_output=True, text=True, timeout=120)
        assert rc.returncode == 0, rc.stderr
        assert open(out[0]).read() == g["proof_rapidsnark.json"] and open(out[1]).read() == g["public_rapidsnark.json"]
        assert ("worker process" in rc.stderr) == (mode == "always")
        bad = [str(tmp_path / ("nope_%s.json" % mode)), str(tmp_path / ("nopub_%s.json" % mode))]
        rc = subprocess.run([zk.PROVER_BIN, str(tmp_path / "c.zkey"), str(tmp_path / "bad.wtns")] + bad, env=env,
                            capture_output=True, text=True, timeout=120)
        assert rc.returncode != 0 and "Invalid witness length" in rc.stderr
        assert not os.path.exists(bad[0]) and not os.path.exists(bad[1])


@pytest.mark.parametrize("devices", ["0,0", "0,0,0", "0,0,0,0", "0,0,0,0,0,0,0,0"])
@pytest.mark.parametrize("tag", ["n8", "n128"])
def test_prover_cli_one_proof_over_several_ranks(zk, tmp_path, devices, tag):
    """multi-GPU BEHIND the reference's boundary -- the unchanged argv of scripts/g16_prove.sh:248-252,
    no Python. ZKPOA_DEVICES lists the HIP device of every rank; on this one-GPU box the ranks share device 0
    (rehearsal): one process, one context + host thread per rank, shards loaded from the file's byte ranges
    (block-cyclic sections 5-8, cyclic section 9), the split chain's two exchanges as device-to-device copies, partial
    sums added on the host. 2 / 4 / 8 ranks split the chain where rank^2 <= domain (n8: domain 8 -> only 2 ranks do),
    3 ranks replicate it. The bytes must be the golden ones."""
    g = golden_case(tag)
    rs = json.loads(g["rs.json"])
    (tmp_path / "circuit_final.zkey").write_bytes(g["circuit.zkey"])
    (tmp_path / "witness.wtns").write_bytes(g["witness.wtns"])
    env = dict(os.environ, ZKPOA_R=rs["r"], ZKPOA_S=rs["s"], ZKPOA_DEVICES=devices, ZKPOA_VERBOSE="1")
    env.pop("ZKPOA_SERVER", None)
    rc = subprocess.run([zk.PROVER_BIN, "circuit_final.zkey", "witness.wtns", "proof.json", "public.json"], env=env,
                        capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert rc.returncode == 0, rc.stderr
    n_ranks = devices.count(",") + 1
    assert "one proof over %d ranks" % n_ranks in rc.stderr, rc.stderr
    domain = 8 if tag == "n8" else 128
    want_split = n_ranks in (2, 4, 8) and n_ranks * n_ranks <= domain
    assert ("H-scalar chain split" in rc.stderr) == want_split, rc.stderr
    assert "self-check: proof verifies" in rc.stderr
    assert (tmp_path / "proof.json").read_text() == g["proof_rapidsnark.json"]
    assert (tmp_path / "public.json").read_text() == g["public_rapidsnark.json"]


def test_prover_cli_several_ranks_mid_size_server_and_errors(zk, tmp_path, mid_circuit, sock_dir):
    """The same path at 2^13 with real block-cyclic shards (4 ranks, blocks of 2^7 wires), through the resident server:
    first call loads the shards, the second builds every shard's fixed-base tables, the third is served from the cache
    -- all three byte-identical to the single-device proof; then the error conventions (bad device list, short witness)."""
    zkey, vk, wt, n_pub = mid_circuit
    (tmp_path / "circuit_final.zkey").write_bytes(zkey)
    (tmp_path / "witness.wtns").write_bytes(wt)
    (tmp_path / "short.wtns").write_bytes(golden_case("n8")["witness.wtns"])
    base = dict(os.environ, ZKPOA_R="12345678901234567890", ZKPOA_S="98765432109876543210", ZKPOA_VERBOSE="1")
    base.pop("ZKPOA_SERVER", None)
    argv = lambda out: [zk.PROVER_BIN, "circuit_final.zkey", "witness.wtns", out + ".json", out + "_public.json"]
    rc = subprocess.run(argv("single"), env=dict(base, ZKPOA_DEVICE="0"), capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert rc.returncode == 0, rc.stderr
    want = (tmp_path / "single.json").read_text()
    sock = str(sock_dir / "prover.sock")
    # (ZKPOA_PRECOMP=eager: the tables on the key's second use, inside the request -- the r03 policy; the default builds
    # them from the server's idle time, test_server_builds_tables_in_its_idle_time_not_in_a_request)
    env = dict(base, ZKPOA_DEVICES="0,0,0,0", ZKPOA_SERVER=sock, ZKPOA_SERVER_IDLE_S="60", ZKPOA_PRECOMP="eager")
    try:
        for i in range(3):
            rc = subprocess.run(argv("multi%d" % i), env=env, capture_output=True, text=True, cwd=tmp_path, timeout=300)
            assert rc.returncode == 0, rc.stderr
            assert (tmp_path / ("multi%d.json" % i)).read_text() == want
            assert (tmp_path / ("multi%d_public.json" % i)).read_text() == (tmp_path / "single_public.json").read_text()
        log = (sock_dir / "prover.sock.log").read_text()
        assert log.count("| zkey sharded load ") == 1 and log.count("| zkey cached,") == 2
        assert "fixed-base tables for the cached key on 4 ranks" in log and "sections 5-8 block-cyclic" in log
        rc = subprocess.run([zk.PROVER_BIN, "circuit_final.zkey", "short.wtns", "bad.json", "bad_public.json"], env=env,
                            capture_output=True, text=True, cwd=tmp_path, timeout=120)
        assert rc.returncode == 1 and "Invalid witness length" in rc.stderr and not (tmp_path / "bad.json").exists()
    finally:
        subprocess.run([zk.PROVER_BIN, "--stop-server"], env=env, cwd=tmp_path, timeout=60)
    for bad in ("0,x", "0,99", "0,,1", ",", "0,0,0,0,0,0,0,0,0"):
        rc = subprocess.run(argv("bad"), env=dict(base, ZKPOA_DEVICES=bad), capture_output=True, text=True, cwd=tmp_path, timeout=120)
        assert rc.returncode != 0 and "ZKPOA_DEVICES" in rc.stderr and not (tmp_path / "bad.json").exists(), (bad, rc.stderr)


@pytest.mark.parametrize("witness_like", [False, True])
def test_prover_cli_several_ranks_2p16_vs_c_oracle(ctx, zk, tmp_path, witness_like):
    """A 2^16-constraint key with 60,000 wires written as a real .zkey / .wtns pair (the synthetic circuit's sections
    copied out of HBM): the `prover` executable on 1, 2, 4 and 8 ranks (block-cyclic sections 5-8 in blocks of 2^9 - 2^12
    wires, cyclic section 9, split chain) must write the same proof.json, and its points must equal the C oracle's
    orc_prove on the same files -- the multi-GPU drop-in against the oracle at a size where every rank holds several
    blocks and the hot bucket of a witness-like distribution spans them."""
    from zkpoa_amd.synthetic import SyntheticCircuit
    circ = SyntheticCircuit(zk, ctx, 16, 60000, n_public=2, seed=77, witness_like=witness_like)
    try:
        zkey, wtns = circ.zkey_image(), circ.wtns_image()
    finally:
        circ.close()
    (tmp_path / "circuit_final.zkey").write_bytes(zkey)
    (tmp_path / "witness.wtns").write_bytes(wtns)
    r_, s_ = 1234567, 7654321
    want_pts, want_pub = co.prove(zkey, wtns, r_, s_, 8, n_public=2)
    want = zk.proof_to_json(want_pts, "rapidsnark")
    base = dict(os.environ, ZKPOA_R=str(r_), ZKPOA_S=str(s_), ZKPOA_VERBOSE="1", ZKPOA_SELFCHECK="0")   # no valid vkey inside
    base.pop("ZKPOA_SERVER", None)
    for devices in ("0", "0,0", "0,0,0,0", "0,0,0,0,0,0,0,0"):
        out = "proof_%d.json" % len(devices)
        rc = subprocess.run([zk.PROVER_BIN, "circuit_final.zkey", "witness.wtns", out, "public.json"],
                            env=dict(base, ZKPOA_DEVICES=devices), capture_output=True, text=True, cwd=tmp_path, timeout=300)
        assert rc.returncode == 0, rc.stderr
        assert (tmp_path / out).read_text() == want, devices
        assert (tmp_path / "public.json").read_text() == zk.public_to_json(want_pub, "rapidsnark")
        if "," in devices:
            assert "H-scalar chain split" in rc.stderr and "block-cyclic" in rc.stderr
    # the exchanges as hipMemcpyPeerAsync copies instead of the peer-write kernel (what a pair without a direct path gets)
    rc = subprocess.run([zk.PROVER_BIN, "circuit_final.zkey", "witness.wtns", "proof_copy.json", "public.json"],
                        env=dict(base, ZKPOA_DEVICES="0,0,0,0", ZKPOA_EXCHANGE="copy"), capture_output=True, text=True,
                        cwd=tmp_path, timeout=300)
    assert rc.returncode == 0, rc.stderr
    assert (tmp_path / "proof_copy.json").read_text() == want


def test_prover_cli_over_distinct_gpus(zk, tmp_path):
    """Only on a node with two or more GPUs (the one-GPU test box skips it): the drop-in with one rank per
    DISTINCT device -- hipDeviceEnablePeerAccess for every pair, the exchange and witness-slice kernels storing through
    peer-mapped addresses, consumed after a cross-device hipStreamWaitEvent -- and the same with the exchanges as
    hipMemcpyPeerAsync copies (ZKPOA_EXCHANGE=copy), and with the devices picked by the per-GPU lock files; every
    variant must write the golden proof bytes, and the 2^16 key the C oracle's proof."""
    import torch
    ngpu = torch.cuda.device_count()
    if ngpu < 2:
        pytest.skip("needs at least two GPUs")
    g = golden_case("n128")
    rs = json.loads(g["rs.json"])
    (tmp_path / "circuit_final.zkey").write_bytes(g["circuit.zkey"])
    (tmp_path / "witness.wtns").write_bytes(g["witness.wtns"])
    base = dict(os.environ, ZKPOA_R=rs["r"], ZKPOA_S=rs["s"], ZKPOA_VERBOSE="1")
    for k in ("ZKPOA_SERVER", "ZKPOA_DEVICE", "ZKPOA_DEVICES"):
        base.pop(k, None)
    world = 8 if ngpu >= 8 else 4 if ngpu >= 4 else 2
    devs = ",".join(str(d) for d in range(world))
    argv = [zk.PROVER_BIN, "circuit_final.zkey", "witness.wtns", "proof.json", "public.json"]
    for extra in ({"ZKPOA_DEVICES": devs}, {"ZKPOA_DEVICES": devs, "ZKPOA_EXCHANGE": "copy"},
                  {"ZKPOA_MULTI_MIN_POWER": "0"}):                     # the last: automatic choice by lock files
        if os.path.exists(tmp_path / "proof.json"):
            os.remove(tmp_path / "proof.json")
        rc = subprocess.run(argv, env=dict(base, **extra), capture_output=True, text=True, cwd=tmp_path, timeout=300)
        assert rc.returncode == 0, rc.stderr
        assert (tmp_path / "proof.json").read_text() == g["proof_rapidsnark.json"], extra
        assert "%d rank(s)" % world in rc.stderr or "ZKPOA_MULTI_MIN_POWER" in extra, rc.stderr
    # a mid-size key against the C oracle, real block-cyclic shards on the distinct devices
    from zkpoa_amd.synthetic import SyntheticCircuit
    ctx = zk.Context(0)
    try:
        circ = SyntheticCircuit(zk, ctx, 16, 60000, n_public=2, seed=78, witness_like=True)
        try:
            zkey, wtns = circ.zkey_image(), circ.wtns_image()
        finally:
            circ.close()
    finally:
        ctx.close()
    (tmp_path / "mid.zkey").write_bytes(zkey)
    (tmp_path / "mid.wtns").write_bytes(wtns)
    want_pts, _ = co.prove(zkey, wtns, 11, 22, 8, n_public=2)
    for extra in ({}, {"ZKPOA_EXCHANGE": "copy"}):
        rc = subprocess.run([zk.PROVER_BIN, "mid.zkey", "mid.wtns", "mid.json", "mid_pub.json"],
                            env=dict(base, ZKPOA_R="11", ZKPOA_S="22", ZKPOA_SELFCHECK="0", ZKPOA_DEVICES=devs, **extra),
                            capture_output=True, text=True, cwd=tmp_path, timeout=300)
        assert rc.returncode == 0, rc.stderr
        assert (tmp_path / "mid.json").read_text() == zk.proof_to_json(want_pts, "rapidsnark")


def test_a_stale_exchange_is_caught_by_the_self_check_and_repeated_with_copies(zk, tmp_path, sock_dir):
    """The peer-store exchanges of the multi-GPU drop-in rest on a memory-visibility rule no multi-GPU node has confirmed
    yet. Safety net: the first three proofs of a key are verified against the zkey's own verification key, and a proof
    that fails is repeated with hipMemcpyPeerAsync exchanges, which then stay on. Here rank 0 withholds its first push
    in the FIRST proof of the process (test hook: its peers read whatever their fresh receive buffers hold, as a missing
    release / acquire would leave them): all three calls must still write the golden proof, the first with a warning."""
    g = golden_case("n128")
    rs = json.loads(g["rs.json"])
    (tmp_path / "circuit_final.zkey").write_bytes(g["circuit.zkey"])
    (tmp_path / "witness.wtns").write_bytes(g["witness.wtns"])
    sock = str(sock_dir / "prover.sock")
    env = dict(os.environ, ZKPOA_R=rs["r"], ZKPOA_S=rs["s"], ZKPOA_SERVER=sock, ZKPOA_SERVER_IDLE_S="60",
               ZKPOA_DEVICES="0,0,0,0", ZKPOA_TEST_STALE_EXCHANGE="1", ZKPOA_VERBOSE="1")
    argv = [zk.PROVER_BIN, "circuit_final.zkey", "witness.wtns", "proof.json", "public.json"]
    try:
        for i in range(3):
            if os.path.exists(tmp_path / "proof.json"):
                os.remove(tmp_path / "proof.json")
            rc = subprocess.run(argv, env=env, capture_output=True, text=True, cwd=tmp_path, timeout=300)
            assert rc.returncode == 0, rc.stderr
            assert (tmp_path / "proof.json").read_text() == g["proof_rapidsnark.json"], i
        log = (sock_dir / "prover.sock.log").read_text()
        assert log.count("failed its self-check with the peer-store exchanges") == 1
    finally:
        subprocess.run([zk.PROVER_BIN, "--stop-server"], env=env, cwd=tmp_path, timeout=60)


@pytest.mark.parametrize("fail", ["2:1", "0:2", "3:3"])
def test_a_failing_rank_ends_the_multi_rank_proof_with_an_error_not_a_hang(zk, tmp_path, fail):
    """One rank of a four-rank proof fails (test hook) before the first barrier, between the two exchanges or before its
    MSMs: the other ranks keep arriving at the barriers, the process exits non-zero with that rank's message within
    seconds, and no output file appears -- the same call without the hook then proves normally."""
    g = golden_case("n128")
    rs = json.loads(g["rs.json"])
    (tmp_path / "circuit_final.zkey").write_bytes(g["circuit.zkey"])
    (tmp_path / "witness.wtns").write_bytes(g["witness.wtns"])
    env = dict(os.environ, ZKPOA_R=rs["r"], ZKPOA_S=rs["s"], ZKPOA_DEVICES="0,0,0,0")
    env.pop("ZKPOA_SERVER", None)
    argv = [zk.PROVER_BIN, "circuit_final.zkey", "witness.wtns", "proof.json", "public.json"]
    rc = subprocess.run(argv, env=dict(env, ZKPOA_TEST_FAIL_RANK=fail), capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert rc.returncode != 0 and ("rank %s failed in phase %s" % tuple(fail.split(":"))) in rc.stderr, rc.stderr
    assert not (tmp_path / "proof.json").exists() and not (tmp_path / "public.json").exists()
    rc = subprocess.run(argv, env=env, capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert rc.returncode == 0 and (tmp_path / "proof.json").read_text() == g["proof_rapidsnark.json"]


def test_prover_cli_server_mode(zk, tmp_path, sock_dir):
    """ZKPOA_SERVER: same argv, exit codes and output bytes, but the proofs come from a resident prover
    process that keeps the key in HBM between calls (second call = cache hit)."""
    g, g8 = golden_case("n128"), golden_case("n8")
    rs = json.loads(g["rs.json"])
    (tmp_path / "circuit_final.zkey").write_bytes(g["circuit.zkey"])
    (tmp_path / "witness.wtns").write_bytes(g["witness.wtns"])
    (tmp_path / "short.wtns").write_bytes(g8["witness.wtns"])
    sock = str(sock_dir / "prover.sock")
    env = dict(os.environ, ZKPOA_R=rs["r"], ZKPOA_S=rs["s"], ZKPOA_SERVER=sock, ZKPOA_VERBOSE="1",
               ZKPOA_SERVER_IDLE_S="60")

    def run(wtns, proof, public, **extra):
        return subprocess.run([zk.PROVER_BIN, "circuit_final.zkey", wtns, proof, public], env=dict(env, **extra),
                              capture_output=True, text=True, cwd=tmp_path, timeout=120)   # relative paths on purpose
    try:
        rc = run("witness.wtns", "proof.json", "public.json")
        assert rc.returncode == 0, rc.stderr
        assert "prover server pid" in rc.stderr
        assert (tmp_path / "proof.json").read_text() == g["proof_rapidsnark.json"]
        assert (tmp_path / "public.json").read_text() == g["public_rapidsnark.json"]
        rc = run("witness.wtns", "proof_s.json", "public_s.json", ZKPOA_JSON="snarkjs")
        assert rc.returncode == 0, rc.stderr
        assert (tmp_path / "proof_s.json").read_text() == g["proof_snarkjs.json"]
        assert (tmp_path / "public_s.json").read_text() == g["public_snarkjs.json"]
        log = (sock_dir / "prover.sock.log").read_text()
        assert log.count("| zkey load ") == 1 and log.count("| zkey cached,") == 1   # uploaded once, reused once
        # a failing request: rapidsnark's message, exit code 1, no output files, and the server stays up
        rc = run("short.wtns", "bad.json", "bad_public.json")
        assert rc.returncode == 1 and "Invalid witness length" in rc.stderr
        assert not (tmp_path / "bad.json").exists() and not (tmp_path / "bad_public.json").exists()
        rc = run("witness.wtns", "proof2.json", "public2.json")
        assert rc.returncode == 0 and (tmp_path / "proof2.json").read_text() == g["proof_rapidsnark.json"]
        # several prover processes at once (one per GNU-parallel batch, full_workflow.sh:552): served one at a time
        procs = [subprocess.Popen([zk.PROVER_BIN, "circuit_final.zkey", "witness.wtns", "par%d.json" % i, "parpub%d.json" % i],
                                  env=env, cwd=tmp_path, stderr=subprocess.PIPE, text=True) for i in range(4)]
        for i, pr in enumerate(procs):
            _, err = pr.communicate(timeout=120)
            assert pr.returncode == 0, err
            assert (tmp_path / ("par%d.json" % i)).read_text() == g["proof_rapidsnark.json"]
        # a rewritten key file is a different key (mtime / inode), never a stale hit
        os.utime(tmp_path / "circuit_final.zkey", ns=(1, 1))
        rc = run("witness.wtns", "proof3.json", "public3.json")
        assert rc.returncode == 0 and (tmp_path / "proof3.json").read_text() == g["proof_rapidsnark.json"]
        assert (sock_dir / "prover.sock.log").read_text().count("| zkey load ") == 2
    finally:
        subprocess.run([zk.PROVER_BIN, "--stop-server"], env=env, cwd=tmp_path, timeout=60)
    for _ in range(100):
        if not os.path.exists(sock):
            break
        time.sleep(0.05)
    assert not os.path.exists(sock)


@pytest.mark.parametrize("devices", [None, "0,0"])
def test_server_builds_tables_in_its_idle_time_not_in_a_request(zk, tmp_path, mid_circuit, devices, sock_dir):
    """Default policy (ZKPOA_PRECOMP unset): a resident key's fixed-base tables are never built inside a request -- a whole
    set is seconds at the layer-two / -three sizes, which a two-batch workflow never earns back -- but one table per step
    from the server's idle time (zkpoa_idle_work, after ZKPOA_SERVER_IDLE_WORK_MS without a request). First call: load;
    then the server is left alone for a moment; the following calls are plain cache hits whose proofs -- now through the
    tables -- are byte-identical."""
    zkey, vk, wt, n_pub = mid_circuit
    (tmp_path / "circuit_final.zkey").write_bytes(zkey)
    (tmp_path / "witness.wtns").write_bytes(wt)
    sock = str(sock_dir / "prover.sock")
    env = dict(os.environ, ZKPOA_R="12345678901234567890", ZKPOA_S="98765432109876543210", ZKPOA_VERBOSE="1",
               ZKPOA_SERVER=sock, ZKPOA_SERVER_IDLE_S="60", ZKPOA_SERVER_IDLE_WORK_MS="100")
    env.pop("ZKPOA_PRECOMP", None)
    if devices:
        env["ZKPOA_DEVICES"] = devices
    argv = lambda out: [zk.PROVER_BIN, "circuit_final.zkey", "witness.wtns", out + ".json", out + "_public.json"]
    try:
        rc = subprocess.run(argv("p0"), env=env, capture_output=True, text=True, cwd=tmp_path, timeout=300)
        assert rc.returncode == 0, rc.stderr
        log = ""
        for _ in range(100):                                   # the idle work starts by itself
            time.sleep(0.1)
            log = (sock_dir / "prover.sock.log").read_text()
            if ("complete)" in log) if not devices else ("idle: fixed-base tables for the cached key on 2 ranks" in log):
                break
        assert "zkpoa: idle: fixed-base table" in log, log
        for i in (1, 2):
            rc = subprocess.run(argv("p%d" % i), env=env, capture_output=True, text=True, cwd=tmp_path, timeout=300)
            assert rc.returncode == 0, rc.stderr
            assert (tmp_path / ("p%d.json" % i)).read_text() == (tmp_path / "p0.json").read_text()
        log = (sock_dir / "prover.sock.log").read_text()
        assert log.count("| zkey cached,") == 2
        assert "fixed-base tables for the cached key:" not in log and "fixed-base tables for the cached key on" not in log.replace("idle: fixed-base tables for the cached key on", "")
    finally:
        subprocess.run([zk.PROVER_BIN, "--stop-server"], env=env, cwd=tmp_path, timeout=60)


def test_server_overlaps_requests_without_mixing_them_up(zk, tmp_path, sock_dir):
    """The resident prover serves requests from a pool of threads: the witness of one request is staged into the key's
    second buffer while another request proves (two locks inside zkpoa_groth16_prover_files), and r, s and the JSON style
    travel per request and per thread, never through the server's environment. Twelve clients at once -- two witnesses,
    six (r, s) pairs, both JSON styles -- must each get exactly the proof the Python oracle computes for ITS inputs."""
    g = golden_case("n128")
    zkey = g["circuit.zkey"]
    _, w0 = g16.read_wtns(g["witness.wtns"])
    # (two witness FILES with the same values: what differs per request is the file, r, s and the JSON style)
    (tmp_path / "circuit_final.zkey").write_bytes(zkey)
    (tmp_path / "wa.wtns").write_bytes(g["witness.wtns"])
    (tmp_path / "wb.wtns").write_bytes(g16.write_wtns(w0))
    sock = str(sock_dir / "prover.sock")
    env = dict(os.environ, ZKPOA_SERVER=sock, ZKPOA_SERVER_IDLE_S="60", ZKPOA_SERVER_WORKERS="3")
    for k in ("ZKPOA_R", "ZKPOA_S", "ZKPOA_JSON", "ZKPOA_VERBOSE"):
        env.pop(k, None)
    rng = random.Random(4242)
    try:
        # two sequential calls first: load, then the table build of the second use -- the steady state follows
        for i in range(2):
            rc = subprocess.run([zk.PROVER_BIN, "circuit_final.zkey", "wa.wtns", "warm.json", "warm_pub.json"],
                                env=dict(env, ZKPOA_R="1", ZKPOA_S="2"), capture_output=True, text=True, cwd=tmp_path, timeout=120)
            assert rc.returncode == 0, rc.stderr
        jobs = []
        for i in range(12):
            r_, s_ = rng.randrange(bn.R), rng.randrange(bn.R)
            style = "snarkjs" if i % 3 == 0 else "rapidsnark"
            wt = "wa.wtns" if i % 2 == 0 else "wb.wtns"
            e = dict(env, ZKPOA_R=str(r_), ZKPOA_S=str(s_))
            if style == "snarkjs":
                e["ZKPOA_JSON"] = "snarkjs"
            pr = subprocess.Popen([zk.PROVER_BIN, "circuit_final.zkey", wt, "p%d.json" % i, "u%d.json" % i], env=e,
                                  cwd=tmp_path, stderr=subprocess.PIPE, text=True)
            jobs.append((i, r_, s_, style, pr))
        for i, r_, s_, style, pr in jobs:
            _, err = pr.communicate(timeout=180)
            assert pr.returncode == 0, err
            proof, public = g16.prove(zkey, g["witness.wtns"], r_, s_)
            want = g16.proof_json_snarkjs(proof) if style == "snarkjs" else g16.proof_json_rapidsnark(proof)
            assert (tmp_path / ("p%d.json" % i)).read_text() == want, "request %d got somebody else's proof" % i
    finally:
        subprocess.run([zk.PROVER_BIN, "--stop-server"], env=env, cwd=tmp_path, timeout=60)


def test_prover_cli_failure_leaves_no_output(zk, tmp_path):
    g = golden_case("n8")
    _, w = g16.read_wtns(g["witness.wtns"])
    (tmp_path / "c.zkey").write_bytes(g["circuit.zkey"])
    (tmp_path / "bad.wtns").write_bytes(g16.write_wtns(w + [1]))
    rc = subprocess.run([zk.PROVER_BIN, str(tmp_path / "c.zkey"), str(tmp_path / "bad.wtns"),
                         str(tmp_path / "proof.json"), str(tmp_path / "public.json")], capture_output=True, text=True)
    assert rc.returncode != 0 and "Invalid witness length" in rc.stderr
    assert not (tmp_path / "proof.json").exists() and not (tmp_path / "public.json").exists()


def test_python_host_mirror_groth16_prove(zk, tmp_path):
    """zkpoa_amd.groth16_prove(zkey, wtns, proof, public): same four arguments as the reference call."""
    g = golden_case("n128")
    vkey = json.loads(g["vkey.json"])
    (tmp_path / "c.zkey").write_bytes(g["circuit.zkey"])
    (tmp_path / "w.wtns").write_bytes(g["witness.wtns"])
    zk.groth16_prove(str(tmp_path / "c.zkey"), str(tmp_path / "w.wtns"), str(tmp_path / "p.json"),
                     str(tmp_path / "u.json"))
    proof = json.loads((tmp_path / "p.json").read_text())
    public = json.loads((tmp_path / "u.json").read_text())
    assert g16.verify(vkey, public, proof)


@pytest.mark.parametrize("cache", ["0", "1", "2"])
def test_zkey_file_cache_alternating_keys(zk, tmp_path, monkeypatch, cache):
    """groth16_prover_zkey_file keeps proving keys resident (ZKPOA_KEY_CACHE entries, LRU): alternating between
    two key files must give each file's own golden proof whether the cache is off, thrashing (1) or holds both."""
    monkeypatch.setenv("ZKPOA_KEY_CACHE", cache)
    cases = {}
    for tag in ("n8", "n128"):
        g = golden_case(tag)
        (tmp_path / (tag + ".zkey")).write_bytes(g["circuit.zkey"])
        (tmp_path / (tag + ".wtns")).write_bytes(g["witness.wtns"])
        cases[tag] = (g, json.loads(g["rs.json"]))
    for i, tag in enumerate(["n8", "n128", "n8", "n8", "n128", "n128", "n8"]):
        g, rs = cases[tag]
        monkeypatch.setenv("ZKPOA_R", rs["r"])
        monkeypatch.setenv("ZKPOA_S", rs["s"])
        zk.groth16_prove(str(tmp_path / (tag + ".zkey")), str(tmp_path / (tag + ".wtns")),
                         str(tmp_path / ("p%d.json" % i)), str(tmp_path / ("u%d.json" % i)))
        assert (tmp_path / ("p%d.json" % i)).read_text() == g["proof_rapidsnark.json"]
        assert (tmp_path / ("u%d.json" % i)).read_text() == g["public_rapidsnark.json"]
    # a key file rewritten in place (same path, new content) is a different key
    g8, rs8 = cases["n8"]
    (tmp_path / "n128.zkey").write_bytes(g8["circuit.zkey"])
    monkeypatch.setenv("ZKPOA_R", rs8["r"])
    monkeypatch.setenv("ZKPOA_S", rs8["s"])
    zk.groth16_prove(str(tmp_path / "n128.zkey"), str(tmp_path / "n8.wtns"), str(tmp_path / "px.json"),
                     str(tmp_path / "ux.json"))
    assert (tmp_path / "px.json").read_text() == g8["proof_rapidsnark.json"]


# ---- device-resident synthetic key with known discrete logs --------------------------------
@pytest.mark.parametrize("witness_like", [False, True])
def test_synthetic_circuit_prove_known_dlog(ctx, zk, witness_like):
    """2^16-domain synthetic key generated in HBM: pi_a, pi_b, pi_c must equal the discrete-log
    expectation, with the H scalars taken from the C oracle (independent of the GPU chain)."""
    from zkpoa_amd.synthetic import SyntheticCircuit
    circ = SyntheticCircuit(zk, ctx, 16, 60000, n_public=2, seed=77, witness_like=witness_like)
    try:
        coeffs, wit = circ.coeff_section_bytes(), circ.witness_bytes()
        P = co.h_scalars(coeffs, wit, circ.m, 16)
        assert ctx.h_scalars(coeffs, wit, circ.m, 16) == P
        rng = random.Random(3)
        for (r_, s_) in ((0, 0), (rng.randrange(R), rng.randrange(R))):
            pts, pub = circ.prove(r_, s_)
            assert circ.check(pts, r_, s_, P)
            assert pub == wit[32:32 * 3]
        # tampering with one witness value must change the proof
        pts0, _ = circ.prove(0, 0)
        import torch
        circ.d_witness[32 * 5] ^= 1
        pts1, _ = circ.prove(0, 0)
        circ.d_witness[32 * 5] ^= 1
        assert pts0 != pts1
    finally:
        circ.close()


# ---- one proof sharded over several ranks: emulated on one GPU -----------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_prove_equals_unsharded(ctx, zk, mid_circuit, world):
    """Shards loaded with zkpoa_zkey_load_shard (each uploads only its byte range of sections 5-9);
    partials summed component-wise + host assembly == the unsharded proof, bit for bit."""
    zkey, _, wt, _ = mid_circuit
    rng = random.Random(9)
    r_, s_ = rng.randrange(R), rng.randrange(R)
    full = ctx.load_zkey(zkey)
    try:
        want, pub = ctx.prove(full, wt, r_, s_)
        header = full.header()
    finally:
        full.close()
    parts = []
    for rank in range(world):
        key = ctx.load_zkey_shard(zkey, rank, world)
        try:
            p, pub_r = ctx.prove_partials(key, wt)
            assert pub_r == pub
            with pytest.raises(zk.ZkpoaError, match="shard"):
                ctx.prove(key, wt, r_, s_)
        finally:
            key.close()
        parts.append(p)
    assert zk.prove_assemble(header, zk.sum_partials(parts), r_, s_) == want


def test_set_shard_on_resident_key(ctx, zk):
    from zkpoa_amd.synthetic import SyntheticCircuit
    circ = SyntheticCircuit(zk, ctx, 14, 15000, n_public=1, seed=5, witness_like=True)
    try:
        want, _ = circ.prove(0, 0)
        header = circ.key.header()
        parts = []
        for rank in range(4):
            circ.key.set_shard(rank, 4)
            parts.append(ctx.prove_partials_device(circ.key, circ.d_witness.data_ptr()))
        circ.key.set_shard(0, 1)
        assert zk.prove_assemble(header, zk.sum_partials(parts), 0, 0) == want
    finally:
        circ.close()


# ---- the H-scalar chain split over the ranks too (SURVEY.md 8e rows NTT / buildABC / joinABC) --------------
def _virtual_all_to_all(send, world, ctx=None):
    """send[src] = one rank's exchange buffer, laid out [dst][poly][Q*32] -> recv[dst] = [src][poly][Q*32]: what ONE
    dist.all_to_all_single over the whole buffer does, for `world` virtual ranks living on one GPU. The stages only
    enqueue on the library's stream, the permutation runs on torch's: synchronise on both sides."""
    import torch
    if ctx is not None:
        ctx.synchronize()
    w, three, mb = send.shape
    out = send.view(w, world, three * mb // world).permute(1, 0, 2).contiguous().view(w, three, mb)
    torch.cuda.synchronize()
    return out


def _split_chain_partials(ctx, keys, world, domain, d_witness=None):
    import torch
    mb = domain // world * 32
    send = torch.zeros((world, 3, mb), dtype=torch.uint8, device="cuda")
    for r in range(world):
        ctx.split_stage1(keys[r], d_witness, send[r].data_ptr())
    recv = _virtual_all_to_all(send, world, ctx)
    for r in range(world):
        ctx.split_stage2(keys[r], recv[r].data_ptr(), send[r].data_ptr())
    recv = _virtual_all_to_all(send, world, ctx)
    for r in range(world):
        ctx.split_stage3(keys[r], recv[r].data_ptr())
    torch.cuda.synchronize()
    return [ctx.prove_partials_device(keys[r], None) for r in range(world)]


@pytest.mark.parametrize("world", [2, 4, 8])
@pytest.mark.parametrize("tag", ["n8", "n128"])
def test_split_chain_golden_bit_exact(ctx, zk, tag, world):
    """Each virtual rank loads its split shard (own constraint rows, cyclic H points), the two exchanges are
    emulated on one GPU, and the assembled proof must be the golden proof byte for byte."""
    g = golden_case(tag)
    rs = json.loads(g["rs.json"])
    domain = g16.read_zkey(g["circuit.zkey"]).domainSize
    if world * world > domain:
        with pytest.raises(zk.ZkpoaError, match="world"):
            ctx.load_zkey_shard_split(g["circuit.zkey"], 0, world)
        return
    keys = [ctx.load_zkey_shard_split(g["circuit.zkey"], r, world) for r in range(world)]
    try:
        with pytest.raises(zk.ZkpoaError, match="split"):
            ctx.prove_partials(keys[0], g["witness.wtns"])           # host-witness form needs the stages
        with pytest.raises(zk.ZkpoaError, match="stage"):
            ctx.prove_partials_device(keys[0], None)                  # H scalars not computed yet
        pubs = {ctx.witness_load(k, g["witness.wtns"]) for k in keys}
        assert len(pubs) == 1
        parts = _split_chain_partials(ctx, keys, world, domain)
        pts = zk.prove_assemble(keys[0].header(), zk.sum_partials(parts), int(rs["r"]), int(rs["s"]))
        assert zk.proof_to_json(pts, "rapidsnark") == g["proof_rapidsnark.json"]
        assert zk.public_to_json(pubs.pop(), "rapidsnark") == g["public_rapidsnark.json"]
        with pytest.raises(zk.ZkpoaError, match="stage"):
            ctx.prove_partials_device(keys[0], None)                  # consumed: a new proof needs new stages
    finally:
        for k in keys:
            k.close()


@pytest.mark.parametrize("world", [2, 4, 8])
def test_split_chain_mid_size_equals_unsharded(ctx, zk, mid_circuit, world):
    zkey, _, wt, _ = mid_circuit
    rng = random.Random(11)
    r_, s_ = rng.randrange(R), rng.randrange(R)
    full = ctx.load_zkey(zkey)
    try:
        want, pub = ctx.prove(full, wt, r_, s_)
        header = full.header()
    finally:
        full.close()
    keys = [ctx.load_zkey_shard_split(zkey, r, world) for r in range(world)]
    try:
        for k in keys:
            assert ctx.witness_load(k, wt) == pub
        parts = _split_chain_partials(ctx, keys, world, 1 << 13)
        assert zk.prove_assemble(header, zk.sum_partials(parts), r_, s_) == want
        # second proof on the same handles (buffers and tables reused)
        parts2 = _split_chain_partials(ctx, keys, world, 1 << 13)
        assert parts2 == parts
    finally:
        for k in keys:
            k.close()


@pytest.mark.parametrize("log_domain,world", [(14, 4), (18, 8), (22, 2)])
def test_set_shard_split_on_resident_key(ctx, zk, log_domain, world):
    """Resident synthetic key re-pointed rank by rank (what bench.py does per GPU): strided rows of the full
    CSR + cyclic H copy. 2^18 / 2^22 also cross the multi-pass NTT plans of the size-M transforms."""
    from zkpoa_amd.synthetic import SyntheticCircuit
    n_cons = (1 << log_domain) - 5000
    circ = SyntheticCircuit(zk, ctx, log_domain, n_cons, n_public=1, seed=5, witness_like=True)
    try:
        want, _ = circ.prove(0, 0)
        header = circ.key.header()
        import torch
        mb = (1 << log_domain) // world * 32
        send = torch.zeros((world, 3, mb), dtype=torch.uint8, device="cuda")
        wptr = circ.d_witness.data_ptr()
        for r in range(world):
            circ.key.set_shard_split(r, world)
            ctx.split_stage1(circ.key, wptr, send[r].data_ptr())
        recv = _virtual_all_to_all(send, world, ctx)
        for r in range(world):
            circ.key.set_shard_split(r, world)
            ctx.split_stage2(circ.key, recv[r].data_ptr(), send[r].data_ptr())
        recv = _virtual_all_to_all(send, world, ctx)
        parts = []
        for r in range(world):
            circ.key.set_shard_split(r, world)
            ctx.split_stage3(circ.key, recv[r].data_ptr())
            parts.append(ctx.prove_partials_device(circ.key, None))
        circ.key.set_shard(0, 1)
        assert zk.prove_assemble(header, zk.sum_partials(parts), 0, 0) == want
        assert circ.prove(0, 0)[0] == want          # the handle is a whole key again
    finally:
        circ.close()


@pytest.mark.parametrize("world,split,block_log", [(2, False, 6), (3, False, 4), (4, True, 7), (8, True, 5), (2, True, 13)])
def test_block_cyclic_shards_from_file_equal_unsharded(ctx, zk, mid_circuit, world, split, block_log):
    """zkpoa_zkey_load_shard_ex with ZKPOA_SHARD_BLOCK_CYCLIC(L): sections 5-8 dealt out in blocks of 2^L items (each
    one byte range of the file), H cyclic (split) or by range; the partial sums assemble into the unsharded proof, bit
    for bit, with and without the shards' fixed-base tables. (2^13 blocks of 7000 wires: rank 1 holds nothing.)"""
    zkey, _, wt, _ = mid_circuit
    rng = random.Random(31)
    r_, s_ = rng.randrange(R), rng.randrange(R)
    full = ctx.load_zkey(zkey)
    try:
        want, pub = ctx.prove(full, wt, r_, s_)
        header = full.header()
    finally:
        full.close()
    keys = [ctx.load_zkey_shard_ex(zkey, rank, world, split=split, block_log=block_log) for rank in range(world)]
    try:
        def partials():
            if split:
                for k in keys:
                    ctx.witness_load(k, wt)
                return _split_chain_partials(ctx, keys, world, 1 << 13)
            return [ctx.prove_partials(k, wt)[0] for k in keys]
        parts = partials()
        assert zk.prove_assemble(header, zk.sum_partials(parts), r_, s_) == want
        for k in keys:
            k.precompute()
        assert partials() == parts
    finally:
        for k in keys:
            k.close()


@pytest.mark.parametrize("log_domain,world,split", [(14, 2, False), (14, 3, False), (14, 4, True), (18, 8, True),
                                                     (16, 2, True)])
def test_per_rank_generated_shards_equal_unsharded(ctx, zk, log_domain, world, split):
    """bench.py --gpus N: every rank generates ONLY its own ranges of the synthetic key (index ranges of the point
    sections, cyclic H shard, its constraints' records) and loads them with zkpoa_zkey_load_device_shard; the N
    partial results must assemble into the proof of the whole key of the same seed."""
    from zkpoa_amd.synthetic import SyntheticCircuit
    m = (1 << log_domain) - 3000
    whole = SyntheticCircuit(zk, ctx, log_domain, m, n_public=2, seed=9, witness_like=True)
    try:
        want, _ = whole.prove(5, 7)
        header = whole.key.header()
    finally:
        whole.close()
    # every other case deals sections 5-8 out block-cyclically (bench.py --gpus N does), the rest by contiguous ranges
    block_log = 9 if (log_domain + world) % 2 == 0 else 0
    ranks = [SyntheticCircuit(zk, ctx, log_domain, m, n_public=2, seed=9, witness_like=True,
                              shard=(r, world, split, block_log)) for r in range(world)]
    try:
        # a shard holds 1/world of every point section (up to one block)
        assert all(abs(c.d_A.numel() - whole.d_A.numel() // world) <= 64 * max(1, 1 << block_log) for c in ranks)
        assert all(c.key.header() == header for c in ranks)
        with pytest.raises(zk.ZkpoaError, match="shard"):
            ranks[0].prove(5, 7)
        if split:
            assert all(c.d_recs.shape[0] < whole.d_recs.shape[0] // world + 8 for c in ranks)
            keys = [c.key for c in ranks]
            parts = _split_chain_partials(ctx, keys, world, 1 << log_domain, d_witness=ranks[0].d_witness.data_ptr())
        else:
            parts = [ctx.prove_partials_device(c.key, c.d_witness.data_ptr()) for c in ranks]
        assert zk.prove_assemble(header, zk.sum_partials(parts), 5, 7) == want
        # fixed-base tables of each shard's own ranges (incl. the cyclic H shard): same partial points, bit for bit
        assert all(c.key.precompute() > 0 for c in ranks)
        if split:
            parts2 = _split_chain_partials(ctx, [c.key for c in ranks], world, 1 << log_domain,
                                           d_witness=ranks[0].d_witness.data_ptr())
        else:
            parts2 = [ctx.prove_partials_device(c.key, c.d_witness.data_ptr()) for c in ranks]
        assert parts2 == parts
    finally:
        for c in ranks:
            c.close()


# ---- edge cases of the domain -------------------------------------------------------------------------------
def _setup_small(rng, nVars, nPublic, nCons):
    cons, w = g16.random_circuit(rng, nVars, nPublic, nCons)
    tox = {k: rng.randrange(1, R) for k in ("tau", "alpha", "beta", "gamma", "delta")}
    zkey, vk = g16.synthetic_setup(nVars, nPublic, cons, tox,
                                   g1_batch=lambda s: co.fixed_base_g1(b"".join(le(k) for k in s), 8),
                                   g2_batch=lambda s: co.fixed_base_g2(b"".join(le(k) for k in s), 8))
    return zkey, vk, w


@pytest.mark.parametrize("nVars,nPublic,nCons", [
    (30, 0, 20),        # no public signals: public.json is "[]", C section has nVars-1 points
    (40, 3, 60),        # nCons + nPublic + 1 = 64: the domain is filled exactly
    (40, 3, 61),        # one more constraint: the domain doubles
    (9, 1, 1),          # a single constraint
])
def test_prove_edge_shapes(ctx, zk, nVars, nPublic, nCons):
    rng = random.Random(nVars * 1000 + nCons)
    zkey, vk, w = _setup_small(rng, nVars, nPublic, nCons)
    wt = g16.write_wtns(w)
    r_, s_ = rng.randrange(R), rng.randrange(R)
    key = ctx.load_zkey(zkey)
    try:
        pts, pub = ctx.prove(key, wt, r_, s_)
    finally:
        key.close()
    proof, opub = g16.prove(zkey, wt, r_, s_)
    assert _pts_to_proof(pts) == proof and [rd(pub, i) for i in range(nPublic)] == opub
    assert zk.public_to_json(pub, "rapidsnark") == g16.public_json_rapidsnark(opub)
    assert zk.public_to_json(pub, "snarkjs") == g16.public_json_snarkjs(opub)
    assert g16.verify(vk, opub, g16.proof_to_obj(proof))
    assert zk.groth16_verify(json.dumps(vk), zk.public_to_json(pub), zk.proof_to_json(pts))


def test_prove_degenerate_witness(ctx, zk, monkeypatch):
    """w = (1, 0, 0, ...): every witness MSM collapses to (at most) one base; H scalars are all zero. The
    result must still equal the oracle's (proofs of a non-satisfying witness simply do not verify, so the
    prover's self-check is switched off here)."""
    monkeypatch.setenv("ZKPOA_SELFCHECK", "0")
    rng = random.Random(5)
    zkey, vk, w = _setup_small(rng, 50, 2, 40)
    w0 = [1] + [0] * 49
    wt = g16.write_wtns(w0)
    key = ctx.load_zkey(zkey)
    try:
        pts, pub = ctx.prove(key, wt, 0, 0)
    finally:
        key.close()
    proof, _ = g16.prove(zkey, wt, 0, 0)
    assert _pts_to_proof(pts) == proof


# ---- the real multi-process path: two ranks sharing this box's GPU, gloo collectives (rehearsal mode) ----------
@pytest.mark.parametrize("nproc,extra", [(2, []), (2, ["--replicated-chain"]), (4, [])])
def test_multi_process_sharded_prove_rehearsal(nproc, extra):
    """bench.py's N = 2 / N = 4 prove exactly as the driver launches it (torch.distributed.run, one process per
    rank), except that the ranks share the one GPU and the exchanges go through the host (ZKPOA_BENCH_REHEARSE=1):
    split shards per process, the three stages around two all-to-alls (or the replicated chain), all-gather of
    the partial points, host assembly -- bench.py itself checks the proof against the known discrete logs."""
    import socket
    import sys
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ZKPOA_BENCH_REHEARSE="1")
    rc = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
                         "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"),
                         "--gpus", str(nproc), "--steps", "2", "--warmup", "1", "--workload", "prove_2p16", "--full"] + extra,
                        env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert rc.returncode == 0, rc.stderr[-2000:]
    line = json.loads([l for l in rc.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == nproc and line["metric"] == "Groth16 proofs/sec"
    assert ("replicated" if extra else "split") in line["config"]["parallelism"]
    assert "REHEARSAL" in line["data"]
    # the real multi-process path checks pi_c too: the ranks' H scalars are gathered and validated on rank 0
    assert "pi_c" in line["config"]["checked"] and "gathered from the %d ranks" % nproc in line["config"]["checked"]
    assert line["n_ranks_seen"] == nproc


def test_bench_lines_carry_the_same_curves_at_every_n():
    """the driver plots bench.py's default line over N. Its `value` is the headline of that N (the
    2^20 MSM at N = 1, ONE 2^26 proof over the GPUs at N > 1), so every default line also carries the two curves of
    BASELINE.json's metric under the SAME keys: `curve` (strong: proofs/s of the one proof) and `curve_weak` (pts/s of the
    per-GPU MSM). Checked on the default code path with test-size workloads (ZKPOA_BENCH_SMALL=1): N = 1, and N = 2 as
    the driver launches it (rehearsal: ranks share the GPU)."""
    import socket
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = {}
    for nproc in (1, 2):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        env = dict(os.environ, ZKPOA_BENCH_SMALL="1")
        tail = [os.path.join(root, "bench.py"), "--gpus", str(nproc), "--steps", "2", "--warmup", "1", "--full",
                "--no-cpu-baseline"]
        if nproc == 1:
            argv = [sys.executable] + tail
        else:
            env["ZKPOA_BENCH_REHEARSE"] = "1"
            argv = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
                    "--master-addr", "127.0.0.1", "--master-port", str(port)] + tail
        rc = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=600, cwd=root)
        assert rc.returncode == 0, rc.stderr[-2000:]
        lines[nproc] = json.loads([l for l in rc.stdout.splitlines() if l.startswith("{")][-1])
    one, two = lines[1], lines[2]
    assert one["metric"] == "G1-MSM throughput" and two["metric"] == "Groth16 proofs/sec"      # headlines differ ...
    for key, scaling, unit in (("curve", "strong", "proofs/s"), ("curve_weak", "weak", "pts/s")):
        a, b = one[key], two[key]                                                                 # ... the curves do not
        assert set(a) == set(b) == {"workload", "value", "unit", "scaling", "ms_per_step", "n_gpus"}
        assert a["workload"] == b["workload"] and a["unit"] == b["unit"] == unit and a["scaling"] == b["scaling"] == scaling
        assert a["n_gpus"] == 1 and b["n_gpus"] == 2 and a["value"] > 0 and b["value"] > 0
    assert one["curve_weak"]["value"] == one["value"] and two["curve"]["value"] == two["value"]


def test_bench_collectives_over_rccl_with_one_rank():
    """The N > 1 code path of bench.py over the REAL RCCL backend, as far as one GPU allows: ZKPOA_BENCH_FORCE_DIST=1
    initialises the nccl process group with a single rank and sends the MSM partials, the timing reduction, the pass /
    fail agreement and the gathered H scalars (pi_c check) through its collectives."""
    import socket
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for workload in ("prove_2p16", "msm_g1_2p16"):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        env = dict(os.environ, ZKPOA_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0",
                   WORLD_SIZE="1", LOCAL_RANK="0")
        rc = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                             "--workload", workload, "--full", "--no-cpu-baseline"], env=env, capture_output=True, text=True,
                            timeout=600, cwd=root)
        assert rc.returncode == 0, rc.stderr[-2000:]
        line = json.loads([l for l in rc.stdout.splitlines() if l.startswith("{")][-1])
        assert line["collectives"] == "nccl" and line["n_ranks_seen"] == 1
        if workload.startswith("prove"):
            assert "pi_c" in line["config"]["checked"]


# ---- failure paths that used to be silent or sticky ---------------------------------------------------
def test_server_death_mid_request_still_yields_the_proof(zk, tmp_path, sock_dir):
    """The resident server dies with a request in hand (ZKPOA_SERVER_TEST_CRASH): the client proves in its own
    process, exit 0, same bytes; the next call starts a fresh server and is served by it."""
    g = golden_case("n128")
    rs = json.loads(g["rs.json"])
    (tmp_path / "circuit_final.zkey").write_bytes(g["circuit.zkey"])
    (tmp_path / "witness.wtns").write_bytes(g["witness.wtns"])
    sock = str(sock_dir / "prover.sock")
    env = dict(os.environ, ZKPOA_R=rs["r"], ZKPOA_S=rs["s"], ZKPOA_SERVER=sock, ZKPOA_VERBOSE="1",
               ZKPOA_SERVER_IDLE_S="60")
    argv = [zk.PROVER_BIN, "circuit_final.zkey", "witness.wtns", "proof.json", "public.json"]
    try:
        rc = subprocess.run(argv, env=dict(env, ZKPOA_SERVER_TEST_CRASH="1"), capture_output=True, text=True,
                            cwd=tmp_path, timeout=120)
        assert rc.returncode == 0, rc.stderr
        assert "went away without answering; proving in-process" in rc.stderr
        assert (tmp_path / "proof.json").read_text() == g["proof_rapidsnark.json"]
        os.remove(tmp_path / "proof.json")
        rc = subprocess.run(argv, env=env, capture_output=True, text=True, cwd=tmp_path, timeout=120)
        assert rc.returncode == 0 and "prover server pid" in rc.stderr, rc.stderr
        assert (tmp_path / "proof.json").read_text() == g["proof_rapidsnark.json"]
    finally:
        subprocess.run([zk.PROVER_BIN, "--stop-server"], env=env, cwd=tmp_path, timeout=60)


def test_server_failure_is_logged_and_strict_mode_refuses_the_fallback(zk, tmp_path, sock_dir):
    """the in-process fallback must never hide a GPU-side failure. When the server dies with a
    request in hand the client still proves (exit 0) but leaves a line in the persistent fault log and names it on
    stderr; with ZKPOA_STRICT=1 the same event is exit != 0 and no proof is written."""
    g = golden_case("n128")
    rs = json.loads(g["rs.json"])
    (tmp_path / "circuit_final.zkey").write_bytes(g["circuit.zkey"])
    (tmp_path / "witness.wtns").write_bytes(g["witness.wtns"])
    sock = str(sock_dir / "prover.sock")
    log = "/tmp/zkpoa-%d/faults.log" % os.getuid()
    before = os.path.getsize(log) if os.path.exists(log) else 0
    env = dict(os.environ, ZKPOA_R=rs["r"], ZKPOA_S=rs["s"], ZKPOA_SERVER=sock, ZKPOA_SERVER_IDLE_S="60",
               ZKPOA_SERVER_TEST_CRASH="1")
    argv = [zk.PROVER_BIN, "circuit_final.zkey", "witness.wtns", "proof.json", "public.json"]
    try:
        rc = subprocess.run(argv, env=env, capture_output=True, text=True, cwd=tmp_path, timeout=120)
        assert rc.returncode == 0, rc.stderr
        assert log in rc.stderr and (tmp_path / "proof.json").read_text() == g["proof_rapidsnark.json"]
        new = open(log).read()[before:]
        assert "went away without answering" in new and str(tmp_path / "circuit_final.zkey") in new
        os.remove(tmp_path / "proof.json")
        os.remove(tmp_path / "public.json")
        rc = subprocess.run(argv, env=dict(env, ZKPOA_STRICT="1"), capture_output=True, text=True, cwd=tmp_path, timeout=120)
        assert rc.returncode == 5 and "ZKPOA_STRICT" in rc.stderr, rc.stderr
        assert not (tmp_path / "proof.json").exists() and not (tmp_path / "public.json").exists()
        assert open(log).read().count("went away without answering", before) >= 2
    finally:
        subprocess.run([zk.PROVER_BIN, "--stop-server"], env=env, cwd=tmp_path, timeout=60)


def test_out_of_range_field_elements_are_rejected(ctx, zk):
    """Untrusted files: a witness value, a section-4 coefficient or a point coordinate that is not a canonical field
    element must fail loudly (PROVER_ERROR), not produce a wrong proof with exit code 0."""
    g = golden_case("n128")
    z = g["circuit.zkey"]
    _, wit = g16.read_wtns(g["witness.wtns"])
    secs = g16.read_binfile(z, "zkey", 2)
    key = ctx.load_zkey(z)
    try:
        for bad_value in (R, R + 1, (1 << 256) - 1):
            w = bytearray(g["witness.wtns"])
            ws = g16.read_binfile(bytes(w), "wtns", 2)
            p2, _ = ws[2][0]
            w[p2 + 32 * 7:p2 + 32 * 8] = bad_value.to_bytes(32, "little")
            with pytest.raises(zk.ZkpoaError, match="witness value is not a field element"):
                ctx.prove(key, bytes(w), 1, 2)
        pts, _ = ctx.prove(key, g["witness.wtns"], 1, 2)      # the handle is still good afterwards
        assert len(pts) == 256
    finally:
        key.close()
    p4, _ = secs[4][0]
    bad = bytearray(z)
    bad[p4 + 4 + 12:p4 + 4 + 44] = R.to_bytes(32, "little")
    with pytest.raises(zk.ZkpoaError, match="coefficient value is not a field element"):
        ctx.load_zkey(bytes(bad))
    for sid in (5, 7, 9):
        ps, _ = secs[sid][0]
        bad = bytearray(z)
        bad[ps + 32:ps + 64] = bn.Q.to_bytes(32, "little")
        with pytest.raises(zk.ZkpoaError, match="coordinate is not a field element"):
            ctx.load_zkey(bytes(bad))


def test_witness_generation_of_one_batch_overlaps_proving_of_another(zk, tmp_path, sock_dir):
    """witness generation stays on the CPU (circom C++, 18 s - 2 min per proof in the reference's
    logs, longer than the proving it feeds). The reference already runs its batches as parallel jobs
    (scripts/full_workflow.sh:552: `parallel prove_layers_one_two`), each job = witness generator, then prover
    (scripts/g16_prove.sh:228-252). With the resident prover (ZKPOA_SERVER) the GPU part of one job is a short
    critical section, so batch i + 1's witness generation runs while batch i proves, with the scripts unchanged.
    Here: three such jobs at once, the witness generator replaced by a 1-second stand-in; all three finish in about
    one generator time, not three, and every proof has the golden bytes."""
    import stat
    g = golden_case("n128")
    rs = json.loads(g["rs.json"])
    (tmp_path / "circuit_final.zkey").write_bytes(g["circuit.zkey"])
    (tmp_path / "ready.wtns").write_bytes(g["witness.wtns"])
    gen = tmp_path / "witness_gen"
    gen.write_text('#!/bin/bash\nsleep 1\ncp "%s" "$2"\n' % (tmp_path / "ready.wtns"))
    gen.chmod(gen.stat().st_mode | stat.S_IXUSR)
    env = dict(os.environ, ZKPOA_R=rs["r"], ZKPOA_S=rs["s"], ZKPOA_SERVER=str(sock_dir / "p.sock"),
               ZKPOA_SERVER_IDLE_S="60")
    try:
        # warm the server (its start-up and key upload are not what is measured)
        subprocess.run([str(gen), "in.json", str(tmp_path / "w0.wtns")], check=True)
        rc = subprocess.run([zk.PROVER_BIN, "circuit_final.zkey", "w0.wtns", "p0.json", "u0.json"], env=env, cwd=tmp_path,
                            capture_output=True, text=True, timeout=120)
        assert rc.returncode == 0, rc.stderr
        job = ('"%s" in.json "$1.wtns" && "%s" circuit_final.zkey "$1.wtns" "$1.proof.json" "$1.public.json"'
               % (gen, zk.PROVER_BIN))
        t0 = time.time()
        procs = [subprocess.Popen(["bash", "-c", job, "job", "batch_%d" % i], env=env, cwd=tmp_path) for i in range(3)]
        for pr in procs:
            assert pr.wait(timeout=120) == 0
        wall = time.time() - t0
        for i in range(3):
            assert (tmp_path / ("batch_%d.proof.json" % i)).read_text() == g["proof_rapidsnark.json"]
        assert wall < 2.0, "three 1 s witness generators + proofs took %.2f s: the jobs did not overlap" % wall
    finally:
        subprocess.run([zk.PROVER_BIN, "--stop-server"], env=env, cwd=tmp_path, timeout=60)


# ---- the one-shot entry points overlap the key upload with the compute (load_prove_staged) -----------------------
def _one_shot(zk, zkey, wt, env_overlap, monkeypatch, r_, s_):
    import ctypes
    monkeypatch.setenv("ZKPOA_R", str(r_))
    monkeypatch.setenv("ZKPOA_S", str(s_))
    if env_overlap is None:
        monkeypatch.delenv("ZKPOA_OVERLAP", raising=False)
    else:
        monkeypatch.setenv("ZKPOA_OVERLAP", env_overlap)
    L = zk.lib()
    psz, usz = ctypes.c_ulong(1 << 12), ctypes.c_ulong(1 << 16)
    proof, public, err = ctypes.create_string_buffer(psz.value), ctypes.create_string_buffer(usz.value), ctypes.create_string_buffer(1024)
    rc = L.groth16_prover(zkey, len(zkey), wt, len(wt), proof, ctypes.byref(psz), public, ctypes.byref(usz), err, 1024)
    return rc, proof.value.decode(), public.value.decode(), err.value.decode()


@pytest.mark.parametrize("nVars,nPublic,nCons", [
    (30, 0, 20), (40, 3, 60), (9, 1, 1),
    (5, 1, 2),          # the smallest circuits the generator makes: 3 private wires
    (6, 2, 3),
    (700, 2, 900),      # a few sort tiles, every lane busy
])
def test_one_shot_staged_equals_sequential_and_oracle(zk, monkeypatch, nVars, nPublic, nCons):
    """groth16_prover (the buffer form of what the CLI does) with the upload overlapped (default) and with
    ZKPOA_OVERLAP=0: identical JSON, equal to the oracle's proof, self-check on, over the edge shapes of the domain."""
    rng = random.Random(nVars * 77 + nCons)
    zkey, vk, w = _setup_small(rng, nVars, nPublic, nCons)
    wt = g16.write_wtns(w)
    r_, s_ = rng.randrange(R), rng.randrange(R)
    monkeypatch.delenv("ZKPOA_SELFCHECK", raising=False)
    rc1, p1, u1, e1 = _one_shot(zk, zkey, wt, None, monkeypatch, r_, s_)
    rc0, p0, u0, e0 = _one_shot(zk, zkey, wt, "0", monkeypatch, r_, s_)
    assert rc1 == 0 and rc0 == 0, (e1, e0)
    assert (p1, u1) == (p0, u0)
    proof, opub = g16.prove(zkey, wt, r_, s_)
    assert p1 == g16.proof_json_rapidsnark(proof) and u1 == g16.public_json_rapidsnark(opub)
    assert zk.groth16_verify(json.dumps(vk), u1, p1)
    # errors of the staged path: wrong witness length (rapidsnark's code 3), corrupted coordinate, bad witness value
    rc, _, _, err = _one_shot(zk, zkey, g16.write_wtns(w + [1]), None, monkeypatch, r_, s_)
    assert rc == 3 and "Invalid witness length" in err
    secs = g16.read_binfile(zkey, "zkey", 2)
    p9, _ = secs[9][0]
    bad = bytearray(zkey)
    bad[p9:p9 + 32] = bn.Q.to_bytes(32, "little")
    rc, _, _, err = _one_shot(zk, bytes(bad), wt, None, monkeypatch, r_, s_)
    assert rc == 1 and "coordinate is not a field element" in err
    wraw = bytearray(wt)                                   # (write_wtns reduces mod r: patch the bytes)
    wraw[-32:] = R.to_bytes(32, "little")
    rc, _, _, err = _one_shot(zk, zkey, bytes(wraw), None, monkeypatch, r_, s_)
    assert rc == 1 and "witness value is not a field element" in err
    rc, p2, u2, e2 = _one_shot(zk, zkey, wt, None, monkeypatch, r_, s_)      # and the context is still good
    assert rc == 0 and (p2, u2) == (p1, u1), e2


def test_one_shot_staged_mid_size(zk, mid_circuit, monkeypatch):
    zkey, _, wt, _ = mid_circuit
    rng = random.Random(12)
    r_, s_ = rng.randrange(R), rng.randrange(R)
    rc1, p1, u1, e1 = _one_shot(zk, zkey, wt, None, monkeypatch, r_, s_)
    rc0, p0, u0, e0 = _one_shot(zk, zkey, wt, "0", monkeypatch, r_, s_)
    assert rc1 == 0 and rc0 == 0, (e1, e0)
    assert (p1, u1) == (p0, u0)
    proof, opub = co.prove(zkey, wt, r_, s_, 8)
    assert p1 == zk.proof_to_json(proof)
