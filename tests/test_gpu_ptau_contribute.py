"""`snarkjs powersoftau new / contribute / beacon` and the section 7 check of `powersoftau verify` on the device
(csrc/ptau_contribute.hip, csrc/ptau_contribute.hip.h, csrc/phase1.hpp; C ABI zkpoa_scalar_mul_each_device,
zkpoa_power_scalars_device, zkpoa_compressed_form, zkpoa_ptau_new / _contribute / _beacon / _contributions).

Every expected byte comes from the oracle or from tests/phase1_ref.py (written from DESIGN.md "Phase-1 transcript"), never
from the code under test: the sections of a contributed file are `setup_files.write_ptau` of the multiplied secrets, the
records are phase1_ref's. Every comparison is exact."""
import os
import random
import struct
import subprocess

import pytest

import phase1_ref as p1
import setup_files as sf
from conftest import le
from oracle import c_oracle as co
from oracle.py import bn254 as bn
from oracle.py import groth16 as g16
from test_gpu_ptau_verify import _g1_double, _g2_double, _offsets, _patch, _rebuild

pytestmark = pytest.mark.gpu
R, Q = bn.R, bn.Q
CONTRIBUTIONS = 0x200
EDGE_SCALARS = [0, 1, 2, R - 1, R - 2, 1 << 253, 1 << 128, (1 << 128) - 1]
BEACON, BEACON_EXP = bytes.fromhex("0102030405060708090a"), 4
S_ENV = (0x1234567, R - 3, 98765432123456789)


def _fb(group, ks):
    data = b"".join(le(k % R) for k in ks)
    return co.fixed_base_g1(data, 8) if group == 1 else co.fixed_base_g2(data, 8)


def _dev(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def _mul_each(ctx, group, points, scalars, in_place=False):
    unit = 64 * group
    n = len(points) // unit
    d_p, d_k = _dev(points), _dev(b"".join(le(k) for k in scalars))
    d_o = d_p if in_place else _dev(bytes(len(points)))
    ctx.scalar_mul_each(group, d_p.data_ptr(), d_k.data_ptr(), n, d_o.data_ptr())
    return d_o.cpu().numpy().tobytes()


def _expected_mul(group, points, scalars):
    unit = 64 * group
    rd, wr, mul = ((g16.g1_from_bytes, g16.g1_to_bytes, bn.g1_mul) if group == 1 else
                   (g16.g2_from_bytes, g16.g2_to_bytes, bn.g2_mul))
    out = []
    for i, k in enumerate(scalars):
        P = rd(points, unit * i)
        out.append(wr(None if P is None or k % R == 0 else mul(P, k)))
    return b"".join(out)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_scalar_mul_each_matches_oracle(ctx, group, n):
    """One workgroup is 64 points (kMulEachThreads) and one inversion run 16: 63, 64, 65 straddle the first, 257 is five
    workgroups and seventeen runs. The forced scalars rotate through the lanes; the points include infinity and the
    generator; a zero scalar and a point at infinity give the all-zero point."""
    rng = random.Random(100 * group + n)
    logs = [rng.randrange(1, R) for _ in range(n)]
    scalars = [rng.randrange(R) for _ in range(n)]
    for i in range(n):
        if i % 3 == 0:
            scalars[i] = EDGE_SCALARS[(i // 3 + n) % len(EDGE_SCALARS)]
    if n == 1:
        logs, scalars = [1], [R - 1]
    else:
        logs[1], logs[n - 1] = 0, 1                                  # infinity, the generator
        logs[n // 2] = 0
        scalars[n // 2] = rng.randrange(1, R)                        # infinity times a full-width scalar
    points = _fb(group, logs)
    want = _expected_mul(group, points, scalars)
    assert _mul_each(ctx, group, points, scalars) == want
    assert _mul_each(ctx, group, points, scalars, in_place=True) == want
    assert want == _fb(group, [a * k for a, k in zip(logs, scalars)])   # the two oracles agree


def test_scalar_mul_each_every_edge_scalar_on_one_point(ctx):
    """Each forced scalar on the generator and on a random point, both groups; k = 2 meets the doubling inside the table."""
    for group in (1, 2):
        logs = [1, 0x1234567890abcdef] * len(EDGE_SCALARS)
        scalars = [k for k in EDGE_SCALARS for _ in range(2)]
        points = _fb(group, logs)
        assert _mul_each(ctx, group, points, scalars) == _expected_mul(group, points, scalars)


def test_scalar_mul_each_1000_random_pairs(ctx):
    rng = random.Random(77)
    logs = [rng.randrange(1, R) for _ in range(1000)]
    scalars = [rng.randrange(R) for _ in range(1000)]
    points = _fb(1, logs)
    assert _mul_each(ctx, 1, points, scalars) == _expected_mul(1, points, scalars)


@pytest.mark.parametrize("group", [1, 2])
def test_scalar_mul_each_across_slab_borders(ctx, group):
    """Above 2^20 points a call runs in several launches (slabs), each with its own offset into the points, the scalars
    and the output. Option ptau_mul_slab forces a slab of 100 points: 257 points are three launches, the last of 57, and
    100 is no multiple of the 64 points of a workgroup nor of the 16 of an inversion run. The same bytes as one launch."""
    rng = random.Random(300 + group)
    logs = [rng.randrange(R) for _ in range(257)]
    scalars = [rng.randrange(R) for _ in range(257)]
    points = _fb(group, logs)
    want = _fb(group, [a * k for a, k in zip(logs, scalars)])
    ctx.set_option("ptau_mul_slab", 100)
    try:
        assert _mul_each(ctx, group, points, scalars) == want
        assert _mul_each(ctx, group, points, scalars, in_place=True) == want
    finally:
        ctx.set_option("ptau_mul_slab", 0)
    assert _mul_each(ctx, group, points, scalars) == want


def test_scalar_mul_each_refuses_a_scalar_of_r(ctx, zk):
    points = _fb(1, [5, 6])
    with pytest.raises(zk.ZkpoaError, match="below r"):
        _mul_each(ctx, 1, points, [3, R])
    with pytest.raises(zk.ZkpoaError):
        ctx.scalar_mul_each(3, 0, 0, 0, 0)


@pytest.mark.parametrize("i0,n", [(0, 1), (0, 300), (255, 2), ((1 << 33) + 5, 70), (2047, 2050)])
def test_power_scalars_match_python(ctx, i0, n):
    """A workgroup makes 2048 scalars (256 threads x 8): (2047, 2050) crosses two workgroup borders with an i0 that is no
    multiple of anything, (2^33 + 5, 70) needs the exponent's upper word."""
    import torch
    rng = random.Random(i0 % 1000 + n)
    for ratio in (1, R - 1, rng.randrange(2, R)):
        for first in (0, rng.randrange(1, R)):
            d = torch.zeros(32 * n + 32, dtype=torch.uint8).cuda()
            ctx.power_scalars(first, ratio, i0, n, d.data_ptr())
            got = d.cpu().numpy().tobytes()
            want = b"".join(le(first * pow(ratio, i0 + i, R) % R) for i in range(n))
            assert got[:32 * n] == want, (ratio, first)
            assert got[32 * n:] == bytes(32)                          # nothing past the end


@pytest.mark.parametrize("group", [1, 2])
def test_compressed_form_matches_reference_across_pieces(ctx, group):
    rng = random.Random(group)
    logs = [1, R - 1, 0] + [rng.randrange(1, R) for _ in range(34)]
    points = _fb(group, logs)
    unit = 64 * group
    rd, comp = (g16.g1_from_bytes, p1.compress_g1) if group == 1 else (g16.g2_from_bytes, p1.compress_g2)
    want = b"".join(comp(rd(points, unit * i)) for i in range(len(logs)))
    one_piece = ctx.compressed_form(group, points)
    assert one_piece[0] == want and one_piece[1] == p1.blake2b(want)
    # a piece holds piece_points G2 points or twice as many G1 points: 37 points cross three pieces
    pp = 13 if group == 2 else 7
    assert ctx.compressed_form(group, points, pp) == one_piece
    signs = {want[(unit // 2) * i] & 0xc0 for i in range(len(logs))}
    assert signs == {0x00, 0x80, 0x40}                                # both signs and infinity occur


def test_compressed_form_of_a_g2_point_with_real_y(ctx):
    """y.c1 = 0: the sign is c0's. The conversion reads coordinates, so the points need not be on the curve."""
    pts = [((7, 9), (5, 0)), ((7, 9), (Q - 5, 0)), ((7, 9), (Q - 5, 1)), ((7, 9), (5, Q - 1)), ((0, 0), (0, 1))]
    data = b"".join(g16.g2_to_bytes(P) for P in pts)
    assert ctx.compressed_form(2, data)[0] == b"".join(p1.compress_g2(P) for P in pts)
    assert [p1.compress_g2(P)[0] for P in pts] == [0, 0x80, 0, 0x80, 0]


# ---- the commands -----------------------------------------------------------------------------------------------------
class _Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _s_env():
    return _Env(ZKPOA_PHASE1_S=",".join([hex(S_ENV[0]), str(S_ENV[1]), str(S_ENV[2])]))


def _secrets(power):
    rng = random.Random(9000 + power)
    return tuple(rng.randrange(1, R) for _ in range(3))


_chains = {}


def _chain(ctx, tmp_path_factory, power):
    """new -> contribute -> beacon -> prepare phase2, once per power: the paths and bytes of every step."""
    if power in _chains:
        return _chains[power]
    d = tmp_path_factory.mktemp("ptau%d" % power)
    c = {"dir": d, "x1": _secrets(power)}
    paths = {k: str(d / (k + ".ptau")) for k in ("new", "contributed", "beaconed", "prepared")}
    ctx.ptau_new(power, paths["new"])
    with _s_env():
        ctx.ptau_contribute(paths["new"], paths["contributed"], c["x1"], name="first")
    ctx.ptau_beacon(paths["contributed"], paths["beaconed"], BEACON, BEACON_EXP, name="the beacon")
    ctx.ptau_prepare_phase2(paths["beaconed"], paths["prepared"])
    c["paths"] = paths
    c["bytes"] = {k: open(p, "rb").read() for k, p in paths.items()}
    c["x2"], c["s2"] = p1.beacon_secrets(BEACON, BEACON_EXP)
    c["want1"] = sf.write_ptau(power, *c["x1"])
    c["want2"] = sf.write_ptau(power, *[a * b % R for a, b in zip(c["x1"], c["x2"])])
    _chains[power] = c
    return c


def _sec(buf, t):
    off, ln = _offsets(buf)[t]
    return buf[off:off + ln]


@pytest.mark.parametrize("power", [1, 3, 5])
def test_new_contribute_beacon_prepare_verify(ctx, tmp_path_factory, power):
    c = _chain(ctx, tmp_path_factory, power)
    n = 1 << power
    new = c["bytes"]["new"]
    assert sorted(_offsets(new)) == [1, 2, 3, 4, 5, 6, 7]
    G1, G2 = g16.g1_to_bytes(bn.G1_GEN), g16.g2_to_bytes(bn.G2_GEN)
    assert [_sec(new, t) for t in range(2, 8)] == [G1 * (2 * n - 1), G2 * n, G1 * n, G1 * n, G2, struct.pack("<I", 0)]
    assert _sec(new, 1) == _sec(c["want1"], 1)
    for t in range(1, 7):
        assert _sec(c["bytes"]["contributed"], t) == _sec(c["want1"], t), t
    for t in range(2, 7):
        assert _sec(c["bytes"]["beaconed"], t) == _sec(c["want2"], t), t
    prepared = c["bytes"]["prepared"]
    for t in (13, 14, 15):
        assert _sec(prepared, t) == _sec(c["want2"], t), t
    # section 12: levels 0..power as write_ptau; its top level needs tau^(2N-1), which no file holds (tests/test_gpu_ptau_prepare.py)
    low = 64 * ((2 << power) - 1)
    assert _sec(prepared, 12)[:low] == _sec(c["want2"], 12)[:low] and len(_sec(prepared, 12)) == len(_sec(c["want2"], 12))
    assert ctx.ptau_verify(c["paths"]["prepared"]) == (0, (power, power, 1, 2))
    assert ctx.ptau_verify(c["paths"]["contributed"]) == (0, (power, power, 0, 1))
    assert ctx.ptau_verify(c["paths"]["new"]) == (0, (power, power, 0, 0))


@pytest.mark.parametrize("power", [1, 3, 5])
def test_section7_equals_the_reference(ctx, zk, tmp_path_factory, power):
    c = _chain(ctx, tmp_path_factory, power)
    secs1, _ = p1.read_sections(c["want1"])
    secs2, _ = p1.read_sections(c["want2"])
    ss = [bn.g1_mul(bn.G1_GEN, s) for s in S_ENV]
    r1 = p1.next_record(p1.fresh_challenge(power), secs1, c["x1"], ss, 0, b"first")
    assert _sec(c["bytes"]["contributed"], 7) == p1.section7([r1])
    r2 = p1.next_record(r1.next_challenge, secs2, c["x2"], c["s2"], 1, b"the beacon", BEACON_EXP, BEACON)
    want7 = p1.section7([r1, r2])
    assert _sec(c["bytes"]["beaconed"], 7) == want7 and _sec(c["bytes"]["prepared"], 7) == want7
    assert zk.ptau_contributions(c["paths"]["prepared"]) == (
        2, ["contribution first " + r1.response_hash().hex(), "beacon the beacon " + r2.response_hash().hex()])


def test_streaming_in_small_pieces_gives_the_same_file(ctx, tmp_path_factory, tmp_path):
    """Power 5: pieces of 19 points cut section 2's 63 points into four and start at i0 = 19, 38, 57 -- no multiple of the
    2048 scalars of a power_scalars workgroup, nor of the 64 points of a multiplication workgroup."""
    c = _chain(ctx, tmp_path_factory, 5)
    out = tmp_path / "small.ptau"
    ctx.set_option("ptau_piece_points", 19)
    try:
        with _s_env():
            ctx.ptau_contribute(c["paths"]["new"], str(out), c["x1"], name="first")
        assert out.read_bytes() == c["bytes"]["contributed"]
        ctx.ptau_beacon(c["paths"]["contributed"], str(out), BEACON, BEACON_EXP, name="the beacon")
        assert out.read_bytes() == c["bytes"]["beaconed"]
    finally:
        ctx.set_option("ptau_piece_points", 0)
    assert ctx.ptau_verify(str(out), 19) == (0, (5, 5, 0, 2))


# ---- tampering ---------------------------------------------------------------------------------------------------------
def _records_at(buf):
    """(offset in the file, length) of each record of section 7"""
    off, ln = _offsets(buf)[7]
    out, at = [], off + 4
    for _ in range(struct.unpack_from("<I", buf, off)[0]):
        _, used = p1.parse_record(buf, at)
        out.append((at, used))
        at += used
    assert at == off + ln
    return out


def test_tampered_trails_are_reported(ctx, zk, tmp_path_factory, tmp_path):
    """Power 3, two records (a contribution, then a beacon). Offsets inside a record: the five points at 0, the key at
    448 (tau.g2_spx at 832), partialHash at 1216, nextChallenge at 1432, type at 1496, the params from 1504."""
    c = _chain(ctx, tmp_path_factory, 3)
    good = c["bytes"]["beaconed"]
    (a0, l0), (a1, l1) = _records_at(good)
    path = tmp_path / "t.ptau"

    def verify(buf):
        path.write_bytes(buf)
        return ctx.ptau_verify(str(path))[0]

    flip = lambda buf, at: _patch(buf, at, bytes([buf[at] ^ 1]))
    assert verify(good) == 0
    # the name is not hashed and not part of any check: a changed name passes (documented in DESIGN.md section 10)
    name_at = a0 + p1.RECORD_FIXED + 2
    assert good[name_at:name_at + 5] == b"first"
    assert verify(flip(good, name_at)) == 0
    swapped = good[:a0] + good[a1:a1 + l1] + good[a0:a0 + l0] + good[a1 + l1:]
    assert verify(swapped) == CONTRIBUTIONS
    assert verify(_patch(good, a0 + 832, _g2_double(good, a0 + 832))) == CONTRIBUTIONS      # g2_spx of record 0
    assert verify(_patch(good, a1, _g1_double(good, a1))) == CONTRIBUTIONS                  # tauG1 of record 1
    assert verify(flip(good, a1 + 1216 + 70)) == CONTRIBUTIONS                              # partialHash (its counter)
    assert verify(flip(good, a1 + 1216 + 3)) == CONTRIBUTIONS                               # partialHash (its h)
    assert verify(flip(good, a1 + 1432 + 9)) == CONTRIBUTIONS                               # nextChallenge of the last
    assert verify(flip(good, a0 + 1432 + 9)) == CONTRIBUTIONS                               # ... of the first: g2_sp of the next
    t5 = _offsets(good)[2][0] + 64 * 5
    assert verify(_patch(good, t5, _g1_double(good, t5))) & CONTRIBUTIONS                   # the powers checks fire too
    exp_at = a1 + p1.RECORD_FIXED + 2 + len(b"the beacon") + 1
    assert good[exp_at - 1] == 2 and good[exp_at] == BEACON_EXP
    assert verify(_patch(good, exp_at, bytes([BEACON_EXP + 1]))) == CONTRIBUTIONS
    # truncation inside a record, left-over bytes, an unknown tag, a type above 1: malformed files
    s7 = _sec(good, 7)
    for bad7 in (s7[:-3], s7[:4 + 800], s7 + b"\0", _patch(s7, a0 - _offsets(good)[7][0] + p1.RECORD_FIXED, b"\x09"),
                 _patch(s7, a1 - _offsets(good)[7][0] + 1496, struct.pack("<I", 2))):
        path.write_bytes(_rebuild(good, {7: bad7}))
        with pytest.raises(zk.ZkpoaError, match="section 7"):
            ctx.ptau_verify(str(path))


# ---- the command line --------------------------------------------------------------------------------------------------
def _cli(zk, *args, env=None):
    return subprocess.run([zk.SETUP_BIN, "powersoftau"] + [str(a) for a in args], capture_output=True, text=True,
                          timeout=600, env=dict(os.environ, **(env or {})))


def test_cli_new_contribute_beacon_verify(zk, tmp_path):
    new, one, two = tmp_path / "0.ptau", tmp_path / "1.ptau", tmp_path / "2.ptau"
    rc = _cli(zk, "new", "bn128", 2, new)
    assert rc.returncode == 0 and "power 2" in rc.stdout, rc.stderr
    rc = _cli(zk, "contribute", new, one, "--name=alice", "-e=some entropy")
    assert rc.returncode == 0 and "contribution #1: contribution alice " in rc.stdout, rc.stderr
    rc = _cli(zk, "beacon", one, two, BEACON.hex(), 3, "--name=final")
    assert rc.returncode == 0 and "contribution #2: beacon final " in rc.stdout, rc.stderr
    rc = _cli(zk, "verify", two)
    assert rc.returncode == 0 and "Powers of Tau Ok!" in rc.stdout, rc.stderr
    assert "contribution #1: contribution alice " in rc.stdout and "contribution #2: beacon final " in rc.stdout
    assert "section 7" not in rc.stderr and "not prepared" in rc.stderr
    rc = _cli(zk, "verify", new)
    assert rc.returncode == 0 and "section 7" in rc.stderr and "no trail" in rc.stderr
    # two runs with secrets from /dev/urandom differ
    again = tmp_path / "1b.ptau"
    assert _cli(zk, "contribute", new, again).returncode == 0
    assert again.read_bytes() != one.read_bytes()
    # a damaged trail: exit 1 and the check's name
    buf = two.read_bytes()
    (a0, _), _ = _records_at(buf)
    (tmp_path / "bad.ptau").write_bytes(_patch(buf, a0 + 832, _g2_double(buf, a0 + 832)))
    rc = _cli(zk, "verify", tmp_path / "bad.ptau")
    assert rc.returncode == 1 and "[ERROR] zkpoa: CONTRIBUTIONS" in rc.stderr and "Ok!" not in rc.stdout


def test_cli_refusals_leave_nothing_behind(zk, tmp_path):
    new = tmp_path / "0.ptau"
    assert _cli(zk, "new", "bn128", 1, new).returncode == 0
    before = new.read_bytes()
    rc = _cli(zk, "contribute", new, new)
    assert rc.returncode == 1 and "names the input" in rc.stderr and new.read_bytes() == before
    for args in (("new", "bn128", 0, tmp_path / "x"), ("new", "bn128", 29, tmp_path / "x"), ("new", "bls12381", 4, tmp_path / "x"),
                 ("beacon", new, tmp_path / "x", "zz", 3), ("beacon", new, tmp_path / "x", "0102", 31),
                 ("beacon", new, tmp_path / "x", "01" * 256, 3), ("contribute", new)):
        rc = _cli(zk, *args)
        assert rc.returncode == 2, args
        assert not (tmp_path / "x").exists()
    # a failing input: nothing appears at the output, and a file already there is untouched
    bad = tmp_path / "bad.ptau"
    off = _offsets(before)[4][0]
    bad.write_bytes(_patch(before, off, g16.g1_to_bytes((1, 3))))               # A_0 off the curve
    out = tmp_path / "out.ptau"
    rc = _cli(zk, "contribute", bad, out)
    assert rc.returncode == 1 and "not on the curve" in rc.stderr and not out.exists()
    out.write_bytes(b"keep me")
    rc = _cli(zk, "beacon", bad, out, "0102", 2)
    assert rc.returncode == 1 and out.read_bytes() == b"keep me"
    assert [p.name for p in tmp_path.iterdir() if ".tmp." in p.name] == []
    rc = _cli(zk, "contribute", new, tmp_path / "s.ptau", env={"ZKPOA_PHASE1_S": "1,2"})
    assert rc.returncode == 1 and "ZKPOA_PHASE1_S" in rc.stderr and not (tmp_path / "s.ptau").exists()
    rc = _cli(zk, "contribute", new, tmp_path / "s.ptau", env={"ZKPOA_PHASE1_S": "1,2,3"})
    assert rc.returncode == 0 and "WARNING" in rc.stderr and "ZKPOA_PHASE1_S" in rc.stderr


# ---- numbers from the environment: one parser behind ZKPOA_PHASE1_S, ZKPOA_PHASE2_S and ZKPOA_DELTA -------------------
ENV_K = (0xabcdef0123456789abcdef, 0x1f2e3d4c5b6a, R - 0xbeef)   # every hex letter occurs
ENV_FORMS = (str, hex, lambda k: "0X%X" % k)                   # decimal, 0x lower case, 0X upper case
ENV_BAD = ("", "0x", "12,", "12a", "0x12g", "0", str(R), str(1 << 256), "0x1" + "0" * 64)


def _zkey_contribute_cli(zk, key, out, delta):
    return subprocess.run([zk.SETUP_BIN, "zkey", "contribute", str(key), str(out)], capture_output=True, text=True,
                          timeout=300, env=dict(os.environ, ZKPOA_DELTA=delta))


def test_env_numbers_parse_alike_for_all_three_variables(ctx, zk, tmp_path, monkeypatch):
    """Power 1 and the committed n8 key (with a non-zero circuit hash patched into section 10 where a record is to be
    appended: `zkey contribute` does not check the hash, `zkey verify` does). The same texts -- decimal, 0x lower case, 0X
    upper case -- are taken by all three variables and give the same bytes, the ones the number itself gives; the same
    refusals apply to all three and leave nothing behind. ZKPOA_DELTA is the command line's (a text that is no number
    below 2^256 ends it with status 2, the library's range check with status 1), the other two are the library's."""
    from conftest import GOLDEN
    for name in ("ZKPOA_PHASE1_S", "ZKPOA_PHASE2_S", "ZKPOA_DELTA"):
        monkeypatch.delenv(name, raising=False)
    new, out = tmp_path / "new.ptau", tmp_path / "out"
    ctx.ptau_new(1, new)
    key = os.path.join(GOLDEN, "gen", "n8", "circuit.zkey")
    kb = open(key, "rb").read()
    off10 = {t: lst[0] for t, lst in g16.read_binfile(kb, "zkey", 1).items()}[10][0]
    tkey = tmp_path / "t.zkey"
    tkey.write_bytes(_patch(kb, off10, bytes(range(1, 65))))
    k_g1 = [g16.g1_to_bytes(bn.g1_mul(bn.G1_GEN, k)) for k in ENV_K]

    def made():
        b = out.read_bytes()
        out.unlink()
        return b

    # ---- accepted: three fixed secrets (PHASE1_S), the first of them (PHASE2_S, DELTA), in each form
    ptaus, zkeys, deltas = [], [], []
    for form in ENV_FORMS:
        monkeypatch.setenv("ZKPOA_PHASE1_S", ",".join(form(k) for k in ENV_K))
        ctx.ptau_contribute(new, out, (3, 5, 7), name="x")
        monkeypatch.delenv("ZKPOA_PHASE1_S")
        ptaus.append(made())
        monkeypatch.setenv("ZKPOA_PHASE2_S", form(ENV_K[0]))
        ctx.zkey_contribute_ex(tkey, out, 11, "x")
        monkeypatch.delenv("ZKPOA_PHASE2_S")
        zkeys.append(made())
        rc = _zkey_contribute_cli(zk, key, out, form(ENV_K[0]))
        assert rc.returncode == 0 and "WARNING" in rc.stderr and "delta" in rc.stderr, rc.stderr
        deltas.append(made())
    assert ptaus[0] == ptaus[1] == ptaus[2] and zkeys[0] == zkeys[1] == zkeys[2] and deltas[0] == deltas[1] == deltas[2]
    (a0, _), = _records_at(ptaus[0])
    assert [ptaus[0][a0 + 448 + 128 * i:a0 + 448 + 128 * i + 64] for i in range(3)] == k_g1      # the key's three g1_s
    s10 = zkeys[0][{t: lst[0] for t, lst in g16.read_binfile(zkeys[0], "zkey", 1).items()}[10][0]:]
    assert s10[64:68] == struct.pack("<I", 1) and s10[68 + 64:68 + 128] == k_g1[0]              # the record's g1_s
    ctx.zkey_contribute(key, out, ENV_K[0])
    assert made() == deltas[0]

    # ---- refused, nothing written
    def nothing_left():
        return sorted(p.name for p in tmp_path.iterdir()) == ["new.ptau", "t.zkey"]

    one, two = hex(ENV_K[0]), str(ENV_K[1])
    for bad in ENV_BAD:
        for text in (bad, ",".join((one, two, bad)), ",".join((bad, one, two)), ",".join((one, bad, two))):
            monkeypatch.setenv("ZKPOA_PHASE1_S", text)
            with pytest.raises(zk.ZkpoaError, match="ZKPOA_PHASE1_S"):
                ctx.ptau_contribute(new, out, (3, 5, 7), name="x")
        monkeypatch.delenv("ZKPOA_PHASE1_S")
        monkeypatch.setenv("ZKPOA_PHASE2_S", bad)
        with pytest.raises(zk.ZkpoaError, match="ZKPOA_PHASE2_S"):
            ctx.zkey_contribute_ex(tkey, out, 11, "x")
        monkeypatch.delenv("ZKPOA_PHASE2_S")
        rc = _zkey_contribute_cli(zk, key, out, bad)
        in_range_text = bad in ("0", str(R))                       # a number below 2^256: the library refuses it
        assert rc.returncode == (1 if in_range_text else 2) and "delta" in rc.stderr.lower(), (bad, rc.stderr)
        assert "ZKPOA_DELTA" in rc.stderr
        assert nothing_left(), bad
    for text in (",".join((one, two)), ",".join((one, two, one, two)), ",".join((one, two, one)) + ","):
        monkeypatch.setenv("ZKPOA_PHASE1_S", text)
        with pytest.raises(zk.ZkpoaError, match="ZKPOA_PHASE1_S"):
            ctx.ptau_contribute(new, out, (3, 5, 7), name="x")
    assert nothing_left()


def test_cli_a_prepared_input_loses_its_lagrange_sections(ctx, zk, tmp_path_factory, tmp_path):
    c = _chain(ctx, tmp_path_factory, 3)
    out = tmp_path / "next.ptau"
    rc = _cli(zk, "contribute", c["paths"]["prepared"], out, "--name=third")
    assert rc.returncode == 0 and "sections 12-15" in rc.stderr and "dropped" in rc.stderr
    assert sorted(_offsets(out.read_bytes())) == [1, 2, 3, 4, 5, 6, 7]
    assert ctx.ptau_verify(str(out)) == (0, (3, 3, 0, 3))


def test_a_ceremony_made_here_feeds_the_workflow(ctx, zk, tmp_path_factory, tmp_path):
    """new + contribute + beacon + prepare phase2 at power 5, then `zkey new` on a small circuit (12 wires, 5 constraints:
    a domain of 2^3), `zkey verify` against the ceremony, a proof and its verification with the existing entry points."""
    c = _chain(ctx, tmp_path_factory, 5)
    cons, w = g16.random_circuit(random.Random(5), 12, 1, 5)
    (tmp_path / "c.r1cs").write_bytes(sf.write_r1cs(12, 1, cons))
    ctx.zkey_new(tmp_path / "c.r1cs", c["paths"]["prepared"], tmp_path / "c.zkey")
    assert ctx.zkey_verify(tmp_path / "c.r1cs", c["paths"]["prepared"], tmp_path / "c.zkey") == 0
    (tmp_path / "w.wtns").write_bytes(g16.write_wtns(w))
    assert ctx.wtns_check(tmp_path / "c.r1cs", tmp_path / "w.wtns") == (0, None)
    key = ctx.load_zkey((tmp_path / "c.zkey").read_bytes())
    try:
        pts, pub = ctx.prove(key, g16.write_wtns(w), 11, 13)
        assert zk.groth16_verify_points(key.vkey_points(), pts, pub)
    finally:
        key.close()
