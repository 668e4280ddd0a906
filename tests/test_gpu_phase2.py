"""The phase-2 transcript on the device and through the commands (DESIGN.md "Phase-2 transcript"): the hash-form and
H-difference kernels against Python; `zkey new --transcript`, `zkey contribute`, `zkey beacon` against tests/phase2_ref.py
byte for byte; `zkey verify` on good and tampered trails; keys without a transcript behave as before."""
import hashlib
import os
import random
import struct
import subprocess

import pytest

import phase2_ref as ref
from conftest import le
from oracle import c_oracle as co
from oracle.py import bn254 as bn
from oracle.py import groth16 as g16
from test_gpu_zkey_verify import _circuit, _fb1, _fb2, _files, _g1_double, _g2_double, _secs

pytestmark = pytest.mark.gpu
R, Q = bn.R, bn.Q


def _run(zk, tmp_path, *args, env=None, timeout=300):
    return subprocess.run([zk.SETUP_BIN] + list(args), cwd=tmp_path, capture_output=True, text=True, timeout=timeout,
                          env=dict(os.environ, **(env or {})))


def _record_spans(s10):
    """[(offset, length)] of the records inside a section 10 payload."""
    count = struct.unpack_from("<I", s10, 64)[0]
    at, out = 68, []
    for _ in range(count):
        plen = struct.unpack_from("<I", s10, at + 388)[0]
        out.append((at, 392 + plen))
        at += 392 + plen
    assert at == len(s10)
    return out


def test_hash_form_kernel(ctx):
    rng = random.Random(41)
    ks = [rng.randrange(R) for _ in range(1000)]
    for i in (0, 5, 191, 192, 999):
        ks[i] = 0                                                   # infinity, also first and last of a piece
    g1 = _fb1(ks)
    want = b"".join(ref.hash_g1(g16.g1_from_bytes(g1, 64 * i)) for i in range(len(ks)))
    assert want[:64] == b"\x40" + bytes(63)
    for piece in (96, 7, 1 << 12):                                  # 192 / 14 G1 points per piece: neither divides 1000
        got, dg = ctx.hash_form(1, g1, piece)
        assert got == want
        assert dg == hashlib.blake2b(want, digest_size=64).digest()
    ks2 = [rng.randrange(R) for _ in range(333)]
    ks2[0] = ks2[100] = ks2[332] = 0
    g2 = _fb2(ks2)
    want = b"".join(ref.hash_g2(g16.g2_from_bytes(g2, 128 * i)) for i in range(len(ks2)))
    for piece in (100, 1, 0):
        got, dg = ctx.hash_form(2, g2, piece)
        assert got == want
        assert dg == hashlib.blake2b(want, digest_size=64).digest()
    assert ctx.hash_form(1, b"", 0) == (b"", hashlib.blake2b(b"", digest_size=64).digest())


def test_h_diff_kernel(ctx):
    rng = random.Random(43)
    for n in (2, 9, 64, 3001):
        ks = [rng.randrange(R) for _ in range(2 * n - 1)]
        if n >= 9:
            ks[n + 1] = ks[1]                   # T[i+n] = T[i]: the difference is infinity
            ks[n + 2] = R - ks[2]               # T[i+n] = -T[i]: a doubling
            ks[3] = 0                           # T[i] at infinity
            ks[n + 4] = 0                       # T[i+n] at infinity
            ks[5] = ks[n + 5] = 0               # both
        pts = _fb1(ks)
        got = ctx.h_diff(pts, n)
        want = _fb1([ks[i + n] - ks[i] for i in range(n - 1)])
        assert got == want, n
        if n == 9:                              # and point by point with the oracle's own addition
            T = [g16.g1_from_bytes(pts, 64 * i) for i in range(2 * n - 1)]
            for i in range(n - 1):
                assert g16.g1_from_bytes(got, 64 * i) == bn.g1_add(T[i + n], bn.ec_neg(T[i], bn.FQ))


@pytest.mark.parametrize("n_vars,n_public,n_cons,long_row,extra_power", [
    (20, 0, 9, False, 0),          # no public signal
    (400, 1, 40, True, 1),         # a long row; a ceremony larger than needed
    (30, 3, 60, False, 0),         # the domain filled exactly
])
def test_new_with_transcript(ctx, zk, tmp_path, n_vars, n_public, n_cons, long_row, extra_power):
    rng = random.Random(n_vars * 7 + n_cons)
    cons = _circuit(rng, n_vars, n_public, n_cons, long_row)
    tox, n = _files(tmp_path, rng, n_vars, n_public, cons, extra_power)
    ptau = (tmp_path / "pot.ptau").read_bytes()
    ctx.zkey_new_ex(tmp_path / "c.r1cs", tmp_path / "pot.ptau", tmp_path / "c_0.zkey")
    got = (tmp_path / "c_0.zkey").read_bytes()
    want0, _ = g16.synthetic_setup(n_vars, n_public, cons, tox, g1_batch=_fb1, g2_batch=_fb2)
    s = _secs(got)
    assert s == _secs(want0) and s[10][1] == 68
    assert got[:s[10][0]] == want0[:s[10][0]] and got[s[10][0] + 68:] == want0[s[10][0] + 68:]
    cs = ref.circuit_hash(want0, ptau)
    assert got[s[10][0]:s[10][0] + 68] == ref.section10(cs, [])
    # the executable writes the same file; without the option it writes the oracle's (zero hash)
    rc = _run(zk, tmp_path, "zkey", "new", "c.r1cs", "pot.ptau", "cli.zkey", "--transcript")
    assert rc.returncode == 0, rc.stderr
    assert (tmp_path / "cli.zkey").read_bytes() == got
    rc = _run(zk, tmp_path, "zkey", "new", "c.r1cs", "pot.ptau", "plain.zkey")
    assert rc.returncode == 0 and (tmp_path / "plain.zkey").read_bytes() == want0
    assert ctx.zkey_verify(tmp_path / "c.r1cs", tmp_path / "pot.ptau", tmp_path / "c_0.zkey") == 0
    rc = _run(zk, tmp_path, "zkey", "verify", "c.r1cs", "pot.ptau", "c_0.zkey")
    assert rc.returncode == 0 and "ZKey Ok!" in rc.stdout and "0 contribution(s)" in rc.stdout, rc.stderr
    assert "section 10" not in rc.stderr and "no contribution" in rc.stderr
    assert zk.zkey_contributions(tmp_path / "c_0.zkey") == (True, [])
    assert zk.zkey_contributions(tmp_path / "plain.zkey") == (False, [])


def _trail(ctx, zk, tmp_path, monkeypatch, rng, n_vars=40, n_public=2, n_cons=50):
    """new --transcript, contribute (C ABI), contribute (CLI), beacon (CLI) with known secrets."""
    cons = _circuit(rng, n_vars, n_public, n_cons)
    tox, n = _files(tmp_path, rng, n_vars, n_public, cons)
    ctx.zkey_new_ex(tmp_path / "c.r1cs", tmp_path / "pot.ptau", tmp_path / "c_0.zkey")
    d1, d2, s1, s2 = (rng.randrange(1, R) for _ in range(4))
    monkeypatch.setenv("ZKPOA_PHASE2_S", str(s1))
    ctx.zkey_contribute_ex(tmp_path / "c_0.zkey", tmp_path / "c_1.zkey", d1, "first")
    monkeypatch.delenv("ZKPOA_PHASE2_S")
    rc = _run(zk, tmp_path, "zkey", "contribute", "c_1.zkey", "c_2.zkey", "--name=second one", "-e=ignored",
              env={"ZKPOA_DELTA": str(d2), "ZKPOA_PHASE2_S": hex(s2)})
    assert rc.returncode == 0 and "ZKPOA_PHASE2_S" in rc.stderr, rc.stderr
    beacon = bytes.fromhex("0102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f")
    rc = _run(zk, tmp_path, "zkey", "beacon", "c_2.zkey", "c_3.zkey", beacon.hex(), "10", "-n=Final Beacon")
    assert rc.returncode == 0, rc.stderr
    return dict(cons=cons, tox=tox, n=n, n_vars=n_vars, n_public=n_public, d=(d1, d2), s=(s1, s2), beacon=beacon)


def test_contribute_contribute_beacon(ctx, zk, tmp_path, monkeypatch):
    rng = random.Random(2025)
    t = _trail(ctx, zk, tmp_path, monkeypatch, rng)
    (d1, d2), (s1, s2), beacon = t["d"], t["s"], t["beacon"]
    ptau = (tmp_path / "pot.ptau").read_bytes()
    want0, _ = g16.synthetic_setup(t["n_vars"], t["n_public"], t["cons"], t["tox"], g1_batch=_fb1, g2_batch=_fb2)
    cs = ref.circuit_hash(want0, ptau)
    db, sb = ref.beacon_secrets(beacon, 10)
    recs = []
    recs.append(ref.next_record(cs, recs, bn.G1_GEN, d1, bn.g1_mul(bn.G1_GEN, s1), 0, b"first"))
    recs.append(ref.next_record(cs, recs, recs[-1].delta_after, d2, bn.g1_mul(bn.G1_GEN, s2), 0, b"second one"))
    recs.append(ref.next_record(cs, recs, recs[-1].delta_after, db, sb, 1, b"Final Beacon", 10, beacon))
    delta = 1
    for k, d in enumerate((d1, d2, db), 1):
        delta = delta * d % R
        got = (tmp_path / ("c_%d.zkey" % k)).read_bytes()
        want, _ = g16.synthetic_setup(t["n_vars"], t["n_public"], t["cons"], dict(t["tox"], delta=delta), g1_batch=_fb1,
                                      g2_batch=_fb2)
        s = _secs(got)
        assert got[:s[10][0] - 8] == want[:s[10][0] - 8]                       # every section before 10, byte for byte
        assert got[s[10][0]:] == ref.section10(cs, recs[:k]), k                # section 10 is the last one
        assert ctx.zkey_verify(tmp_path / "c.r1cs", tmp_path / "pot.ptau", tmp_path / ("c_%d.zkey" % k)) == 0
    rc = _run(zk, tmp_path, "zkey", "verify", "c.r1cs", "pot.ptau", "c_3.zkey")
    assert rc.returncode == 0 and "ZKey Ok!" in rc.stdout, rc.stderr
    assert "3 contribution(s)" in rc.stdout
    for line in ("#1: contribution first", "#2: contribution second one", "#3: beacon Final Beacon"):
        assert line in rc.stdout
    assert "section 10" not in rc.stderr and "no contribution" not in rc.stderr
    assert zk.zkey_contributions(tmp_path / "c_3.zkey") == (True, [("contribution", "first"), ("contribution", "second one"),
                                                                    ("beacon", "Final Beacon")])


def test_tampered_trails_fail_with_their_bit(ctx, zk, tmp_path, monkeypatch):
    B = zk.ZKEY_CHECKS
    rng = random.Random(77)
    t = _trail(ctx, zk, tmp_path, monkeypatch, rng)
    good = (tmp_path / "c_3.zkey").read_bytes()
    s = _secs(good)
    s10 = s[10][0]
    spans = _record_spans(good[s10:s10 + s[10][1]])
    verify = lambda name="t.zkey": ctx.zkey_verify(tmp_path / "c.r1cs", tmp_path / "pot.ptau", tmp_path / name)
    assert verify("c_3.zkey") == 0

    def tampered(at, data):
        b = bytearray(good)
        b[at:at + len(data)] = data
        (tmp_path / "t.zkey").write_bytes(bytes(b))
        return verify()
    # one byte of the circuit hash
    assert tampered(s10 + 17, bytes([good[s10 + 17] ^ 1])) == B["CSHASH"]
    # records 0 and 1 swapped (the section keeps its length)
    (o0, l0), (o1, l1) = spans[0], spans[1]
    swapped = good[s10 + o1:s10 + o1 + l1] + good[s10 + o0:s10 + o0 + l0]
    assert tampered(s10 + o0, swapped) == B["CONTRIBUTIONS"]
    # a wrong g2_spx (a valid G2 point)
    at = s10 + spans[1][0] + 192
    assert tampered(at, _g2_double(good, at)) == B["CONTRIBUTIONS"]
    # the beacon record with other beacon bytes (the last byte of its params)
    at = s10 + spans[2][0] + spans[2][1] - 1
    assert tampered(at, bytes([good[at] ^ 0x80])) == B["CONTRIBUTIONS"]
    # a deltaAfter in the middle of the chain; the last deltaAfter != delta1
    at = s10 + spans[1][0]
    assert tampered(at, _g1_double(good, at)) == B["CONTRIBUTIONS"]
    at = s10 + spans[2][0]
    assert tampered(at, _g1_double(good, at)) == B["CONTRIBUTIONS"]
    # a contribution by the old entry point after a transcript existed: a stale trail
    ctx.zkey_contribute(tmp_path / "c_3.zkey", tmp_path / "stale.zkey", rng.randrange(1, R))
    assert verify("stale.zkey") == B["CONTRIBUTIONS"]
    rc = _run(zk, tmp_path, "zkey", "verify", "c.r1cs", "pot.ptau", "stale.zkey")
    assert rc.returncode == 1 and "CONTRIBUTIONS:" in rc.stderr and "ZKey Ok!" not in rc.stdout
    # a truncated and an over-long section 10 are malformed files
    last = s10 + s[10][1]
    for name, data in (("short.zkey", good[:s10 - 8] + struct.pack("<Q", s[10][1] - 5) + good[s10:last - 5]),
                       ("long.zkey", good[:s10 - 8] + struct.pack("<Q", s[10][1] + 3) + good[s10:last] + bytes(3))):
        (tmp_path / name).write_bytes(data)
        with pytest.raises(zk.ZkpoaError, match="section 10"):
            verify(name)
    assert verify("c_3.zkey") == 0


def test_keys_without_a_transcript_behave_as_before(ctx, zk, tmp_path):
    rng = random.Random(99)
    n_vars, n_public = 24, 1
    cons = _circuit(rng, n_vars, n_public, 20)
    tox, n = _files(tmp_path, rng, n_vars, n_public, cons)
    ctx.zkey_new(tmp_path / "c.r1cs", tmp_path / "pot.ptau", tmp_path / "c_0.zkey")
    want0, _ = g16.synthetic_setup(n_vars, n_public, cons, tox, g1_batch=_fb1, g2_batch=_fb2)
    assert (tmp_path / "c_0.zkey").read_bytes() == want0
    d = rng.randrange(1, R)
    rc = _run(zk, tmp_path, "zkey", "contribute", "c_0.zkey", "c_1.zkey", "--name=x", env={"ZKPOA_DELTA": str(d)})
    assert rc.returncode == 0, rc.stderr
    want1, _ = g16.synthetic_setup(n_vars, n_public, cons, dict(tox, delta=d), g1_batch=_fb1, g2_batch=_fb2)
    assert (tmp_path / "c_1.zkey").read_bytes() == want1
    rc = _run(zk, tmp_path, "zkey", "verify", "c.r1cs", "pot.ptau", "c_1.zkey")
    assert rc.returncode == 0 and "ZKey Ok!" in rc.stdout and "section 10" in rc.stderr and "contribution(s)" not in rc.stdout
    # beacon and contribute_ex need a transcript
    rc = _run(zk, tmp_path, "zkey", "beacon", "c_1.zkey", "b.zkey", "0102", "3")
    assert rc.returncode == 1 and "transcript" in rc.stderr and not (tmp_path / "b.zkey").exists()
    with pytest.raises(zk.ZkpoaError, match="transcript"):
        ctx.zkey_contribute_ex(tmp_path / "c_1.zkey", tmp_path / "b.zkey", d, "x")
    with pytest.raises(zk.ZkpoaError, match="30"):
        ctx.zkey_beacon(tmp_path / "c_1.zkey", tmp_path / "b.zkey", b"\x01", 31)
    rc = _run(zk, tmp_path, "zkey", "beacon", "c_1.zkey", "b.zkey", "0102", "31")
    assert rc.returncode == 2
    # a ptau without the powers of section 2 cannot give a transcript
    ptau = (tmp_path / "pot.ptau").read_bytes()
    secs = g16.read_binfile(ptau, "ptau", 1)
    (tmp_path / "nopow.ptau").write_bytes(g16.write_binfile("ptau", 1, [
        (t, b"" if t == 2 else ptau[secs[t][0][0]:secs[t][0][0] + secs[t][0][1]]) for t in sorted(secs)]))
    with pytest.raises(zk.ZkpoaError, match="section 2"):
        ctx.zkey_new_ex(tmp_path / "c.r1cs", tmp_path / "nopow.ptau", tmp_path / "n.zkey")
    ctx.zkey_new(tmp_path / "c.r1cs", tmp_path / "nopow.ptau", tmp_path / "n.zkey")
    assert (tmp_path / "n.zkey").read_bytes() == want0
