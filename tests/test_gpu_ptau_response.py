"""`snarkjs powersoftau export challenge / challenge contribute / import response` on the device (csrc/ptau_response.hip:
the square root, compressed form -> wire form, hash form -> wire form; csrc/ptau_contribute.hip: the three commands; C ABI
zkpoa_sqrt_device, zkpoa_decompressed_form, zkpoa_from_hash_form, zkpoa_ptau_export_challenge / _challenge_contribute /
_import_response).

Every expected byte comes from the oracle or from tests/response_ref.py, tests/phase1_ref.py and tests/phase2_ref.py
(written from DESIGN.md "Phase-1 transcript"), never from the code under test; the one exception the text of the feature
asks for is the imported file, which is also compared with the file `powersoftau contribute` makes from the same inputs.
Every comparison is exact."""
import os
import random
import subprocess

import pytest

import phase1_ref as p1
import phase2_ref as p2
import response_ref as rr
import setup_files as sf
from conftest import le
from oracle import c_oracle as co
from oracle.py import bn254 as bn
from oracle.py import groth16 as g16
from test_gpu_ptau_contribute import S_ENV, _chain, _s_env, _sec
from test_gpu_ptau_verify import _patch

gpu = pytest.mark.gpu
R, Q = bn.R, bn.Q
F2 = bn.FQ2
W = 256                                                             # kFormThreads: the workgroup of the new kernels
TAU_G1, CONTRIBUTIONS = 0x002, 0x200


def _fb(group, ks):
    data = b"".join(le(k % R) for k in ks)
    return co.fixed_base_g1(data, 8) if group == 1 else co.fixed_base_g2(data, 8)


def _points(group, data):
    unit = 64 * group
    rd = g16.g1_from_bytes if group == 1 else g16.g2_from_bytes
    return [rd(data, unit * i) for i in range(len(data) // unit)]


def _compress(group, data):
    comp = p1.compress_g1 if group == 1 else p1.compress_g2
    return b"".join(comp(P) for P in _points(group, data))


def _hash(group, data):
    return b"".join((p2.hash_g1 if group == 1 else p2.hash_g2)(P) for P in _points(group, data))


def _mont(a):
    return le(bn.to_mont(a % Q, Q))


# ---- without a GPU ---------------------------------------------------------------------------------------------------
def test_reference_roots_agree_with_the_host_hooks(zk):
    rng = random.Random(1)
    for a in [0, 1, Q - 1, 4, 3] + [rng.randrange(Q) for _ in range(40)]:
        want, got = rr.fq_sqrt(a), zk.fq_sqrt(a)
        assert (want is None) == (got is None), a
        if want is not None:
            assert got in (want, Q - want) and not p2.fq_negative(want) and want * want % Q == a
    cases = [(0, 0), (9, 0), (Q - 9, 0), (5, 0), (Q - 5, 0)] + [(rng.randrange(Q), rng.randrange(Q)) for _ in range(40)]
    cases += [F2.sqr((rng.randrange(Q), rng.randrange(Q))) for _ in range(10)]
    for a in cases:
        want, got = rr.fq2_sqrt(a), zk.fq2_sqrt(a)
        assert (want is None) == (got is None), a
        if want is not None:
            assert got in (want, F2.neg(want)) and not p2.fq2_negative(want) and F2.eq(F2.sqr(want), a)
    assert sum(rr.fq2_sqrt(a) is None for a in cases) > 5           # non-squares occur


@pytest.mark.parametrize("group", [1, 2])
def test_reference_decompression_inverts_compression(group):
    rng = random.Random(10 + group)
    points = _points(group, _fb(group, [1, R - 1, 0] + [rng.randrange(1, R) for _ in range(20)]))
    comp, dec = (p1.compress_g1, rr.decompress_g1) if group == 1 else (p1.compress_g2, rr.decompress_g2)
    hsh, unh = (p2.hash_g1, rr.unhash_g1) if group == 1 else (p2.hash_g2, rr.unhash_g2)
    assert [dec(comp(P)) for P in points] == points
    assert [unh(hsh(P)) for P in points] == points
    assert {comp(P)[0] & 0xc0 for P in points} == {0x00, 0x80, 0x40}


def test_reference_file_sizes_give_the_power_back():
    for power in range(1, 29):
        for size_of in (rr.challenge_size, rr.response_size):
            size = size_of(power)
            assert rr.power_of(size, size_of) == power
            assert rr.power_of(size - 1, size_of) is None and rr.power_of(size + 1, size_of) is None
    n = 8
    secs = {2: [bn.G1_GEN] * (2 * n - 1), 3: [bn.G2_GEN] * n, 4: [bn.G1_GEN] * n, 5: [bn.G1_GEN] * n, 6: [bn.G2_GEN]}
    assert len(rr.challenge_file(bytes(64), secs)) == rr.challenge_size(3)
    assert len(rr.response_file(bytes(64), secs, [bn.G1_GEN] * 6, [bn.G2_GEN] * 3)) == rr.response_size(3)


# ---- the kernels -----------------------------------------------------------------------------------------------------
def _fq_values():
    rng = random.Random(2)
    vals = [0, 1, Q - 1]
    while len(vals) < W + 1:
        c = rng.randrange(1, Q)
        vals += [c * c % Q, Q - c * c % Q, rng.randrange(Q)]       # a square, a non-square (-1 is none), either
    return vals[:W + 1]


@gpu
@pytest.mark.parametrize("n", [1, W - 1, W, W + 1])
def test_sqrt_device_fq(ctx, n):
    vals = _fq_values()
    vals = vals[-n:] if n < 4 else vals[:n]                        # n = 1: not the zero
    roots, flags = ctx.sqrt_device(0, b"".join(_mont(a) for a in vals))
    want = [rr.fq_sqrt(a) for a in vals]
    assert list(flags) == [0 if r is None else 1 for r in want]
    assert roots == b"".join(_mont(r or 0) for r in want)
    if n >= W - 1:
        assert 0 in flags and 1 in flags and vals[:3] == [0, 1, Q - 1]


@gpu
def test_sqrt_device_fq2(ctx):
    """a = 0; (c^2, 0), whose root is real: (c, 0) or (-c, 0), the sign rule falls to c0; (-c^2, 0), whose root is purely
    imaginary; squares and non-squares in general; W + 1 elements are two workgroups."""
    rng = random.Random(3)
    vals = [(0, 0), (1, 0), (Q - 1, 0)]
    for _ in range(6):
        c = rng.randrange(1, Q)
        vals += [(c * c % Q, 0), (Q - c * c % Q, 0)]
    while len(vals) < W + 1:
        vals += [F2.sqr((rng.randrange(Q), rng.randrange(Q))), (rng.randrange(Q), rng.randrange(Q))]
    vals = vals[:W + 1]
    roots, flags = ctx.sqrt_device(2, b"".join(_mont(a[0]) + _mont(a[1]) for a in vals))
    want = [rr.fq2_sqrt(a) for a in vals]
    assert list(flags) == [0 if r is None else 1 for r in want]
    assert roots == b"".join(_mont(r[0]) + _mont(r[1]) for r in [w or (0, 0) for w in want])
    assert 0 in flags and all(flags[:15])
    real = [w for w in want[3:15:2]]
    assert all(w[1] == 0 and w[0] <= (Q - 1) // 2 for w in real) and all(w[0] == 0 for w in want[4:15:2])
    with pytest.raises(Exception, match="below q|field element"):
        ctx.sqrt_device(0, le(Q))


def _mixed_logs(n, seed):
    rng = random.Random(seed)
    return ([1, R - 1, 0] + [rng.randrange(1, R) for _ in range(n)])[:n]


@gpu
@pytest.mark.parametrize("group", [1, 2])
def test_decompressed_form_inverts_the_reference_compression(ctx, group):
    points = _fb(group, _mixed_logs(37, group))
    comp = _compress(group, points)
    unit = 32 * group
    assert {comp[unit * i] & 0xc0 for i in range(37)} == {0x00, 0x80, 0x40}          # both signs and infinity occur
    assert ctx.decompressed_form(group, comp) == points
    assert ctx.decompressed_form(group, comp, 13 if group == 2 else 7) == points      # 37 points cross pieces
    assert ctx.decompressed_form(group, b"") == b""


@gpu
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("n", [W - 1, W, W + 1])
def test_decompressed_form_at_the_workgroup_border(ctx, group, n):
    points = _fb(group, _mixed_logs(n, 100 * group + n))
    assert ctx.decompressed_form(group, _compress(group, points)) == points


def _bad_compressed(group):
    """what to put in a point's place -> the words the message must hold"""
    unit = 32 * group
    x1 = rr.g1_x_off_curve(5)
    x2 = rr.g2_x_off_curve(5)
    off_curve = x1.to_bytes(32, "big") if group == 1 else x2[1].to_bytes(32, "big") + x2[0].to_bytes(32, "big")
    with pytest.raises(rr.FormError, match="curve"):
        (rr.decompress_g1 if group == 1 else rr.decompress_g2)(off_curve)
    return [(Q.to_bytes(32, "big") + bytes(unit - 32), "not below q"),
            (bytes(unit - 32) + Q.to_bytes(32, "big") if group == 2 else (Q + 1).to_bytes(32, "big"), "not below q"),
            (b"\xc0" + bytes(unit - 1), "both flag bits"),
            (b"\x40" + bytes(unit - 2) + b"\x01", "0x40"),
            (off_curve, "not on the curve")]


@gpu
@pytest.mark.parametrize("group", [1, 2])
def test_decompressed_form_refusals_name_the_point(ctx, zk, group):
    comp = _compress(group, _fb(group, _mixed_logs(37, 7 + group)))
    unit = 32 * group
    for bad, words in _bad_compressed(group):
        for at in (0, 18, 36):
            data = _patch(comp, unit * at, bad)
            for piece in (0, 7):
                with pytest.raises(zk.ZkpoaError, match=r"point %d: .*%s" % (at, words)):
                    ctx.decompressed_form(group, data, piece)
    # two offenders: the first is named
    data = _patch(_patch(comp, unit * 30, b"\xc0" + bytes(unit - 1)), unit * 4, _bad_compressed(group)[4][0])
    with pytest.raises(zk.ZkpoaError, match="point 4: "):
        ctx.decompressed_form(group, data)
    assert ctx.decompressed_form(group, comp) == _fb(group, _mixed_logs(37, 7 + group))   # the context goes on working


@gpu
@pytest.mark.parametrize("group", [1, 2])
def test_from_hash_form_inverts_hash_form(ctx, zk, group):
    for n, piece in ((37, 7), (W + 1, 0)):
        points = _fb(group, _mixed_logs(n, 50 * group + n))
        hashed = _hash(group, points)
        assert ctx.hash_form(group, points)[0] == hashed
        assert ctx.from_hash_form(group, hashed) == points
        assert ctx.from_hash_form(group, hashed, piece or 100) == points
    unit = 64 * group
    hashed = _hash(group, _fb(group, _mixed_logs(37, 9)))
    assert hashed[2 * unit] == 0x40                                  # point 2 is infinity
    for at in (0, 18, 36):
        for coord in range(2 * group):
            with pytest.raises(zk.ZkpoaError, match="point %d: .*not below q" % at):
                ctx.from_hash_form(group, _patch(hashed, unit * at + 32 * coord, Q.to_bytes(32, "big")), 7)
        with pytest.raises(zk.ZkpoaError, match="point %d: .*bit 7" % at):
            ctx.from_hash_form(group, _patch(hashed, unit * at, bytes([hashed[unit * at] | 0x80])))
        with pytest.raises(zk.ZkpoaError, match="point %d: .*0x40" % at):
            ctx.from_hash_form(group, _patch(hashed, unit * at, b"\x40" + bytes(unit - 2) + b"\x02"))


# ---- the commands ------------------------------------------------------------------------------------------------------
def _gen_secs(power):
    n = 1 << power
    return {2: [bn.G1_GEN] * (2 * n - 1), 3: [bn.G2_GEN] * n, 4: [bn.G1_GEN] * n, 5: [bn.G1_GEN] * n, 6: [bn.G2_GEN]}


def _key_points():
    return [bn.g1_mul(bn.G1_GEN, s) for s in S_ENV]


def _no_leftovers(d):
    return [p.name for p in d.iterdir() if ".tmp." in p.name] == []


_trips = {}


def _trip(ctx, tmp_path_factory, power):
    """export -> challenge contribute -> import on the fresh file of the chain, once per power"""
    if power in _trips:
        return _trips[power]
    c = _chain(ctx, tmp_path_factory, power)
    d = tmp_path_factory.mktemp("trip%d" % power)
    t = {"dir": d, "challenge": str(d / "challenge"), "response": str(d / "response"), "new": str(d / "imported.ptau")}
    t["challenge_hash"] = ctx.ptau_export_challenge(c["paths"]["new"], t["challenge"])
    with _s_env():
        t["response_hash"] = ctx.ptau_challenge_contribute(t["challenge"], t["response"], c["x1"])
    ctx.ptau_import_response(c["paths"]["new"], t["response"], t["new"], name="first")
    t["bytes"] = {k: open(t[k], "rb").read() for k in ("challenge", "response", "new")}
    _trips[power] = t
    return t


@gpu
@pytest.mark.parametrize("power", [1, 3, 5])
def test_export_challenge(ctx, tmp_path_factory, tmp_path, power):
    c = _chain(ctx, tmp_path_factory, power)
    t = _trip(ctx, tmp_path_factory, power)
    fresh = t["bytes"]["challenge"]
    assert fresh == rr.challenge_file(p1.blake2b(b""), _gen_secs(power)) and len(fresh) == rr.challenge_size(power)
    assert t["challenge_hash"] == p1.blake2b(fresh) == p1.fresh_challenge(power)
    # a file with a record: its response hash, then the sections it made
    secs1, _ = p1.read_sections(c["want1"])
    r1 = p1.next_record(p1.fresh_challenge(power), secs1, c["x1"], _key_points(), 0, b"first")
    out = tmp_path / "challenge"
    h = ctx.ptau_export_challenge(c["paths"]["contributed"], out)
    data = out.read_bytes()
    assert data[:64] == r1.response_hash() and data == rr.challenge_file(r1.response_hash(), secs1)
    assert h == p1.blake2b(data) == r1.next_challenge
    # a prepared file exports what the file before it exports: sections 12-15 play no part
    h2 = ctx.ptau_export_challenge(c["paths"]["prepared"], tmp_path / "c2")
    assert h2 == p1.blake2b((tmp_path / "c2").read_bytes()) == p1.parse_record(_sec(c["bytes"]["beaconed"], 7), 4 + len(r1.to_bytes()))[0].next_challenge


@gpu
def test_export_refuses_sections_that_are_not_the_records(ctx, zk, tmp_path_factory, tmp_path):
    c = _chain(ctx, tmp_path_factory, 3)
    buf = c["bytes"]["contributed"]
    off = g16.read_binfile(buf, "ptau", 1)[4][0][0]
    bad = tmp_path / "bad.ptau"
    bad.write_bytes(_patch(buf, off + 64 * 3, g16.g1_to_bytes(bn.g1_mul(bn.G1_GEN, 77))))
    with pytest.raises(zk.ZkpoaError, match="not the file's challenge"):
        ctx.ptau_export_challenge(bad, tmp_path / "challenge")
    with pytest.raises(zk.ZkpoaError, match="names the input"):
        ctx.ptau_export_challenge(bad, bad)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["bad.ptau"]


@gpu
@pytest.mark.parametrize("power", [1, 3, 5])
def test_challenge_contribute_and_import_on_a_fresh_file(ctx, zk, tmp_path_factory, power):
    c = _chain(ctx, tmp_path_factory, power)
    t = _trip(ctx, tmp_path_factory, power)
    challenge = p1.fresh_challenge(power)
    secs1, _ = p1.read_sections(c["want1"])
    k1, k2 = p1.make_key(c["x1"], _key_points(), challenge)
    response = t["bytes"]["response"]
    assert response == rr.response_file(challenge, secs1, k1, k2) and len(response) == rr.response_size(power)
    assert t["response_hash"] == p1.blake2b(response)
    assert t["bytes"]["new"] == c["bytes"]["contributed"]            # what `powersoftau contribute` makes of the same
    r1 = p1.next_record(challenge, secs1, c["x1"], _key_points(), 0, b"first")
    assert _sec(t["bytes"]["new"], 7) == p1.section7([r1]) and r1.response_hash() == t["response_hash"]
    for s in range(2, 7):
        assert _sec(t["bytes"]["new"], s) == _sec(c["want1"], s), s
    assert ctx.ptau_verify(t["new"]) == (0, (power, power, 0, 1))
    assert _no_leftovers(t["dir"])


@gpu
@pytest.mark.parametrize("power,piece", [(1, 0), (3, 0), (5, 0), (5, 5)])
def test_round_trip_on_a_file_that_holds_a_record(ctx, zk, tmp_path_factory, tmp_path, power, piece):
    """The challenge is a nextChallenge and the sections carry a product of secrets; the old file is the prepared one, so
    its sections 12-15 are dropped. piece = 5 cuts section 2's 63 points into thirteen pieces."""
    c = _chain(ctx, tmp_path_factory, power)
    rng = random.Random(400 + power)
    x3 = tuple(rng.randrange(1, R) for _ in range(3))
    old = c["paths"]["prepared"]
    want = tmp_path / "want.ptau"
    with _s_env():
        ctx.ptau_contribute(old, want, x3, name="third")
    ctx.set_option("ptau_piece_points", piece)
    try:
        ch = ctx.ptau_export_challenge(old, tmp_path / "challenge")
        with _s_env():
            rh = ctx.ptau_challenge_contribute(tmp_path / "challenge", tmp_path / "response", x3)
        ctx.ptau_import_response(old, tmp_path / "response", tmp_path / "new.ptau", name="third")
    finally:
        ctx.set_option("ptau_piece_points", 0)
    records, at, s7 = [], 4, _sec(c["bytes"]["beaconed"], 7)
    for _ in range(2):
        r, used = p1.parse_record(s7, at)
        records.append(r)
        at += used
    assert ch == records[1].next_challenge
    secs3, _ = p1.read_sections(sf.write_ptau(power, *[a * b * k % R for a, b, k in zip(c["x1"], c["x2"], x3)]))
    k1, k2 = p1.make_key(x3, _key_points(), ch)
    response = (tmp_path / "response").read_bytes()
    assert response == rr.response_file(ch, secs3, k1, k2) and rh == p1.blake2b(response)
    new = (tmp_path / "new.ptau").read_bytes()
    assert new == want.read_bytes()
    r3 = p1.next_record(ch, secs3, x3, _key_points(), 0, b"third")
    assert _sec(new, 7) == p1.section7(records + [r3])
    assert ctx.ptau_verify(tmp_path / "new.ptau", piece) == (0, (power, power, 0, 3))


@gpu
def test_import_refusals_leave_nothing_behind(ctx, zk, tmp_path_factory, tmp_path):
    power = 3
    c = _chain(ctx, tmp_path_factory, power)
    t = _trip(ctx, tmp_path_factory, power)
    good, old, out = t["bytes"]["response"], c["paths"]["new"], tmp_path / "out.ptau"
    bad = tmp_path / "response"

    def refused(old_path, data, words):
        bad.write_bytes(data)
        with pytest.raises(zk.ZkpoaError, match=words):
            ctx.ptau_import_response(old_path, bad, out, name="first")
        assert not out.exists() and _no_leftovers(tmp_path)

    refused(c["paths"]["contributed"], good, "another challenge")
    refused(old, good[:-32], "bytes")
    refused(old, good + bytes(32), "bytes")
    at4 = rr.response_offset(power, 4, 6)
    refused(old, _patch(good, at4, rr.g1_x_off_curve(1000).to_bytes(32, "big")), "section 4: point 6: .*not on the curve")
    P = rr.twist_point_outside_g2(3)
    assert bn.g2_is_on_curve(P) and bn.ec_mul(P, R, F2, order=1 << 300) is not None
    refused(old, _patch(good, rr.response_offset(power, 3, 2), p1.compress_g2(P)), "section 3: .*outside G2")
    at2 = rr.response_offset(power, 2, 1)
    refused(old, _patch(good, at2, bytes([good[at2] ^ 0x80])), "does not verify")      # -tau G1: the record's ratio check
    refused(old, _patch(good, len(good) - 1, bytes([good[-1] ^ 1])), "the record does not verify")   # a key byte: beta.g2_spx leaves its curve
    refused(old, _patch(good, len(good) - rr.KEY_BYTES, b"\x80"), "point 0 of the key is not in hash form")
    with pytest.raises(zk.ZkpoaError, match="names an input"):
        bad.write_bytes(good)
        ctx.ptau_import_response(old, bad, bad)
    assert bad.read_bytes() == good
    # the powers are `powersoftau verify`'s business: -tau^5 G1 imports, and verify names the section
    at5 = rr.response_offset(power, 2, 5)
    bad.write_bytes(_patch(good, at5, bytes([good[at5] ^ 0x80])))
    ctx.ptau_import_response(old, bad, out, name="first")
    failed, info = ctx.ptau_verify(out)
    assert failed & TAU_G1 and not failed & CONTRIBUTIONS and info == (power, power, 0, 1)


@gpu
def test_challenge_contribute_refusals(ctx, zk, tmp_path_factory, tmp_path):
    t = _trip(ctx, tmp_path_factory, 3)
    good, out = t["bytes"]["challenge"], tmp_path / "response"
    bad = tmp_path / "challenge"
    for data, words in ((good[:-64], "no challenge of a power"), (good + bytes(64), "no challenge of a power"),
                        (_patch(good, 64 + 64 * 4, Q.to_bytes(32, "big")), "section 2: point 4: .*not below q"),
                        (_patch(good, 64 + 64 * 15 + 128 * 3, b"\x80"), "section 3: point 3: .*bit 7"),
                        (_patch(good, 64 + 64 * 2 + 32, (3).to_bytes(32, "big")), "section 2: .*not on the curve")):
        bad.write_bytes(data)
        with pytest.raises(zk.ZkpoaError, match=words):
            ctx.ptau_challenge_contribute(bad, out, (3, 5, 7))
        assert not out.exists() and _no_leftovers(tmp_path)
    bad.write_bytes(good)
    with pytest.raises(zk.ZkpoaError, match="names the input"):
        ctx.ptau_challenge_contribute(bad, bad, (3, 5, 7))
    with pytest.raises(zk.ZkpoaError, match=r"\[1, r\)"):
        ctx.ptau_challenge_contribute(bad, out, (3, 0, 7))
    assert bad.read_bytes() == good and not out.exists()


# ---- the command line --------------------------------------------------------------------------------------------------
def _cli(zk, cwd, *args):
    return subprocess.run([zk.SETUP_BIN, "powersoftau"] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True,
                          timeout=600, env=dict(os.environ))


@gpu
def test_cli_export_contribute_import_verify(zk, tmp_path):
    new, out = tmp_path / "0.ptau", tmp_path / "1.ptau"
    assert _cli(zk, tmp_path, "new", "bn128", 2, new).returncode == 0
    rc = _cli(zk, tmp_path, "export", "challenge", new)             # the default name, in the working directory
    assert rc.returncode == 0, rc.stderr
    challenge = (tmp_path / "challenge").read_bytes()
    assert "challenge hash: " + p1.blake2b(challenge).hex() in rc.stdout and p1.blake2b(challenge) == p1.fresh_challenge(2)
    rc = _cli(zk, tmp_path, "challenge", "contribute", "bn128", "challenge", "--name=bob", "-e=some entropy")
    assert rc.returncode == 0, rc.stderr
    response = (tmp_path / "response").read_bytes()
    assert "response hash: " + p1.blake2b(response).hex() in rc.stdout and response[:64] == p1.blake2b(challenge)
    rc = _cli(zk, tmp_path, "import", "response", new, "response", out, "--name=bob")
    assert rc.returncode == 0 and "contribution #1: contribution bob " + p1.blake2b(response).hex() in rc.stdout, rc.stderr
    rc = _cli(zk, tmp_path, "verify", out)
    assert rc.returncode == 0 and "Powers of Tau Ok!" in rc.stdout, rc.stderr
    assert "contribution #1: contribution bob " + p1.blake2b(response).hex() in rc.stdout
    # named outputs; an output that is the input; a wrong curve; too few arguments
    rc = _cli(zk, tmp_path, "export", "challenge", out, tmp_path / "c2")
    assert rc.returncode == 0 and (tmp_path / "c2").read_bytes()[:64] == p1.blake2b(response)
    before = new.read_bytes()
    rc = _cli(zk, tmp_path, "export", "challenge", new, new)
    assert rc.returncode == 1 and "names the input" in rc.stderr and new.read_bytes() == before
    assert _cli(zk, tmp_path, "challenge", "contribute", "bls12381", "challenge", "r2").returncode == 2
    assert _cli(zk, tmp_path, "import", "response", new, "response").returncode == 2
    assert _cli(zk, tmp_path, "challenge", "contribute", "bn128").returncode == 2
    assert not (tmp_path / "r2").exists() and _no_leftovers(tmp_path)


# what ZKPOA_VERBOSE=1 prints on stderr, per command: (arguments, command name, width of the label column, labels in order)
VERBOSE = [
    (("new", "bn128", 2, "0.ptau"), "powersoftau new", 0, []),
    (("contribute", "0.ptau", "1.ptau", "--name=alice"), "powersoftau contribute", 34,
     ["sections, challenge, key", "read (file -> HBM)", "compute (checks, scalars, products)",
      "hashes (response, nextChallenge)", "write (HBM -> file; overlaps the rest)",
      "sections 2-7 written, file renamed into place"]),
    (("export", "challenge", "1.ptau", "challenge"), "powersoftau export challenge", 40,
     ["sections, records", "read (file -> HBM)", "convert (waiting for the device)", "hash (Blake2b)",
      "write (challenge file)", "challenge written, file renamed into place"]),
    (("challenge", "contribute", "bn128", "challenge", "response"), "powersoftau challenge contribute", 40,
     ["challenge (Blake2b of the input)", "key", "read (file -> HBM)", "convert (hash form -> wire form)",
      "compute (checks, scalars, products)", "hash (compressed form, Blake2b)", "write (response file)",
      "response written, file renamed into place"]),
    (("import", "response", "1.ptau", "response", "2.ptau", "--name=bob"), "powersoftau import response", 40,
     ["old file, response, key", "read (file -> HBM)", "decompress (waiting for the device)", "checks (curve, G2 subgroup)",
      "hashes (response, nextChallenge)", "write (HBM -> file; overlaps the rest)",
      "sections 2-7 written, file renamed into place"]),
]


@gpu
def test_cli_verbose_lines(zk, tmp_path):
    """Power 2, one process per command: the `zkpoa: <command>: <label>` lines of ZKPOA_VERBOSE, in order, each label
    padded to the command's column width and followed by " %8.1f ms" (the milliseconds themselves are not compared)."""
    for args, command, width, labels in VERBOSE:
        rc = subprocess.run([zk.SETUP_BIN, "powersoftau"] + [str(a) for a in args], cwd=tmp_path, capture_output=True,
                            text=True, timeout=600, env=dict(os.environ, ZKPOA_VERBOSE="1"))
        assert rc.returncode == 0, rc.stderr
        lines = [ln for ln in rc.stderr.splitlines() if ln.startswith("zkpoa: powersoftau ")]
        assert [ln[:-12] for ln in lines] == ["zkpoa: %s: %s" % (command, what.ljust(width)) for what in labels], rc.stderr
        for ln in lines:
            assert ln.endswith(" ms") and ln[-12] == " " and float(ln[-11:-3]) >= 0, ln
    assert _no_leftovers(tmp_path)
