"""`snarkjs powersoftau verify <pot.ptau>` on the device (csrc/ptau_verify.hip, C ABI zkpoa_ptau_verify,
`zkpoa-setup powersoftau verify`). Good files -- prepared or not, several powers, random tau, alpha, beta -- pass; each
kind of tampering sets exactly the bits the math predicts (the untampered file passing in the same test); the G2
subgroup test agrees with the oracle's [r]Q == O point by point in sections 3 and 13; malformed files are errors; the
piece size changes nothing; and a consistent file at the layer-one ceremony size passes."""
import random
import struct
import subprocess
import time

import pytest

from conftest import le
from oracle import c_oracle as co
from oracle.py import bn254 as bn
from oracle.py import groth16 as g16

pytestmark = pytest.mark.gpu
R, Q = bn.R, bn.Q


def _fb1(ks):
    return co.fixed_base_g1(b"".join(le(k % R) for k in ks), 8)


def _fb2(ks):
    return co.fixed_base_g2(b"".join(le(k % R) for k in ks), 8)


def _ptau(power, tau, alpha, beta):
    from setup_files import write_ptau
    return write_ptau(power, tau, alpha, beta)


def _sections(buf):
    """[(type, payload)] in file order"""
    return [(t, buf[off:off + ln]) for t, lst in g16.read_binfile(buf, "ptau", 1).items() for off, ln in lst]


def _offsets(buf):
    return {t: lst[0] for t, lst in g16.read_binfile(buf, "ptau", 1).items()}


def _rebuild(buf, replace=None, drop=()):
    replace = replace or {}
    return g16.write_binfile("ptau", 1, [(t, replace.get(t, p)) for t, p in _sections(buf) if t not in drop])


def _cli(zk, cwd, *args):
    return subprocess.run([zk.SETUP_BIN, "powersoftau", "verify"] + list(args), cwd=cwd, capture_output=True, text=True,
                          timeout=600)


def _g1_double(buf, off):
    P = g16.g1_from_bytes(buf, off)
    return g16.g1_to_bytes(bn.g1_add(P, P))


def _g2_double(buf, off):
    P = g16.g2_from_bytes(buf, off)
    return g16.g2_to_bytes(bn.g2_add(P, P))


def _patch(buf, at, data):
    b = bytearray(buf)
    b[at:at + len(data)] = data
    return bytes(b)


def _lag_at(power, sec, level, j):
    """byte offset, inside its section, of point j of a level of Lagrange section sec"""
    unit = 128 if sec == 13 else 64
    return unit * ((1 << level) - 1 + j)


@pytest.mark.parametrize("power", [1, 3, 7])
def test_good_files_pass(ctx, zk, tmp_path, power):
    rng = random.Random(power)
    good = _ptau(power, rng.randrange(2, R), rng.randrange(2, R), rng.randrange(2, R))
    (tmp_path / "pot.ptau").write_bytes(good)
    assert ctx.ptau_verify(tmp_path / "pot.ptau") == (0, (power, power, 1, 0))
    rc = _cli(zk, tmp_path, "pot.ptau")
    assert rc.returncode == 0 and "Powers of Tau Ok!" in rc.stdout, rc.stderr
    assert "section 7" in rc.stderr and "[ERROR]" not in rc.stderr and "not prepared" not in rc.stderr
    # the same file without sections 12-15: only the powers are checked
    (tmp_path / "raw.ptau").write_bytes(_rebuild(good, drop=(12, 13, 14, 15)))
    assert ctx.ptau_verify(tmp_path / "raw.ptau") == (0, (power, power, 0, 0))
    rc = _cli(zk, tmp_path, "raw.ptau", "-v")
    assert rc.returncode == 0 and "Powers of Tau Ok!" in rc.stdout, rc.stderr
    assert "not prepared" in rc.stderr


def _tampered_cases(B, power, rng):
    """(name, file bytes, expected mask) for the good file and each kind of tampering"""
    tau, alpha, beta = rng.randrange(2, R), rng.randrange(2, R), rng.randrange(2, R)
    good = _ptau(power, tau, alpha, beta)
    s = _offsets(good)
    N = 1 << power
    cases = [("good", good, 0)]
    # one Lagrange point doubled in the middle of level p of each of 12-15
    for sec, bit in ((12, "LAGRANGE_TAU_G1"), (13, "LAGRANGE_TAU_G2"), (14, "LAGRANGE_ALPHA"), (15, "LAGRANGE_BETA")):
        at = s[sec][0] + _lag_at(power, sec, power, N // 2)
        cases.append(("lag%d" % sec, _patch(good, at, (_g2_double if sec == 13 else _g1_double)(good, at)), B[bit]))
    # the top level p+1 of section 12
    at = s[12][0] + _lag_at(power, 12, power + 1, N + 1)
    cases.append(("lag12top", _patch(good, at, _g1_double(good, at)), B["LAGRANGE_TAU_G1"]))
    # one T_i, 2 <= i <= 2N-2, replaced
    i = rng.randrange(2, 2 * N - 1)
    at = s[2][0] + 64 * i
    cases.append(("tau_i", _patch(good, at, _g1_double(good, at)), B["TAU_G1"] | B["LAGRANGE_TAU_G1"]))
    # section 14 made with another alpha
    other = _ptau(power, tau, rng.randrange(2, R), beta)
    o = _offsets(other)
    cases.append(("alpha14", _rebuild(good, {14: other[o[14][0]:o[14][0] + o[14][1]]}), B["LAGRANGE_ALPHA"]))
    # beta2 for another beta
    cases.append(("beta2", _rebuild(good, {6: _fb2([rng.randrange(2, R)])}), B["BETA"]))
    # U (and section 13, consistently) from another tau
    other = _ptau(power, rng.randrange(2, R), alpha, beta)
    o = _offsets(other)
    cases.append(("tau2", _rebuild(good, {t: other[o[t][0]:o[t][0] + o[t][1]] for t in (3, 13)}),
                  B["TAU_G1"] | B["TAU_G2"] | B["ALPHA"] | B["BETA"]))
    return cases, good, s


def test_tampering_sets_its_bits(ctx, zk, tmp_path):
    B = zk.PTAU_CHECKS
    power = 3
    cases, good, s = _tampered_cases(B, power, random.Random(2026))
    for name, data, want in cases:
        (tmp_path / "t.ptau").write_bytes(data)
        got, info = ctx.ptau_verify(tmp_path / "t.ptau")
        assert got == want, (name, hex(got), hex(want))
        assert info == (power, power, 1, 0)
    # an off-curve point (y + 1, still a field element) in the middle of section 15
    at = s[15][0] + 64 * (s[15][1] // 128)
    y = bn.from_mont(int.from_bytes(good[at + 32:at + 64], "little"), Q)
    (tmp_path / "t.ptau").write_bytes(_patch(good, at + 32, le(bn.to_mont((y + 1) % Q, Q))))
    got, _ = ctx.ptau_verify(tmp_path / "t.ptau")
    assert got & B["POINTS"] and not got & ~(B["POINTS"] | B["LAGRANGE_BETA"]), hex(got)
    # the CLI names each failed check on stderr and exits 1
    name, data, want = next(c for c in cases if c[0] == "tau2")
    (tmp_path / "t.ptau").write_bytes(data)
    rc = _cli(zk, tmp_path, "t.ptau")
    assert rc.returncode == 1 and "Powers of Tau Ok!" not in rc.stdout
    assert [ln.split(":")[1].strip() for ln in rc.stderr.splitlines() if ln.startswith("[ERROR]")] == \
        ["TAU_G1", "TAU_G2", "ALPHA", "BETA"], rc.stderr
    (tmp_path / "t.ptau").write_bytes(good)
    assert ctx.ptau_verify(tmp_path / "t.ptau")[0] == 0


def _fq_sqrt(a):
    r = pow(a, (Q + 1) // 4, Q)
    return r if r * r % Q == a % Q else None


def _fq2_sqrt(a):
    a0, a1 = a
    d = _fq_sqrt((a0 * a0 + a1 * a1) % Q)
    if d is None:
        return None
    inv2 = pow(2, -1, Q)
    for t in ((a0 + d) * inv2 % Q, (a0 - d) * inv2 % Q):
        c0 = _fq_sqrt(t)
        if c0:
            c1 = a1 * pow(2 * c0, -1, Q) % Q
            if bn.FQ2.eq(bn.FQ2.sqr((c0, c1)), a):
                return (c0, c1)
    return None


def _twist_points_outside_g2(rng, count):
    """Points of the twist y^2 = x^3 + 3 / (9 + u) that are not in G2, from random x and an Fq2 square root;
    [r]Q != O is asserted with the oracle."""
    out = []
    while len(out) < count:
        x = (rng.randrange(Q), rng.randrange(Q))
        y = _fq2_sqrt(bn.FQ2.add(bn.FQ2.mul(bn.FQ2.sqr(x), x), bn.B2))
        if y is None:
            continue
        P = (x, y)
        assert bn.g2_is_on_curve(P)
        assert bn.ec_mul(P, R, bn.FQ2, order=R * R) is not None          # outside G2
        out.append(P)
    return out


def test_subgroup_verdicts_match_the_oracle(ctx, zk, tmp_path):
    """Multiples of the G2 generator, infinity, twist points outside G2 and [r]P of such points (cofactor part only),
    each put into the middle of section 3 and of section 13 in turn: POINTS is set exactly when [r]P != O."""
    rng = random.Random(348)
    power = 3
    good = _ptau(power, rng.randrange(2, R), rng.randrange(2, R), rng.randrange(2, R))
    s = _offsets(good)
    outside = _twist_points_outside_g2(rng, 6)
    batch = [bn.g2_mul(bn.G2_GEN, k) for k in (1, 2, R - 1, rng.randrange(R))] + [None] + outside[:3] + \
        [bn.ec_mul(P, R, bn.FQ2, order=R * R) for P in outside[3:]]
    bit = zk.PTAU_CHECKS["POINTS"]
    N = 1 << power
    for i, P in enumerate(batch):
        want = P is not None and bn.ec_mul(P, R, bn.FQ2, order=R * R) is not None
        for at in (s[3][0] + 128 * (N // 2), s[13][0] + _lag_at(power, 13, power, N // 2)):
            (tmp_path / "t.ptau").write_bytes(_patch(good, at, g16.g2_to_bytes(P)))
            got, _ = ctx.ptau_verify(tmp_path / "t.ptau")
            assert bool(got & bit) == want, (i, at, hex(got))


def test_malformed_files_are_errors(ctx, zk, tmp_path):
    rng = random.Random(99)
    power = 2
    good = _ptau(power, rng.randrange(2, R), rng.randrange(2, R), rng.randrange(2, R))
    s = _offsets(good)
    secs = dict(_sections(good))
    hdr = secs[1]
    cases = {
        "coord.ptau": (_patch(good, s[2][0] + 64 * 3, le(Q)), "field element"),
        "short12.ptau": (_rebuild(good, {12: secs[12][:-64]}), "section 12"),
        "len2.ptau": (_rebuild(good, {2: secs[2][:-64]}), "section 2"),
        "empty23.ptau": (_rebuild(good, {2: b"", 3: b""}), "section 2"),
        "no3.ptau": (_rebuild(good, drop=(3,)), "section 3 missing"),
        "q.ptau": (_rebuild(good, {1: hdr[:4] + le(Q + 2) + hdr[36:]}), "BN254"),
        "magic.ptau": (b"ptax" + good[4:], "magic"),
        "truncated.ptau": (good[:len(good) - 100], "past the end"),
    }
    for name, (data, msg) in cases.items():
        (tmp_path / name).write_bytes(data)
        with pytest.raises(zk.ZkpoaError, match=msg):
            ctx.ptau_verify(tmp_path / name)
        rc = _cli(zk, tmp_path, name)
        assert rc.returncode != 0 and "zkpoa-setup:" in rc.stderr and msg in rc.stderr, (name, rc.stderr)
    rc = subprocess.run([zk.SETUP_BIN, "powersoftau", "verify"], cwd=tmp_path, capture_output=True, text=True)
    assert rc.returncode == 2 and "usage" in rc.stderr
    # the context is still usable
    (tmp_path / "pot.ptau").write_bytes(good)
    assert ctx.ptau_verify(tmp_path / "pot.ptau")[0] == 0


def test_piece_size_changes_nothing(ctx, zk, tmp_path):
    """Pieces of 3, 7 and 64 points put boundaries at odd offsets inside levels and across them."""
    power = 5
    cases, _, _ = _tampered_cases(zk.PTAU_CHECKS, power, random.Random(5))
    for name, data, want in cases:
        if name not in ("good", "lag12", "lag13", "lag12top", "tau_i", "tau2"):
            continue
        (tmp_path / "t.ptau").write_bytes(data)
        for piece in (0, 3, 7, 64):
            got, _ = ctx.ptau_verify(tmp_path / "t.ptau", piece_points=piece)
            assert got == want, (name, piece, hex(got), hex(want))


def test_layer_one_ceremony_size(ctx, zk, tmp_path):
    """A consistent power-21 file made on the device (tau powers on the host, Lagrange values by the oracle's inverse
    NTT per level, points by zkpoa_setup_accumulate from one base point each) passes; one doubled point in the middle
    of level p of section 14 then gives LAGRANGE_ALPHA."""
    import torch
    power = 21
    N = 1 << power
    rng = random.Random(21)
    tau, alpha, beta = rng.randrange(2, R), rng.randrange(2, R), rng.randrange(2, R)
    t0 = time.time()
    pw = [1]
    for _ in range(2 * N - 1):
        pw.append(pw[-1] * tau % R)
    pw_b = b"".join(x.to_bytes(32, "little") for x in pw)
    del pw
    lag = [co.ntt(pw_b[:32 << lvl], lvl, inverse=True) for lvl in range(power + 2)]

    def points(group, bases, base_idx, coefs):
        cnt = len(coefs) // 32
        size = 64 if group == 1 else 128
        d_pts = torch.frombuffer(bytearray(bases), dtype=torch.uint8).cuda()
        d_coef = torch.frombuffer(bytearray(coefs), dtype=torch.uint8).cuda()
        d_pidx = torch.full((cnt,), base_idx, dtype=torch.int32, device="cuda")
        d_sig = torch.arange(cnt, dtype=torch.int32, device="cuda")
        out = torch.empty(cnt * size, dtype=torch.uint8, device="cuda")
        ctx.setup_accumulate(group, d_pts.data_ptr(), len(bases) // size, d_coef.data_ptr(), d_pidx.data_ptr(),
                             d_sig.data_ptr(), cnt, cnt, out.data_ptr())
        return out.cpu().numpy().tobytes()
    g1 = g16.g1_to_bytes(bn.G1_GEN) + _fb1([alpha, beta])
    g2 = g16.g2_to_bytes(bn.G2_GEN)
    lag_p = b"".join(lag[:power + 1])
    secs = [(1, struct.pack("<I", 32) + le(Q) + struct.pack("<II", power, power)),
            (2, points(1, g1, 0, pw_b[:32 * (2 * N - 1)])), (3, points(2, g2, 0, pw_b[:32 * N])),
            (4, points(1, g1, 1, pw_b[:32 * N])), (5, points(1, g1, 2, pw_b[:32 * N])), (6, _fb2([beta])),
            (7, struct.pack("<I", 0)), (12, points(1, g1, 0, b"".join(lag))), (13, points(2, g2, 0, lag_p)),
            (14, points(1, g1, 1, lag_p)), (15, points(1, g1, 2, lag_p))]
    del pw_b, lag, lag_p
    with open(tmp_path / "pot.ptau", "wb") as f:
        f.write(b"ptau" + struct.pack("<II", 1, len(secs)))
        for sid, payload in secs:
            f.write(struct.pack("<IQ", sid, len(payload)))
            f.write(payload)
    pos = 12
    for sid, payload in secs:
        pos += 12
        if sid == 14:
            rel = _lag_at(power, 14, power, N // 2)
            at, double = pos + rel, _g1_double(payload, rel)
        pos += len(payload)
    del secs
    t_files = time.time() - t0
    t0 = time.time()
    rc = _cli(zk, tmp_path, "pot.ptau")
    t_verify = time.time() - t0
    assert rc.returncode == 0 and "Powers of Tau Ok!" in rc.stdout, rc.stderr
    with open(tmp_path / "pot.ptau", "r+b") as f:
        f.seek(at)
        f.write(double)
    assert ctx.ptau_verify(tmp_path / "pot.ptau") == (zk.PTAU_CHECKS["LAGRANGE_ALPHA"], (power, power, 1, 0))
    print("power %d: file made in %.1f s; zkpoa-setup powersoftau verify %.2f s (CLI, wall)" % (power, t_files, t_verify))
