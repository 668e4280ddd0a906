"""`snarkjs zkey verify <circuit.r1cs> <pot.ptau> <circuit.zkey>` on the device (csrc/setup.hip zkey_verify, C ABI
zkpoa_zkey_verify, `zkpoa-setup zkey verify`; scripts/g16_verify.sh -z). Good keys -- from `zkey new`, after one and two
contributions, and written by the oracle's own setup from the same toxic waste -- pass; every kind of tampering sets
exactly the check bit it breaks (the untampered key passing in the same test); malformed files are errors; the G2
subgroup pass agrees with the oracle's [r]Q == O point by point."""
import os
import random
import subprocess
import time

import pytest

from conftest import le
from oracle import c_oracle as co
from oracle.py import bn254 as bn

pytestmark = pytest.mark.gpu
R, Q = bn.R, bn.Q


def _fb1(ks):
    return co.fixed_base_g1(b"".join(le(k % R) for k in ks), 8)


def _fb2(ks):
    return co.fixed_base_g2(b"".join(le(k % R) for k in ks), 8)


def _circuit(rng, n_vars, n_public, n_cons, long_row=False, sparse_b=True):
    """Constraints that need not be satisfiable (zkey verify reads no witness). B uses the lower half of the wires
    only (sparse_b), so the upper signals' B2 points are at infinity; long_row adds one A row of 300 terms."""
    cons = []
    for c in range(n_cons):
        a = {rng.randrange(n_vars): rng.choice([1, R - 1, 7, rng.randrange(R)]) for _ in range(rng.randrange(1, 4))}
        b = {rng.randrange(max(1, n_vars // 2) if sparse_b else n_vars): rng.choice([1, 3, rng.randrange(R)])}
        cc = {rng.randrange(n_vars): 1}
        cons.append((a, b, cc))
    if long_row:
        cons[len(cons) // 2] = ({s: rng.randrange(1, R) for s in rng.sample(range(n_vars), 300)}, {0: 1}, {1: 5})
    return cons


def _files(tmp_path, rng, n_vars, n_public, cons, extra_power=0, tau=None):
    from setup_files import write_ptau, write_r1cs
    tox = {"tau": tau or rng.randrange(2, R), "alpha": rng.randrange(2, R), "beta": rng.randrange(2, R), "gamma": 1,
           "delta": 1}
    n = 1
    while n < len(cons) + n_public + 1:
        n <<= 1
    (tmp_path / "c.r1cs").write_bytes(write_r1cs(n_vars, n_public, cons))
    (tmp_path / "pot.ptau").write_bytes(write_ptau(n.bit_length() - 1 + extra_power, tox["tau"], tox["alpha"],
                                                   tox["beta"]))
    return tox, n


def _secs(buf):
    from oracle.py import groth16 as g16
    return {t: lst[0] for t, lst in g16.read_binfile(buf, "zkey", 1).items()}


def _cli(zk, tmp_path, *args, env=None):
    return subprocess.run([zk.SETUP_BIN, "zkey", "verify"] + list(args), cwd=tmp_path, capture_output=True, text=True,
                          timeout=600, env=env)


@pytest.mark.parametrize("n_vars,n_public,n_cons,long_row,extra_power", [
    (20, 0, 9, False, 0),          # no public signal; B2 points at infinity
    (400, 1, 40, True, 1),         # a 300-term constraint (the one-wave-per-row path); a ceremony larger than needed
    (30, 3, 60, False, 0),         # several public signals; nC + nPublic + 1 = 64 = n: the domain filled exactly
])
def test_good_keys_pass(ctx, zk, tmp_path, n_vars, n_public, n_cons, long_row, extra_power):
    from oracle.py import groth16 as g16
    rng = random.Random(n_vars * 7 + n_cons)
    cons = _circuit(rng, n_vars, n_public, n_cons, long_row)
    tox, n = _files(tmp_path, rng, n_vars, n_public, cons, extra_power)
    ctx.zkey_new(tmp_path / "c.r1cs", tmp_path / "pot.ptau", tmp_path / "c_0.zkey")
    want0, _ = g16.synthetic_setup(n_vars, n_public, cons, tox, g1_batch=_fb1, g2_batch=_fb2)
    assert (tmp_path / "c_0.zkey").read_bytes() == want0
    assert ctx.zkey_verify(tmp_path / "c.r1cs", tmp_path / "pot.ptau", tmp_path / "c_0.zkey") == 0
    rc = _cli(zk, tmp_path, "c.r1cs", "pot.ptau", "c_0.zkey")
    assert rc.returncode == 0 and "ZKey Ok!" in rc.stdout, rc.stderr
    assert "no contribution" in rc.stderr and "section 10" in rc.stderr
    # one contribution (C ABI), a second through the executable with ZKPOA_DELTA
    d1, d2 = rng.randrange(1, R), rng.randrange(1, R)
    ctx.zkey_contribute(tmp_path / "c_0.zkey", tmp_path / "c_1.zkey", d1)
    assert ctx.zkey_verify(tmp_path / "c.r1cs", tmp_path / "pot.ptau", tmp_path / "c_1.zkey") == 0
    rc = subprocess.run([zk.SETUP_BIN, "zkey", "contribute", "c_1.zkey", "c_2.zkey", "--name=x"], cwd=tmp_path,
                        capture_output=True, text=True, timeout=300, env=dict(os.environ, ZKPOA_DELTA=str(d2)))
    assert rc.returncode == 0, rc.stderr
    rc = _cli(zk, tmp_path, "c.r1cs", "pot.ptau", "c_2.zkey", "-v", "--ignored=1")
    assert rc.returncode == 0 and "ZKey Ok!" in rc.stdout, rc.stderr
    assert "no contribution" not in rc.stderr
    # the oracle's own key from the same toxic waste (independent of the device code), delta = d1 * d2
    want2, _ = g16.synthetic_setup(n_vars, n_public, cons, dict(tox, delta=d1 * d2 % R), g1_batch=_fb1, g2_batch=_fb2)
    assert (tmp_path / "c_2.zkey").read_bytes() == want2
    (tmp_path / "o.zkey").write_bytes(want2)
    assert ctx.zkey_verify(tmp_path / "c.r1cs", tmp_path / "pot.ptau", tmp_path / "o.zkey") == 0


def _g1_double(buf, off):
    from oracle.py import groth16 as g16
    P = g16.g1_from_bytes(buf, off)
    return g16.g1_to_bytes(bn.g1_add(P, P))


def _g2_double(buf, off):
    from oracle.py import groth16 as g16
    P = g16.g2_from_bytes(buf, off)
    return g16.g2_to_bytes(bn.g2_add(P, P))


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


def test_tampered_keys_fail_with_their_bit(ctx, zk, tmp_path):
    from oracle.py import groth16 as g16
    from setup_files import write_ptau, write_r1cs
    B = zk.ZKEY_CHECKS
    rng = random.Random(2024)
    n_vars, n_public = 40, 2
    cons = _circuit(rng, n_vars, n_public, 50)
    tox, n = _files(tmp_path, rng, n_vars, n_public, cons)
    ctx.zkey_new(tmp_path / "c.r1cs", tmp_path / "pot.ptau", tmp_path / "c_0.zkey")
    ctx.zkey_contribute(tmp_path / "c_0.zkey", tmp_path / "c.zkey", rng.randrange(1, R))
    good = (tmp_path / "c.zkey").read_bytes()
    s = _secs(good)
    verify = lambda name="t.zkey", r1cs="c.r1cs", ptau="pot.ptau": ctx.zkey_verify(tmp_path / r1cs, tmp_path / ptau,
                                                                                    tmp_path / name)
    assert verify("c.zkey") == 0

    def tampered(at, data):
        b = bytearray(good)
        b[at:at + len(data)] = data
        (tmp_path / "t.zkey").write_bytes(bytes(b))
        return verify()
    # one point of a point section replaced by its double (a valid point of the same group)
    for sec, bit in ((3, "ICCH"), (5, "A"), (6, "B1"), (7, "B2"), (8, "ICCH"), (9, "ICCH")):
        unit = 128 if sec == 7 else 64
        off = s[sec][0]
        cnt = s[sec][1] // unit
        i = next(j for j in range(cnt) if any(good[off + unit * j:off + unit * (j + 1)]))   # a point not at infinity
        at = off + unit * i
        got = tampered(at, (_g2_double if sec == 7 else _g1_double)(good, at))
        assert got == B[bit], (sec, got)
    h = s[2][0]
    kHdr = 84
    # section 4: a coefficient value changed; a record's signal index changed
    rec0 = s[4][0] + 4
    assert tampered(rec0 + 12, le((int.from_bytes(good[rec0 + 12:rec0 + 44], "little") + 1) % R)) == B["COEFFS"]
    sig = int.from_bytes(good[rec0 + 8:rec0 + 12], "little")
    assert tampered(rec0 + 8, ((sig + 1) % n_vars).to_bytes(4, "little")) == B["COEFFS"]
    # delta1 changed alone; gamma2 changed; alpha1 from another ceremony
    assert tampered(h + kHdr + 384, _g1_double(good, h + kHdr + 384)) == B["DELTA"]
    assert tampered(h + kHdr + 256, _g2_double(good, h + kHdr + 256)) == B["HEADER"]
    assert tampered(h + kHdr, _fb1([rng.randrange(2, R)])) == B["HEADER"]
    # a G1 point moved off the curve (y + 1, still a field element)
    at = s[5][0] + 64 * next(j for j in range(n_vars) if any(good[s[5][0] + 64 * j:s[5][0] + 64 * j + 64]))
    y = bn.from_mont(int.from_bytes(good[at + 32:at + 64], "little"), Q)
    assert tampered(at + 32, le(bn.to_mont((y + 1) % Q, Q))) & B["POINTS"]
    # a B2 point replaced by a twist point outside G2
    P = _twist_points_outside_g2(rng, 1)[0]
    assert tampered(s[7][0], g16.g2_to_bytes(P)) & B["POINTS"]
    # the right key against an r1cs with one coefficient changed; against a ptau with the same alpha, beta, another tau
    bad_cons = [tuple(dict(lc) for lc in c) for c in cons]
    s0 = next(iter(bad_cons[3][0]))
    bad_cons[3][0][s0] = (bad_cons[3][0][s0] + 1) % R
    (tmp_path / "bad.r1cs").write_bytes(write_r1cs(n_vars, n_public, bad_cons))
    assert verify("c.zkey", r1cs="bad.r1cs") & B["COEFFS"]
    (tmp_path / "tau.ptau").write_bytes(write_ptau(n.bit_length() - 1, (tox["tau"] + 1) % R, tox["alpha"], tox["beta"]))
    assert verify("c.zkey", ptau="tau.ptau") & B["A"]
    assert verify("c.zkey") == 0
    # the CLI names a failed check on stderr and exits 1
    tampered(at, _g1_double(good, at))
    rc = _cli(zk, tmp_path, "c.r1cs", "pot.ptau", "t.zkey")
    assert rc.returncode == 1 and "[ERROR]" in rc.stderr and "A:" in rc.stderr and "ZKey Ok!" not in rc.stdout


def test_malformed_files_are_errors(ctx, zk, tmp_path):
    import struct
    from setup_files import write_r1cs
    rng = random.Random(31)
    n_vars, n_public = 24, 1
    cons = _circuit(rng, n_vars, n_public, 20)
    _files(tmp_path, rng, n_vars, n_public, cons)
    ctx.zkey_new(tmp_path / "c.r1cs", tmp_path / "pot.ptau", tmp_path / "c.zkey")
    good = (tmp_path / "c.zkey").read_bytes()
    s = _secs(good)
    cases = {"truncated.zkey": good[:len(good) - 100],
             "seclen.zkey": good[:s[5][0] - 8] + struct.pack("<Q", s[5][1] - 64) + good[s[5][0]:s[5][0] + s[5][1] - 64]
             + good[s[5][0] + s[5][1]:],
             "magic.zkey": b"zkex" + good[4:]}
    for name, data in cases.items():
        (tmp_path / name).write_bytes(data)
        with pytest.raises(zk.ZkpoaError):
            ctx.zkey_verify(tmp_path / "c.r1cs", tmp_path / "pot.ptau", tmp_path / name)
        rc = _cli(zk, tmp_path, "c.r1cs", "pot.ptau", name)
        assert rc.returncode == 1 and "zkpoa-setup:" in rc.stderr, (name, rc.stderr)
    # the key of a circuit with one more wire: nVars differs from the r1cs
    (tmp_path / "more.r1cs").write_bytes(write_r1cs(n_vars + 1, n_public, cons))
    with pytest.raises(zk.ZkpoaError, match="nVars"):
        ctx.zkey_verify(tmp_path / "more.r1cs", tmp_path / "pot.ptau", tmp_path / "c.zkey")
    rc = _cli(zk, tmp_path, "more.r1cs", "pot.ptau", "c.zkey")
    assert rc.returncode == 1 and "nVars" in rc.stderr
    # a coefficient >= r in section 4
    b = bytearray(good)
    b[s[4][0] + 4 + 12:s[4][0] + 4 + 44] = le(R)
    (tmp_path / "coef.zkey").write_bytes(bytes(b))
    with pytest.raises(zk.ZkpoaError, match="field element"):
        ctx.zkey_verify(tmp_path / "c.r1cs", tmp_path / "pot.ptau", tmp_path / "coef.zkey")
    # wrong argument count
    rc = subprocess.run([zk.SETUP_BIN, "zkey", "verify", "c.r1cs", "c.zkey"], cwd=tmp_path, capture_output=True, text=True)
    assert rc.returncode == 2 and "usage" in rc.stderr
    # the context is still usable
    assert ctx.zkey_verify(tmp_path / "c.r1cs", tmp_path / "pot.ptau", tmp_path / "c.zkey") == 0


def test_subgroup_pass_matches_the_oracle(ctx, zk, tmp_path):
    """Multiples of the G2 generator, twist points outside G2 and the point at infinity, each put into section 7 of a
    good key in turn: the POINTS bit is set exactly when the oracle's [r]Q != O."""
    from oracle.py import groth16 as g16
    rng = random.Random(77)
    n_vars, n_public = 16, 1
    cons = _circuit(rng, n_vars, n_public, 10, sparse_b=False)
    _files(tmp_path, rng, n_vars, n_public, cons)
    ctx.zkey_new(tmp_path / "c.r1cs", tmp_path / "pot.ptau", tmp_path / "c.zkey")
    good = (tmp_path / "c.zkey").read_bytes()
    s = _secs(good)
    batch = [bn.g2_mul(bn.G2_GEN, k) for k in (1, 2, R - 1, rng.randrange(R))] + [None] + \
        _twist_points_outside_g2(rng, 6)
    bit = zk.ZKEY_CHECKS["POINTS"]
    for i, P in enumerate(batch):
        outside = P is not None and bn.ec_mul(P, R, bn.FQ2, order=R * R) is not None
        b = bytearray(good)
        at = s[7][0] + 128 * (i % n_vars)
        b[at:at + 128] = g16.g2_to_bytes(P)
        (tmp_path / "t.zkey").write_bytes(bytes(b))
        got = ctx.zkey_verify(tmp_path / "c.r1cs", tmp_path / "pot.ptau", tmp_path / "t.zkey")
        assert bool(got & bit) == outside, (i, got)


def test_layer_one_shape(ctx, zk, tmp_path):
    """zkey new -> contribute -> zkey verify at the layer_one(2 sigs) shape (2^21 domain, 2,083,343 wires); one point in
    the middle of section 8 replaced by its double then fails with ICCH."""
    from setup_files import write_full_shape_inputs
    write_full_shape_inputs(ctx, 21, 2083343, str(tmp_path), seed=3, n_public=1)
    for args in (["zkey", "new", "c.r1cs", "pot.ptau", "c_0.zkey"], ["zkey", "contribute", "c_0.zkey", "c.zkey"]):
        rc = subprocess.run([zk.SETUP_BIN] + args, cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert rc.returncode == 0, rc.stderr
    (tmp_path / "c_0.zkey").unlink()
    t0 = time.time()
    rc = _cli(zk, tmp_path, "c.r1cs", "pot.ptau", "c.zkey")
    t_verify = time.time() - t0
    assert rc.returncode == 0 and "ZKey Ok!" in rc.stdout, rc.stderr
    with open(tmp_path / "c.zkey", "r+b") as f:
        buf = f.read()
        s = _secs(buf)
        at = s[8][0] + 64 * (s[8][1] // 128)
        f.seek(at)
        f.write(_g1_double(buf, at))
    del buf
    assert ctx.zkey_verify(tmp_path / "c.r1cs", tmp_path / "pot.ptau", tmp_path / "c.zkey") == zk.ZKEY_CHECKS["ICCH"]
    print("layer-one shape: zkpoa-setup zkey verify %.2f s (CLI, wall)" % t_verify)
