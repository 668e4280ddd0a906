"""`snarkjs powersoftau prepare phase2 <in.ptau> <out.ptau>` on the device (csrc/ptau_prepare.hip, csrc/ec_ntt.hip.h; C ABI
zkpoa_ec_intt_device and zkpoa_ptau_prepare_phase2; `zkpoa-setup powersoftau prepare phase2`).

Every expected byte comes from the oracle, never from the code under test: the discrete logs of the input points go
through the C oracle's field transform `co.ntt(..., inverse=True)` and then through its fixed-base products.

The top level (power + 1) of section 12 is, as in snarkjs, the transform of the 2N - 1 points of section 2 and one point
at infinity. `setup_files.write_ptau` fills that one level with L_j(tau) of the full 2N-point domain, which needs
tau^(2N-1) G1 -- a point no ceremony file holds -- so that level of its files cannot be reproduced from their powers
(`powersoftau verify` accepts both: it checks the level on the 2N - 1 powers that exist). The comparisons with
write_ptau's files therefore cover sections 13-15 and levels 0..power of section 12 byte for byte, and the top level of
section 12 is compared with the oracle's transform of the 2N - 1 powers and a zero."""
import random
import struct
import subprocess
import time

import pytest

from conftest import le
from oracle import c_oracle as co
from oracle.py import bn254 as bn
from oracle.py import groth16 as g16
from test_gpu_ptau_verify import _offsets, _patch, _rebuild, _sections, _twist_points_outside_g2

pytestmark = pytest.mark.gpu
R, Q = bn.R, bn.Q
ORDER = [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]
# one butterfly per thread in workgroups of 64 (csrc/ec_ntt.hip.h kEcNttThreads), the same kernels at every size
BUTTERFLIES_PER_WORKGROUP = 64


def _fb(group, ks):
    data = b"".join(le(k % R) for k in ks)
    return co.fixed_base_g1(data, 8) if group == 1 else co.fixed_base_g2(data, 8)


def _intt_scalars(ks, log_n):
    out = co.ntt(b"".join(le(k % R) for k in ks), log_n, inverse=True)
    return [int.from_bytes(out[32 * i:32 * i + 32], "little") for i in range(1 << log_n)]


def _expected(group, ks, log_n):
    return _fb(group, _intt_scalars(ks, log_n))


def _device_intt(ctx, group, points, log_n, in_place):
    import torch
    d_in = torch.frombuffer(bytearray(points), dtype=torch.uint8).cuda()
    d_out = d_in if in_place else torch.empty_like(d_in)
    ctx.ec_intt(group, d_in.data_ptr(), log_n, d_out.data_ptr())
    if not in_place:
        assert d_in.cpu().numpy().tobytes() == points          # the input is left as it was
    return d_out.cpu().numpy().tobytes()


def _cli(zk, cwd, *args):
    return subprocess.run([zk.SETUP_BIN, "powersoftau", "prepare", "phase2"] + [str(a) for a in args], cwd=cwd,
                          capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("group,log_n", [(1, k) for k in (0, 1, 2, 3, 5, 8, 11)] + [(2, k) for k in (0, 1, 3, 6, 9)])
def test_ec_intt_matches_oracle(ctx, group, log_n):
    """Random multiples of the generator, out of place and in place. There is no size threshold: every size runs the
    load, stage and store kernels of csrc/ec_ntt.hip.h, n / 2 butterflies in workgroups of 64. Sizes up to 2^7 points are
    one workgroup per stage; G1 2^8 is 2, G1 2^11 is 16 and G2 2^9 is 4 workgroups (asserted below for the largest)."""
    rng = random.Random(1000 * group + log_n)
    ks = [rng.randrange(1, R) for _ in range(1 << log_n)]
    points = _fb(group, ks)
    want = _expected(group, ks, log_n)
    assert _device_intt(ctx, group, points, log_n, False) == want
    assert _device_intt(ctx, group, points, log_n, True) == want
    if (group, log_n) in ((1, 11), (2, 9)):
        assert (1 << (log_n - 1)) // BUTTERFLIES_PER_WORKGROUP > 1


@pytest.mark.parametrize("group", [1, 2])
def test_ec_intt_edge_points(ctx, group):
    """The exceptional cases of the additions, 16 points: P + P and P - P in every first-stage butterfly, all infinity,
    P and -P alternating, a single point, and an upper half at infinity (the top level of section 12 in miniature)."""
    rng = random.Random(40 + group)
    k = rng.randrange(1, R)
    n = 16
    cases = {
        "all equal": [k] * n,
        "all zero": [0] * n,
        "k, r - k": [k if i % 2 == 0 else R - k for i in range(n)],
        "single": [k if i == 5 else 0 for i in range(n)],
        "upper half zero": [rng.randrange(1, R) if i < n // 2 else 0 for i in range(n)],
    }
    assert _fb(group, [0]) == bytes(64 * group)                  # the oracle's infinity is the all-zero point
    for name, ks in cases.items():
        points = _fb(group, ks)
        want = _expected(group, ks, 4)
        assert _device_intt(ctx, group, points, 4, False) == want, name
        assert _device_intt(ctx, group, points, 4, True) == want, name


def _powers(power, tau, alpha, beta):
    """{source section: (group, discrete logs of its points)}"""
    n = 1 << power
    pw = [1]
    for _ in range(2 * n - 2):
        pw.append(pw[-1] * tau % R)
    return {2: (1, pw), 3: (2, pw[:n]), 4: (1, [alpha * x % R for x in pw[:n]]), 5: (1, [beta * x % R for x in pw[:n]])}


def _raw_ptau(power, tau, alpha, beta):
    """Sections 1-7 of a ceremony file, made by the oracle."""
    src = _powers(power, tau, alpha, beta)
    hdr = struct.pack("<I", 32) + le(Q) + struct.pack("<II", power, power)
    secs = [(1, hdr)] + [(t, _fb(*src[t])) for t in (2, 3, 4, 5)] + [(6, _fb(2, [beta])), (7, struct.pack("<I", 0))]
    return g16.write_binfile("ptau", 1, secs)


def _level_scalars(power, tau, alpha, beta, sec, level, cache={}):
    """Discrete logs of the points of a level of Lagrange section sec: co.ntt over the first 2^level source scalars
    (section 12's top level: the 2N - 1 powers and a zero)."""
    key = (power, tau, alpha, beta, sec, level)
    if key not in cache:
        _, ks = _powers(power, tau, alpha, beta)[sec - 10]
        ks = (ks + [0])[:1 << level] if sec == 12 else ks[:1 << level]
        cache[key] = _intt_scalars(ks, level)
    return cache[key]


def _lagrange_section(power, tau, alpha, beta, sec):
    group = 2 if sec == 13 else 1
    top = power + 1 if sec == 12 else power
    return b"".join(_fb(group, _level_scalars(power, tau, alpha, beta, sec, lvl)) for lvl in range(top + 1))


@pytest.mark.parametrize("power", [1, 3, 7])
def test_prepare_reproduces_the_oracle_file(ctx, zk, tmp_path, power):
    from setup_files import write_ptau
    rng = random.Random(700 + power)
    tau, alpha, beta = rng.randrange(2, R), rng.randrange(2, R), rng.randrange(2, R)
    good = write_ptau(power, tau, alpha, beta)
    raw = _rebuild(good, drop=(12, 13, 14, 15))
    (tmp_path / "good.ptau").write_bytes(good)
    (tmp_path / "raw.ptau").write_bytes(raw)
    assert ctx.ptau_prepare_phase2(tmp_path / "raw.ptau", tmp_path / "out.ptau") == (power, power, 0, 0)
    out = (tmp_path / "out.ptau").read_bytes()
    secs, want = dict(_sections(out)), dict(_sections(good))
    assert [t for t, _ in _sections(out)] == ORDER
    for t in range(1, 8):
        assert secs[t] == dict(_sections(raw))[t], t
    for t in (13, 14, 15):
        assert secs[t] == want[t], t
    below_top = 64 * ((2 << power) - 1)                        # levels 0..power of section 12
    assert secs[12][:below_top] == want[12][:below_top]
    assert secs[12] == _lagrange_section(power, tau, alpha, beta, 12)   # ... and its top level (see the module docstring)
    assert ctx.ptau_verify(tmp_path / "out.ptau") == (0, (power, power, 1, 0))
    # sections 12-15 of the input are ignored: the prepared file gives the same bytes
    assert ctx.ptau_prepare_phase2(tmp_path / "good.ptau", tmp_path / "again.ptau") == (power, power, 1, 0)
    assert (tmp_path / "again.ptau").read_bytes() == out
    rc = _cli(zk, tmp_path, "raw.ptau", "cli.ptau", "-v")
    assert rc.returncode == 0 and "[INFO]  zkpoa: Prepared phase 2" in rc.stdout, rc.stderr
    assert (tmp_path / "cli.ptau").read_bytes() == out


@pytest.mark.parametrize("which", ["one", "root"])
def test_special_tau(ctx, zk, tmp_path, which):
    """tau = 1 and tau = the primitive 8th root of unity at power 3: the Lagrange values are 0 and 1, so most output
    points are the point at infinity and the transforms meet it at every stage."""
    power = 3
    tau = 1 if which == "one" else bn.fr_root_of_unity(3)
    alpha, beta = 0x1234567, 0x7654321
    (tmp_path / "raw.ptau").write_bytes(_raw_ptau(power, tau, alpha, beta))
    ctx.ptau_prepare_phase2(tmp_path / "raw.ptau", tmp_path / "out.ptau")
    secs = dict(_sections((tmp_path / "out.ptau").read_bytes()))
    for t in (12, 13, 14, 15):
        assert secs[t] == _lagrange_section(power, tau, alpha, beta, t), t
    for t, unit in ((12, 64), (13, 128), (14, 64), (15, 64)):
        level3 = secs[t][unit * 7:unit * 15]
        assert sum(level3[unit * j:unit * (j + 1)] != bytes(unit) for j in range(8)) == 1, t


def test_power_12(ctx, zk, tmp_path):
    """A power-12 file: `powersoftau verify` accepts the result, and 32 points of each Lagrange section, among them the
    first point, the last point of the top level and points of seven more levels, match the oracle."""
    power = 12
    rng = random.Random(12)
    tau, alpha, beta = rng.randrange(2, R), rng.randrange(2, R), rng.randrange(2, R)
    (tmp_path / "raw.ptau").write_bytes(_raw_ptau(power, tau, alpha, beta))
    t0 = time.time()
    assert ctx.ptau_prepare_phase2(tmp_path / "raw.ptau", tmp_path / "out.ptau") == (power, power, 0, 0)
    print("power %d: prepare phase2 %.2f s (library call, wall)" % (power, time.time() - t0))
    assert ctx.ptau_verify(tmp_path / "out.ptau") == (0, (power, power, 1, 0))
    secs = dict(_sections((tmp_path / "out.ptau").read_bytes()))
    for t in (12, 13, 14, 15):
        group, unit = (2, 128) if t == 13 else (1, 64)
        top = power + 1 if t == 12 else power
        samples = [(0, 0), (top, (1 << top) - 1)]
        for lvl in (1, 2, 5, 9, 11, top - 1, top):
            samples += [(lvl, rng.randrange(1 << lvl)) for _ in range(6 if lvl == top else 5 if lvl >= 9 else 3)]
        assert len(samples) == 32 and len({lvl for lvl, _ in samples}) >= 4
        want = _fb(group, [_level_scalars(power, tau, alpha, beta, t, lvl)[j] for lvl, j in samples])
        for i, (lvl, j) in enumerate(samples):
            at = unit * ((1 << lvl) - 1 + j)
            assert secs[t][at:at + unit] == want[unit * i:unit * (i + 1)], (t, lvl, j)


def test_bad_inputs(ctx, zk, tmp_path):
    rng = random.Random(66)
    power = 2
    N = 1 << power
    good = _raw_ptau(power, rng.randrange(2, R), rng.randrange(2, R), rng.randrange(2, R))
    s = _offsets(good)
    secs = dict(_sections(good))
    hdr = secs[1]
    at4 = s[4][0] + 64 * 2
    y = bn.from_mont(int.from_bytes(good[at4 + 32:at4 + 64], "little"), Q)
    outside = _twist_points_outside_g2(rng, 1)[0]
    cases = {
        "no3.ptau": (_rebuild(good, drop=(3,)), "section 3 missing"),
        "short2.ptau": (_rebuild(good, {2: secs[2][:-64]}), "section 2 has the wrong length"),
        "coord.ptau": (_patch(good, s[2][0] + 64 * 3, le(Q)), "section 2: a coordinate is not a field element"),
        "offcurve.ptau": (_patch(good, at4 + 32, le(bn.to_mont((y + 1) % Q, Q))), "section 4: a point is not on the curve"),
        "subgroup.ptau": (_patch(good, s[3][0] + 128 * (N // 2), g16.g2_to_bytes(outside)), "section 3: a point is outside G2"),
        "truncated.ptau": (good[:len(good) - 100], "past the end"),
        "power28.ptau": (_rebuild(good, {1: hdr[:36] + struct.pack("<II", 28, 28)}), "power above 27"),
    }
    out = tmp_path / "out.ptau"
    for name, (data, msg) in cases.items():
        (tmp_path / name).write_bytes(data)
        with pytest.raises(zk.ZkpoaError, match=msg):
            ctx.ptau_prepare_phase2(tmp_path / name, out)
        assert not out.exists(), name
        rc = _cli(zk, tmp_path, name, "out.ptau")
        assert rc.returncode == 1 and "zkpoa-setup:" in rc.stderr and msg in rc.stderr, (name, rc.stderr)
        assert not out.exists() and "Prepared" not in rc.stdout, name
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(cases)          # no temporary file is left either
    # a file already at the output path keeps its bytes
    out.write_bytes(b"keep me")
    with pytest.raises(zk.ZkpoaError, match="not on the curve"):
        ctx.ptau_prepare_phase2(tmp_path / "offcurve.ptau", out)
    assert _cli(zk, tmp_path, "offcurve.ptau", "out.ptau").returncode == 1
    assert out.read_bytes() == b"keep me"
    out.unlink()
    # the output must not be the input
    (tmp_path / "good.ptau").write_bytes(good)
    with pytest.raises(zk.ZkpoaError, match="names the input file"):
        ctx.ptau_prepare_phase2(tmp_path / "good.ptau", tmp_path / "good.ptau")
    rc = _cli(zk, tmp_path, "good.ptau", "./good.ptau")
    assert rc.returncode == 1 and "names the input file" in rc.stderr
    assert (tmp_path / "good.ptau").read_bytes() == good
    # wrong argument counts
    for args in (["good.ptau"], ["good.ptau", "a.ptau", "b.ptau"]):
        rc = _cli(zk, tmp_path, *args)
        assert rc.returncode == 2 and "usage" in rc.stderr and "powersoftau prepare phase2 <in.ptau> <out.ptau>" in rc.stderr
    # the context is still usable
    assert ctx.ptau_prepare_phase2(tmp_path / "good.ptau", out) == (power, power, 0, 0)
    assert ctx.ptau_verify(out) == (0, (power, power, 1, 0))
