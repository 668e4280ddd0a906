"""The secp256k1 layer function by function on the device (zkpoa_secp_prim, include/zkpoa_secp_prim.h): Fp, Sc, the signed
recoding, to_affine, fixed_mul and double_mul of csrc/secp256k1.hip.h at the operand sets of tests/secp_limb_ref.py, which
reach every arm of every correction (tests/test_secp_limb_ref.py proves that on the CPU), against % on big integers and
the affine arithmetic of tests/secp_ref.py. Every comparison is exact. One launch per op."""
import pytest

import secp_limb_ref as lr
import secp_ref as sr
import sign_ref as sg

pytestmark = pytest.mark.gpu

SETS = lr.prim_sets()


def run_op(ctx, name, operands):
    """operands: one tuple per record -> one tuple per record: the op's 8-word results, then its extra words"""
    op, n_in, n8, tail = lr.OPS[name]
    n = len(operands)
    data = b"".join(int(t[j]).to_bytes(32, "little") for j in range(n_in) for t in operands)
    out = ctx.secp_prim(op, data, n, 8 * n8 + tail)
    assert len(out) == 4 * n * (8 * n8 + tail)
    res = []
    for i in range(n):
        vals = [int.from_bytes(out[32 * (j * n + i):32 * (j * n + i) + 32], "little") for j in range(n8)]
        at = 32 * n * n8 + 4 * tail * i
        res.append(tuple(vals + [int.from_bytes(out[at + 4 * k:at + 4 * k + 4], "little") for k in range(tail)]))
    return res


@pytest.mark.parametrize("name", list(SETS))
def test_field_and_scalar_ops(ctx, name):
    cases = SETS[name]
    got = run_op(ctx, name, [c[0] for c in cases])
    if name == "recode_signed4":
        got = [lr.recode_canonical(*g) for g in got]
    bad = [(name, [hex(v) for v in c[0]]) for c, g in zip(cases, got) if g != tuple(c[1])]
    assert bad[:10] == []


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_partial_last_wave(ctx, n):
    """Fp products, the ones that take a correction arm first: whole waves, a partial last wave, a batch of one lane"""
    cases = [c for c in SETS["fp_mul"] if lr.fp_mul(*c[0])[1]["outcome"] != "none"] + SETS["fp_mul"]
    cases = cases[:n]
    assert run_op(ctx, "fp_mul", [c[0] for c in cases]) == [tuple(c[1]) for c in cases]


def test_bad_op_and_empty_batch(zk, ctx):
    for op in (-1, 21, 99):
        for n in (0, 1):
            with pytest.raises(zk.ZkpoaError, match="secp_prim"):
                ctx.secp_prim(op, bytes(128), n, 8)
    for op in range(21):
        assert ctx.secp_prim(op, b"", 0, 33) == b""
    with pytest.raises(zk.ZkpoaError, match="secp_prim"):
        ctx.secp_prim(0, bytes(64), (1 << 16) + 1, 0)   # refused before anything is read


def to_affine(ctx, points):
    return run_op(ctx, "to_affine", points)


def test_fixed_mul(ctx):
    keys = sg.edge_keys()
    got = run_op(ctx, "fixed_mul", [(k,) for k in keys])
    want = [sr.mul(k, sr.G) for k in keys]
    assert [lr.affine_of(*g) for g in got] == want
    assert to_affine(ctx, got) == want


def test_double_mul(ctx):
    """u2 R + u1 G with both scalars at the recoding's borders and R among the entries of the shared G table: additions
    that double, cancel, pass through infinity or end there"""
    cases = lr.ladder_cases()
    got = run_op(ctx, "double_mul", [(pt[0], pt[1], u2, u1) for _, pt, u2, u1, _ in cases])
    bad = [c[0] for c, g in zip(cases, got) if lr.affine_of(*g[:4]) != c[4] or g[4] != int(c[4] is None)]
    assert bad[:10] == []
    finite = [(c, g) for c, g in zip(cases, got) if c[4] is not None]
    assert len(finite) >= 800 and len(cases) - len(finite) >= 20
    assert to_affine(ctx, [g[:4] for _, g in finite]) == [c[4] for c, _ in finite]
    by_name = {c[0]: g for c, g in zip(cases, got)}
    assert by_name["cancel 1"][4] == 1 and lr.affine_of(*by_name["through infinity"][:4]) == sr.G
