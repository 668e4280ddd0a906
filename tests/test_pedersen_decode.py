"""zkpoa_pedersen_decode (include/zkpoa_audit.h; host only, no GPU): the commitment a layer-three proof binds, read off its
first 12 public signals, against a big-integer restatement written here -- on both layer-three public.json files the
reference commits, and on signals that spell no point."""
import json
import os

import pytest

import layer_inputs_ref as ref
from conftest import GOLDEN

P = 2 ** 255 - 19
D = (-121665 * pow(121666, P - 2, P)) % P
CASES = ["1_sigs_1_batches_5_height", "4_sigs_2_batches_12_height"]


def signals_of(case):
    with open(os.path.join(GOLDEN, "ref", case + "__layer_three", "public.json")) as f:
        return [int(v) for v in json.load(f)]


def decode(signals):
    """-> the RFC 8032 encoding, or None where the issue's contract says "not valid"."""
    if any(s >> 85 for s in signals[:12]):
        return None
    X, Y, Z, T = [(signals[3 * i] + (signals[3 * i + 1] << 85) + (signals[3 * i + 2] << 170)) % P for i in range(4)]
    if Z == 0 or (Y * Y - X * X - Z * Z - D * T * T) % P or (X * Y - Z * T) % P:
        return None
    zi = pow(Z, P - 2, P)
    x, y = X * zi % P, Y * zi % P
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def compress(point):
    x, y, z, _ = point
    zi = pow(z, P - 2, P)
    return (y * zi % P | ((x * zi % P & 1) << 255)).to_bytes(32, "little")


def rechunk(coords):
    return [(c >> (85 * k)) & ((1 << 85) - 1) for c in coords for k in range(3)]


def test_restated_constant():
    assert D == ref.D and P == ref.P


@pytest.mark.parametrize("case", CASES)
def test_decode_of_the_committed_public_signals(zk, case):
    signals = signals_of(case)
    want = decode(signals)
    assert want is not None and zk.pedersen_decode(signals) == want
    # the affine point it encodes is on the curve: -x^2 + y^2 = 1 + d x^2 y^2
    y = int.from_bytes(want, "little") & (2 ** 255 - 1)
    X, _, Z, _ = ref.dechunk_to_point(signals[:12])
    x = X * pow(Z, P - 2, P) % P
    assert (y * y - x * x - 1 - D * x * x * y * y) % P == 0 and (x & 1) == want[31] >> 7


def test_decode_is_the_commitment_of_the_fixtures_balance_sum(zk):
    """1_sigs_1_batches_5_height: one batch, its balances sum to 354, blinding factor 2 (tests/test_gpu_layer_inputs.py)."""
    with open(os.path.join(GOLDEN, "layer_inputs", "1_sigs__layer_two_batch_0_input.json")) as f:
        total = sum(int(b) for b in json.load(f)["leaf_balances"])
    assert total == 354
    want = compress(ref.pedersen_commitment(total, 2))
    assert zk.pedersen_decode(signals_of(CASES[0])) == want == compress(zk.pedersen_commit(total, 2))
    assert zk.pedersen_decode(signals_of(CASES[0])) != compress(ref.pedersen_commitment(total + 1, 2))


def test_decode_does_not_depend_on_the_projective_representative(zk):
    """The same point scaled by another Z encodes to the same 32 bytes (that is what the inversion is for)."""
    signals = signals_of(CASES[1])
    X, Y, Z, T = ref.dechunk_to_point(signals[:12])
    k = 0x1234567890abcdef1234567890abcdef
    scaled = rechunk([X * k % P, Y * k % P, Z * k % P, T * k % P])
    assert decode(scaled) == decode(signals)
    assert zk.pedersen_decode(scaled) == zk.pedersen_decode(signals)
    # coordinates given as p + value (still three 85-bit chunks) are the same residues
    if X + P < 2 ** 255:
        assert zk.pedersen_decode(rechunk([X + P, Y, Z, T])) == decode(signals)


@pytest.mark.parametrize("case", CASES)
def test_signals_that_spell_no_point(zk, case):
    signals = signals_of(case)
    X, Y, Z, T = ref.dechunk_to_point(signals[:12])
    too_wide = list(signals)
    too_wide[4] = 2 ** 85
    bad_t = rechunk([X, Y, Z, (T + 1) % P])
    zero_z = rechunk([X, Y, 0, T])
    all_zero = [0] * 12
    off_curve = rechunk([X, (Y + 1) % P, Z, T])
    for name, bad in [("2^85", too_wide), ("T + 1", bad_t), ("Z = 0", zero_z), ("all zero", all_zero), ("Y + 1", off_curve)]:
        assert decode(bad) is None, name
        assert zk.pedersen_decode(bad) is None, name
    widest = list(signals)                                   # 2^85 - 1 fits: rejected for the curve, not for its width
    widest[4] = 2 ** 85 - 1
    assert zk.pedersen_decode(widest) == decode(widest)
    with pytest.raises(zk.ZkpoaError):
        zk.pedersen_decode(signals[:11])
