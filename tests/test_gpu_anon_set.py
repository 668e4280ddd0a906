"""The stable device index of the anonymity set's addresses (zkpoa_anon_set_index_device) and the duplicate check over it
(zkpoa_anon_set_audit), against Python's own stable sort: sorted(range(n), key=lambda i: (a[i], i)). The expected output
is unique because the order is stable, so every comparison is for equality. Sizes sit around the wave (64), the tile
(2048) and several tiles; key patterns are the ones chosen to hurt a radix sort: all equal, two values, keys that share 31
of their 32 bytes, and sorted input in both directions."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
SIZES = [1, 2, 63, 64, 65, 2047, 2048, 2049, 2 * 2048 + 3, 70001]       # 70001: 35 tiles
BASE = int.from_bytes(bytes(range(1, 32)) + b"\x11", "little")          # no zero byte, below r


def with_byte(pos, value):
    return BASE & ~(0xff << (8 * pos)) | (value << (8 * pos))


def distinct_keys(n, rng):
    keys = set()
    while len(keys) < n:
        keys.add(rng.getrandbits(160))
    out = list(keys)
    rng.shuffle(out)
    return out


def patterns(n, rng):
    """name -> n keys"""
    distinct = sorted(distinct_keys(n, rng))
    two = (rng.getrandbits(160), rng.getrandbits(160))
    return {
        "random 160-bit": distinct_keys(n, rng),
        "random below r": [rng.randrange(R) for _ in range(n)],                      # no pass is skipped
        "all equal": [BASE] * n,
        "two values": [two[rng.getrandbits(1)] for _ in range(n)],
        "byte 0 only": [with_byte(0, rng.getrandbits(8)) for _ in range(n)],
        "byte 19 only": [with_byte(19, rng.getrandbits(8)) for _ in range(n)],
        "byte 31 only": [with_byte(31, rng.randrange(0x30)) for _ in range(n)],
        "ascending": distinct,
        "descending": distinct[::-1],
        "many repeats over two bytes": [rng.getrandbits(11) << 4 for _ in range(n)],  # a later pass must keep the earlier order
    }


def key_bytes(keys):
    return b"".join(k.to_bytes(32, "little") for k in keys)


def model_index(a):
    return sorted(range(len(a)), key=lambda i: (a[i], i))


def model_audit(a):
    """(rows equal to an earlier row, the pair with the smallest later row, strictly ascending) of zkpoa_anon_set_audit"""
    seen, dups, pair = {}, 0, None
    for j, k in enumerate(a):
        if k in seen:
            dups += 1
            if pair is None:
                pair = (seen[k], j)
        else:
            seen[k] = j
    return dups, pair, all(x < y for x, y in zip(a, a[1:]))


def device_index(ctx, keys):
    import torch
    n = len(keys)
    d_keys = torch.from_numpy(np.frombuffer(key_bytes(keys), dtype=np.uint8).copy()).cuda()
    d_perm = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.anon_set_index(d_keys.data_ptr(), n, d_perm.data_ptr())
    return [int(v) & 0xffffffff for v in d_perm.cpu().numpy()[:n]]


@pytest.mark.parametrize("n", SIZES)
def test_index_is_the_stable_sort(ctx, n):
    rng = random.Random(1000 + n)
    for name, keys in patterns(n, rng).items():
        assert device_index(ctx, keys) == model_index(keys), (name, n)
    assert ctx.last_ms(9) > 0


def test_index_of_nothing_is_a_no_op(ctx):
    ctx.anon_set_index(0, 0, 0)
    assert ctx.last_ms(9) == 0


@pytest.mark.parametrize("n", SIZES)
def test_audit_of_every_pattern(ctx, n):
    rng = random.Random(2000 + n)
    for name, keys in patterns(n, rng).items():
        assert ctx.anon_set_audit(key_bytes(keys)) == model_audit(keys), (name, n)


def test_audit_duplicates(ctx):
    rng = random.Random(7)
    n = 2 * 2048 + 3
    clean = distinct_keys(n, rng)
    assert ctx.anon_set_audit(key_bytes(clean)) == (0, None, False) == model_audit(clean)
    asc = sorted(clean)
    assert ctx.anon_set_audit(key_bytes(asc)) == (0, None, True)
    adjacent = list(clean)
    adjacent[1001] = adjacent[1000]
    assert ctx.anon_set_audit(key_bytes(adjacent)) == (1, (1000, 1001), False) == model_audit(adjacent)
    adjacent_sorted = list(asc)                       # equal neighbours in an otherwise ascending file: not strictly ascending
    adjacent_sorted[1001] = adjacent_sorted[1000]
    assert ctx.anon_set_audit(key_bytes(adjacent_sorted)) == (1, (1000, 1001), False)
    far = list(clean)
    far[4090] = far[5]                                # first and third tile
    assert ctx.anon_set_audit(key_bytes(far)) == (1, (5, 4090), False) == model_audit(far)
    triple = list(clean)
    triple[3000] = triple[2100] = triple[40]
    assert ctx.anon_set_audit(key_bytes(triple)) == (2, (40, 2100), False) == model_audit(triple)
    both = list(triple)                               # a later group whose second member comes first in the file
    both[2050] = both[2049]
    assert ctx.anon_set_audit(key_bytes(both)) == (3, (2049, 2050), False) == model_audit(both)
    assert ctx.anon_set_audit(b"") == (0, None, True) == model_audit([])
