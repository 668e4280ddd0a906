"""The phase-1 transcript without a GPU (DESIGN.md "Phase-1 transcript"): tests/phase1_ref.py against independent
expectations, and the host side of csrc/phase1.hpp through the C ABI -- the saved Blake2b state of a record's
partialHash, the compressed form of a point, the record layout, and zkpoa_ptau_contributions on hand-built section 7
images, every malformed kind included."""
import hashlib
import random
import struct

import pytest

import phase1_ref as p1
import phase2_ref as p2
from oracle.py import bn254 as bn
from oracle.py import groth16 as g16

Q, R = bn.Q, bn.R
LENGTHS = [0, 1, 127, 128, 129, 1000]


def _data(rng, n):
    return rng.getrandbits(8 * n).to_bytes(n, "little") if n else b""


@pytest.mark.parametrize("n", LENGTHS + [256, 257])
def test_reference_blake2b_matches_hashlib(n):
    d = _data(random.Random(n), n)
    assert p1.Blake2b().update(d).digest() == hashlib.blake2b(d, digest_size=64).digest()
    assert p1.Blake2b().update(d[:n // 3]).update(d[n // 3:]).digest() == hashlib.blake2b(d, digest_size=64).digest()


@pytest.mark.parametrize("n1", LENGTHS)
@pytest.mark.parametrize("n2", LENGTHS)
def test_blake2b_partial_state_round_trip(zk, n1, n2):
    """The state after m1, restored, then m2, gives the digest of m1 | m2: in the reference, through the C ABI, and
    across the two (the 216 bytes are the same bytes)."""
    rng = random.Random(1000 * n1 + n2)
    m1, m2 = _data(rng, n1), _data(rng, n2)
    want = hashlib.blake2b(m1 + m2, digest_size=64).digest()
    st = p1.Blake2b().update(m1).state()
    assert len(st) == 216
    assert p1.Blake2b.from_state(st).update(m2).digest() == want
    assert zk.blake2b_state(m1) == st
    assert zk.blake2b_resume(st, m2) == want


def test_blake2b_state_layout(zk):
    """h[8], t[2], buffer, fill: a full buffer stays in the state (the last block is compressed by final alone), and the
    buffer is zero past its fill."""
    st = zk.blake2b_state(b"")
    h0 = list(p1._IV)
    h0[0] ^= 0x01010040
    assert st == struct.pack("<8Q", *h0) + bytes(16 + 128 + 8)
    d = bytes(range(128))
    st = zk.blake2b_state(d)
    assert st[:64] == struct.pack("<8Q", *h0) and st[64:80] == bytes(16) and st[80:208] == d and st[208:] == struct.pack("<Q", 128)
    st = zk.blake2b_state(d + b"\xaa")
    assert st[64:80] == struct.pack("<2Q", 128, 0) and st[80:208] == b"\xaa" + bytes(127) and st[208:] == struct.pack("<Q", 1)
    with pytest.raises(zk.ZkpoaError):
        zk.blake2b_resume(st[:208] + struct.pack("<Q", 129), b"")


def test_compressed_form_of_known_points():
    G1, G2 = bn.G1_GEN, bn.G2_GEN
    assert G1 == (1, 2)
    assert p1.compress_g1(G1) == bytes(31) + b"\x01"                                  # y = 2 is the positive root
    assert p1.compress_g1(bn.ec_neg(G1, bn.FQ)) == b"\x80" + bytes(30) + b"\x01"      # y = q - 2 is the negative one
    assert p1.compress_g1(None) == b"\x40" + bytes(31)
    (x0, x1), (y0, y1) = G2
    c = p1.compress_g2(G2)
    assert len(c) == 64 and c[32:] == x0.to_bytes(32, "big")
    assert c[1:32] == x1.to_bytes(32, "big")[1:] and c[0] & 0x3f == x1 >> 248
    assert (c[0] & 0x80 != 0) == (y1 > (Q - 1) // 2)
    cn = p1.compress_g2(bn.ec_neg(G2, bn.FQ2))
    assert cn[1:] == c[1:] and cn[0] ^ c[0] == 0x80
    assert p1.compress_g2(None) == b"\x40" + bytes(63)
    # a G2 point whose y has c1 = 0: the sign is that of c0 (the compressed form reads the coordinates it is given)
    for y0v in (5, Q - 5):
        P = ((7, 9), (y0v, 0))
        c = p1.compress_g2(P)
        assert c == bytes([0x80 if y0v > (Q - 1) // 2 else 0]) + (9).to_bytes(32, "big")[1:] + (7).to_bytes(32, "big")
    assert p1.compress_g2(((7, 9), (Q - 5, 1)))[0] == 0          # c1 = 1 is positive whatever c0
    assert p1.compress_g2(((7, 9), (5, Q - 1)))[0] == 0x80


def _record(seed, type_=0, name=b"", exp=0, beacon=b""):
    rng = random.Random(seed)
    g1 = lambda: bn.g1_mul(bn.G1_GEN, rng.randrange(1, R))
    g2 = lambda: bn.g2_mul(bn.G2_GEN, rng.randrange(1, R))
    h = p1.Blake2b().update(_data(rng, 300))
    return p1.Record((g1(), g2(), g1(), g1(), g2()), [g1() for _ in range(6)], [g2() for _ in range(3)], h.state(),
                     _data(rng, 64), type_, name, exp, beacon)


def test_record_round_trip():
    for r in (_record(1), _record(2, 0, b"alice"), _record(3, 1, b"", 4, b"\x01\x02"), _record(4, 1, b"bob", 10, bytes(255))):
        b = r.to_bytes()
        assert len(b) == p1.RECORD_FIXED + len(p1.params(r.type, r.name, r.exp, r.beacon))
        back, used = p1.parse_record(b)
        assert used == len(b) and back.to_bytes() == b
        assert (back.type, back.name, back.exp, back.beacon) == (r.type, r.name, r.exp, r.beacon)
        assert back.points == r.points and back.key_g1 == r.key_g1 and back.key_g2 == r.key_g2
        assert back.response_hash() == r.response_hash()
    assert p1.RECORD_FIXED == 1504


def _ptau_with_section7(s7):
    hdr = struct.pack("<I", 32) + Q.to_bytes(32, "little") + struct.pack("<II", 1, 1)
    return g16.write_binfile("ptau", 1, [(1, hdr), (7, s7)])


def test_ptau_contributions_on_hand_built_sections(zk, tmp_path):
    recs = [_record(11, 0, b"first"), _record(12, 1, b"", 3, b"\xbe\xac"), _record(13)]
    path = tmp_path / "t.ptau"
    path.write_bytes(_ptau_with_section7(p1.section7(recs)))
    count, lines = zk.ptau_contributions(str(path))
    assert count == 3
    assert lines == ["contribution first " + recs[0].response_hash().hex(), "beacon  " + recs[1].response_hash().hex(),
                     "contribution  " + recs[2].response_hash().hex()]
    path.write_bytes(_ptau_with_section7(p1.section7([])))
    assert zk.ptau_contributions(str(path)) == (0, [])
    good = p1.section7(recs[:2])
    one = p1.section7(recs[:1])
    tag_at = 4 + p1.RECORD_FIXED                                   # the first tag byte of record 0's params
    type_at = 4 + p1.RECORD_FIXED - 8
    bad = {
        "ends inside a record": good[:-1],
        "ends inside the fixed part": good[:4 + 700],
        "count above the records": struct.pack("<I", 3) + good[4:],
        "left-over bytes": good + b"\0",
        "left-over record": struct.pack("<I", 1) + good[4:],
        "unknown tag": one[:tag_at] + b"\x07" + one[tag_at + 1:],
        "type above 1": one[:type_at] + struct.pack("<I", 2) + one[type_at + 4:],
        "name runs past the params": one[:tag_at + 1] + b"\xff" + one[tag_at + 2:],
        "shorter than a count": b"\0\0",
    }
    for name, s7 in bad.items():
        path.write_bytes(_ptau_with_section7(s7))
        with pytest.raises(zk.ZkpoaError):
            zk.ptau_contributions(str(path))
            raise AssertionError(name + " was accepted")
    with pytest.raises(zk.ZkpoaError):
        zk.ptau_contributions(str(tmp_path / "missing.ptau"))


def test_fresh_challenge_and_key_are_deterministic():
    """The challenge of a fresh file depends on the power alone; g2_sp depends on the personalisation byte."""
    c1, c2 = p1.fresh_challenge(1), p1.fresh_challenge(2)
    assert len(c1) == 64 and c1 != c2 and c1 == p1.fresh_challenge(1)
    n = 2
    want = hashlib.blake2b(digest_size=64)
    want.update(hashlib.blake2b(b"", digest_size=64).digest())
    want.update(p2.hash_g1(bn.G1_GEN) * (2 * n - 1) + p2.hash_g2(bn.G2_GEN) * n + p2.hash_g1(bn.G1_GEN) * (2 * n) +
                p2.hash_g2(bn.G2_GEN))
    assert c1 == want.digest()
    s = bn.g1_mul(bn.G1_GEN, 5)
    sx = bn.g1_mul(s, 7)
    assert p1.g2_sp(0, c1, s, sx) != p1.g2_sp(1, c1, s, sx)
    assert bn.g2_mul(p1.g2_sp(2, c1, s, sx), R) is None           # in G2
