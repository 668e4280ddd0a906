"""The host primitives of the phase-2 transcript (csrc/phase2.hpp through the host-only C entry points) against
independent implementations: Blake2b-512 and SHA-256 against hashlib, the ChaCha generator, the square roots, `fromRng`,
hash-to-G2 and the beacon derivation against tests/phase2_ref.py (and the ChaCha20 block against the `cryptography`
package where it is installed). No GPU."""
import hashlib
import random
import struct

import pytest

import phase2_ref as ref
from oracle.py import bn254 as bn
from oracle.py import groth16 as g16

Q, R = bn.Q, bn.R


def _data(rng, n):
    return rng.getrandbits(8 * n).to_bytes(n, "little") if n else b""


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 3 << 20, (5 << 20) + 77])
def test_blake2b_and_sha256_match_hashlib(zk, n):
    d = _data(random.Random(n), n)
    assert zk.blake2b512(d) == hashlib.blake2b(d, digest_size=64).digest()
    assert zk.sha256(d) == hashlib.sha256(d).digest()


def test_blake2b_streaming_with_ragged_splits(zk):
    rng = random.Random(5)
    d = _data(rng, (2 << 20) + 131)
    want = hashlib.blake2b(d, digest_size=64).digest()
    for cuts in ([0, 0, 1, 127, 128, 129, 256, 1 << 20], [128] * 9, [127, 1, 128, 1, 127, 129], [1] * 300, []):
        pieces, at = [], 0
        for c in cuts:
            pieces.append(d[at:at + c])
            at += c
        pieces.append(d[at:])
        assert zk.blake2b512_stream(pieces) == want, cuts
    # a stream that ends exactly on a block boundary, and an empty one
    assert zk.blake2b512_stream([d[:128], d[128:256]]) == hashlib.blake2b(d[:256], digest_size=64).digest()
    assert zk.blake2b512_stream([]) == hashlib.blake2b(b"", digest_size=64).digest()


def test_chacha_generator_matches_the_reference(zk):
    rng = random.Random(9)
    for _ in range(6):
        key = [rng.getrandbits(32) for _ in range(8)]
        a, b = zk.ChaCha(key), ref.ChaCha(key)
        for i in range(200):                       # crosses block boundaries with every kind of draw
            kind = rng.randrange(3)
            if kind == 0:
                assert a.next_u32() == b.next_u32()
            elif kind == 1:
                assert a.next_u64() == b.next_u64()
            else:
                assert a.next_bool() == b.next_bool()
    # next_u64 is the high word first
    key = list(range(8))
    a, b = zk.ChaCha(key), zk.ChaCha(key)
    hi, lo = b.next_u32(), b.next_u32()
    assert a.next_u64() == hi << 32 | lo


def test_chacha_block_against_cryptography():
    """The reference generator's block function is ChaCha20 with a 64-bit counter and a zero nonce: pinned against the
    `cryptography` package, whose 16-byte nonce sets the state words 12-15."""
    cryptography = pytest.importorskip("cryptography")
    from cryptography.hazmat.primitives.ciphers import Cipher, algorithms
    rng = random.Random(3)
    for counter in (0, 1, 2, (1 << 32) - 1, 1 << 32):
        key = [rng.getrandbits(32) for _ in range(8)]
        nonce = struct.pack("<QQ", counter, 0)
        enc = Cipher(algorithms.ChaCha20(struct.pack("<8I", *key), nonce), mode=None).encryptor()
        assert list(struct.unpack("<16I", enc.update(bytes(64)))) == ref.chacha_block(key, counter)


def test_chacha_zero_key_block_is_the_published_keystream():
    """The first keystream bytes of ChaCha20 under the zero key, counter and nonce (the widely published test vector),
    independent of any installed package."""
    first = ref.chacha_block([0] * 8, 0)
    assert struct.pack("<4I", *first[:4]).hex() == "76b8e0ada0f13d90405d6ae55386bd28"


def test_square_roots(zk):
    rng = random.Random(11)
    seen_non_square = 0
    for a in [0, 1, 4, Q - 1, 3] + [rng.randrange(Q) for _ in range(200)]:
        got, want = zk.fq_sqrt(a), ref.fq_sqrt(a)
        assert (got is None) == (want is None)
        seen_non_square += got is None
        if got is not None:
            assert got * got % Q == a and got < Q
    assert seen_non_square > 50
    assert zk.fq_sqrt(Q) is None                   # not a field element
    cases = [(0, 0), (4, 0), (Q - 4, 0), (3, 0), (0, 5)] + [(rng.randrange(Q), rng.randrange(Q)) for _ in range(200)]
    cases += [bn.FQ2.sqr((rng.randrange(Q), rng.randrange(Q))) for _ in range(50)]
    n_sq = 0
    for a in cases:
        got, want = zk.fq2_sqrt(a), ref.fq2_sqrt(a)
        assert (got is None) == (want is None), a
        if got is not None:
            n_sq += 1
            assert bn.FQ2.eq(bn.FQ2.sqr(got), a)
    assert 100 < n_sq < len(cases)


def test_from_rng_matches_the_reference(zk):
    rng = random.Random(13)
    for i in range(200):
        key = [rng.getrandbits(32) for _ in range(8)]
        assert zk.fr_from_rng(key) == ref.fr_from_rng(ref.ChaCha(key))
        P = g16.g1_from_bytes(zk.g1_from_rng(key))
        assert P == ref.g1_from_rng(ref.ChaCha(key))
        assert bn.g1_is_on_curve(P) and bn.g1_mul(P, R - 1) == bn.ec_neg(P, bn.FQ)          # [r] P = O
    for i in range(100):
        key = [rng.getrandbits(32) for _ in range(8)]
        P = g16.g2_from_bytes(zk.g2_from_rng(key))
        assert P == ref.g2_from_rng(ref.ChaCha(key))
        assert bn.g2_is_on_curve(P)
        assert bn.ec_mul(P, R, bn.FQ2, order=R * R) is None                                 # in G2


def test_hash_to_g2_matches_the_reference(zk):
    rng = random.Random(17)
    for i in range(100):
        h = hashlib.blake2b(b"transcript %d" % i, digest_size=64).digest() if i else bytes(64)
        P = g16.g2_from_bytes(zk.hash_to_g2(h))
        assert P == ref.hash_to_g2(h)
        assert bn.g2_is_on_curve(P) and bn.ec_mul(P, R, bn.FQ2, order=R * R) is None
    # only the first 32 bytes key the generator, as big-endian words
    h = bytes(range(64))
    assert zk.hash_to_g2(h) == zk.hash_to_g2(h[:32] + bytes(32))
    assert zk.hash_to_g2(h) == zk.g2_from_rng(list(struct.unpack(">8I", h[:32])))


@pytest.mark.parametrize("exp", [0, 1, 10])
def test_beacon_derivation(zk, exp):
    for beacon in (bytes.fromhex("0102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f"), b"\x00", b"z" * 255):
        key = zk.beacon_key(beacon, exp)
        cur = beacon
        for _ in range(1 << exp):
            cur = hashlib.sha256(cur).digest()
        assert key == list(struct.unpack(">8I", cur)) == ref.beacon_key(beacon, exp)
        d, s = ref.beacon_secrets(beacon, exp)
        assert zk.fr_from_rng(key) == d


def test_beacon_exponent_is_capped(zk):
    with pytest.raises(zk.ZkpoaError):
        zk.beacon_key(b"\x01", 31)


def test_transcript_symbols_and_check_bits(zk):
    assert zk.ZKEY_CHECKS["CSHASH"] == 0x100 and zk.ZKEY_CHECKS["CONTRIBUTIONS"] == 0x200
    for name in ("zkpoa_zkey_new_ex", "zkpoa_zkey_contribute_ex", "zkpoa_zkey_beacon", "zkpoa_hash_form", "zkpoa_h_diff"):
        assert hasattr(zk.lib(), name)
