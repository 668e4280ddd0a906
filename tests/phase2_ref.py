"""Big-integer restatement of DESIGN.md "Phase-2 transcript" (test infrastructure): the hash form of a point, the circuit
hash, the ChaCha generator, `fromRng`, hash-to-G2, the beacon and the records of a .zkey's section 10. Written from that
section, not from csrc/phase2.hpp. hashlib supplies Blake2b-512 and SHA-256, oracle/py/bn254.py the curve arithmetic;
the generator, the square roots, `fromRng` and the record builder are this file's own."""
import hashlib
import struct

from oracle.py import bn254 as bn
from oracle.py import groth16 as g16

Q, R = bn.Q, bn.R
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
G2_COFACTOR = 2 * Q - R
MONT_INV_Q = pow(1 << 256, -1, Q)
MONT_INV_R = pow(1 << 256, -1, R)
MAX_BEACON_EXP = 30


# ---- hash form -------------------------------------------------------------------------------------------------------
def hash_u32(v):
    return struct.pack(">I", v)


def hash_g1(P):
    if P is None:
        return b"\x40" + bytes(63)
    return P[0].to_bytes(32, "big") + P[1].to_bytes(32, "big")


def hash_g2(P):
    if P is None:
        return b"\x40" + bytes(127)
    (x0, x1), (y0, y1) = P
    return b"".join(v.to_bytes(32, "big") for v in (x1, x0, y1, y0))          # an Fq2 coordinate: c1 then c0


# ---- ChaCha20 generator: key words 4-11, 64-bit block counter in words 12-13, zero nonce -----------------------------------
def _rotl(x, n):
    return ((x << n) | (x >> (32 - n))) & M32


def chacha_block(key, counter):
    st = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574] + list(key) + [counter & M32, counter >> 32, 0, 0]
    w = list(st)

    def quarter(a, b, c, d):
        w[a] = (w[a] + w[b]) & M32; w[d] = _rotl(w[d] ^ w[a], 16)
        w[c] = (w[c] + w[d]) & M32; w[b] = _rotl(w[b] ^ w[c], 12)
        w[a] = (w[a] + w[b]) & M32; w[d] = _rotl(w[d] ^ w[a], 8)
        w[c] = (w[c] + w[d]) & M32; w[b] = _rotl(w[b] ^ w[c], 7)
    for _ in range(10):
        quarter(0, 4, 8, 12); quarter(1, 5, 9, 13); quarter(2, 6, 10, 14); quarter(3, 7, 11, 15)
        quarter(0, 5, 10, 15); quarter(1, 6, 11, 12); quarter(2, 7, 8, 13); quarter(3, 4, 9, 14)
    return [(a + b) & M32 for a, b in zip(w, st)]


class ChaCha:
    def __init__(self, key):
        assert len(key) == 8
        self.key, self.counter, self.words = list(key), 0, []

    def next_u32(self):
        if not self.words:
            self.words = chacha_block(self.key, self.counter)
            self.counter += 1
        return self.words.pop(0)

    def next_u64(self):
        hi = self.next_u32()
        return hi << 32 | self.next_u32()

    def next_bool(self):
        return self.next_u32() & 1 == 1


def key_of(b32):
    return list(struct.unpack(">8I", bytes(b32[:32])))


# ---- square roots ----------------------------------------------------------------------------------------------------
def fq_sqrt(a):
    r = pow(a, (Q + 1) // 4, Q)
    return r if r * r % Q == a % Q else None


def fq2_sqrt(a):
    a0, a1 = a[0] % Q, a[1] % Q
    if a1 == 0:
        r = fq_sqrt(a0)
        if r is not None:
            return (r, 0)
        r = fq_sqrt(-a0 % Q)
        return None if r is None else (0, r)
    d = fq_sqrt((a0 * a0 + a1 * a1) % Q)
    if d is None:
        return None
    inv2 = pow(2, -1, Q)
    for t in ((a0 + d) * inv2 % Q, (a0 - d) * inv2 % Q):
        c0 = fq_sqrt(t)
        if c0:
            c1 = a1 * pow(2 * c0, -1, Q) % Q
            if bn.FQ2.eq(bn.FQ2.sqr((c0, c1)), (a0, a1)):
                return (c0, c1)
    return None


def fq_negative(a):
    return a % Q > (Q - 1) // 2


def fq2_negative(a):
    return fq_negative(a[0]) if a[1] % Q == 0 else fq_negative(a[1])


# ---- fromRng ---------------------------------------------------------------------------------------------------------
def _field_from_rng(rng, p, mont_inv):
    """Four 64-bit draws, least significant first, masked to 254 bits, redrawn while >= p; the accepted integer is the
    element's Montgomery representation."""
    while True:
        v = 0
        for i in range(4):
            v |= rng.next_u64() << (64 * i)
        v &= (1 << 254) - 1
        if v < p:
            return v * mont_inv % p


def fq_from_rng(rng):
    return _field_from_rng(rng, Q, MONT_INV_Q)


def fr_from_rng(rng):
    return _field_from_rng(rng, R, MONT_INV_R)


def g1_from_rng(rng):
    while True:
        x = fq_from_rng(rng)
        greatest = rng.next_bool()
        y = fq_sqrt((x * x * x + 3) % Q)
        if y is None:
            continue
        if greatest != fq_negative(y):
            y = -y % Q
        return (x, y)


def g2_from_rng(rng):
    F = bn.FQ2
    while True:
        c0 = fq_from_rng(rng)
        x = (c0, fq_from_rng(rng))
        greatest = rng.next_bool()
        y = fq2_sqrt(F.add(F.mul(F.sqr(x), x), bn.B2))
        if y is None:
            continue
        if greatest != fq2_negative(y):
            y = F.neg(y)
        return bn.ec_mul((x, y), G2_COFACTOR, F, order=1 << 300)


def hash_to_g2(h64):
    return g2_from_rng(ChaCha(key_of(h64)))


def beacon_key(beacon, exp):
    assert exp <= MAX_BEACON_EXP
    cur = bytes(beacon)
    for _ in range(1 << exp):
        cur = hashlib.sha256(cur).digest()
    return key_of(cur)


def beacon_secrets(beacon, exp):
    """(d, g1_s) of a beacon: both from one generator, d first."""
    rng = ChaCha(beacon_key(beacon, exp))
    d = fr_from_rng(rng)
    return d, g1_from_rng(rng)


# ---- circuit hash ----------------------------------------------------------------------------------------------------
def circuit_hash(zkey0, ptau):
    """zkey0: the bytes of an INITIAL key (delta = 1; sections 3, 5-8 are the initial points); ptau: the ceremony file."""
    zk = g16.read_zkey(zkey0)
    n = zk.domainSize
    ps = {t: lst[0] for t, lst in g16.read_binfile(ptau, "ptau", 1).items()}
    tau = [g16.g1_from_bytes(ptau, ps[2][0] + 64 * i) for i in range(2 * n - 1)]
    h = hashlib.blake2b(digest_size=64)
    h.update(hash_g1(zk.alpha1) + hash_g1(zk.beta1) + hash_g2(zk.beta2) + hash_g2(bn.G2_GEN) + hash_g1(bn.G1_GEN) +
             hash_g2(bn.G2_GEN))
    h.update(hash_u32(zk.nPublic + 1) + b"".join(hash_g1(P) for P in zk.IC))
    h.update(hash_u32(n - 1))
    for i in range(n - 1):
        h.update(hash_g1(bn.g1_add(tau[i + n], bn.ec_neg(tau[i], bn.FQ))))
    for pts, hp in ((zk.C, hash_g1), (zk.A, hash_g1), (zk.B1, hash_g1), (zk.B2, hash_g2)):
        h.update(hash_u32(len(pts)) + b"".join(hp(P) for P in pts))
    return h.digest()


# ---- records ---------------------------------------------------------------------------------------------------------
class Record:
    def __init__(self, delta_after, g1_s, g1_sx, g2_spx, transcript, type_, name=b"", exp=0, beacon=b""):
        self.delta_after, self.g1_s, self.g1_sx, self.g2_spx = delta_after, g1_s, g1_sx, g2_spx
        self.transcript, self.type, self.name, self.exp, self.beacon = transcript, type_, name, exp, beacon

    def pubkey_hash_bytes(self):
        return hash_g1(self.delta_after) + hash_g1(self.g1_s) + hash_g1(self.g1_sx) + hash_g2(self.g2_spx) + \
            self.transcript

    def to_bytes(self):
        params = b""
        if self.name:
            params += bytes([1, len(self.name)]) + self.name
        if self.type == 1:
            params += bytes([2, self.exp]) + bytes([3, len(self.beacon)]) + self.beacon
        return (g16.g1_to_bytes(self.delta_after) + g16.g1_to_bytes(self.g1_s) + g16.g1_to_bytes(self.g1_sx) +
                g16.g2_to_bytes(self.g2_spx) + self.transcript + struct.pack("<II", self.type, len(params)) + params)


def next_record(cs_hash, records, delta_before, d, g1_s, type_=0, name=b"", exp=0, beacon=b""):
    """The record a contribution of secret d adds after `records` (delta_before: delta1 before it)."""
    g1_sx = bn.g1_mul(g1_s, d)
    h = hashlib.blake2b(digest_size=64)
    h.update(cs_hash)
    for r in records:
        h.update(r.pubkey_hash_bytes())
    h.update(hash_g1(g1_s) + hash_g1(g1_sx))
    th = h.digest()
    g2_spx = bn.g2_mul(hash_to_g2(th), d)
    return Record(bn.g1_mul(delta_before, d), g1_s, g1_sx, g2_spx, th, type_, name, exp, beacon)


def section10(cs_hash, records):
    return cs_hash + struct.pack("<I", len(records)) + b"".join(r.to_bytes() for r in records)
