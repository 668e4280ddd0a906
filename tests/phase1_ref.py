"""Big-integer restatement of DESIGN.md "Phase-1 transcript" (test infrastructure): the compressed form of a point, the
saved Blake2b state, the contribution key, the challenge of a fresh file and the records of a .ptau's section 7. Written
from that section, not from csrc/phase1.hpp. The primitives it shares with the phase-2 transcript (hash form, ChaCha,
`fromRng`, hash-to-G2, the beacon key) come from tests/phase2_ref.py; Blake2b is restated here because hashlib cannot
export the state that a record's partialHash holds."""
import hashlib
import struct

import phase2_ref as p2
from oracle.py import bn254 as bn
from oracle.py import groth16 as g16

Q, R = bn.Q, bn.R
M64 = (1 << 64) - 1
STATE_LEN = 216
RECORD_FIXED = 448 + 768 + STATE_LEN + 64 + 8


# ---- Blake2b-512, unkeyed (RFC 7693), with the state of a partialHash --------------------------------------------------
_IV = [0x6a09e667f3bcc908, 0xbb67ae8584caa73b, 0x3c6ef372fe94f82b, 0xa54ff53a5f1d36f1,
       0x510e527fade682d1, 0x9b05688c2b3e6c1f, 0x1f83d9abfb41bd6b, 0x5be0cd19137e2179]
_SIGMA = [[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15], [14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3],
          [11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4], [7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8],
          [9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13], [2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9],
          [12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11], [13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10],
          [6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5], [10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0]]


def _rotr(x, n):
    return ((x >> n) | (x << (64 - n))) & M64


class Blake2b:
    """The last block is held back until final(): a full buffer is compressed only when more input arrives."""

    def __init__(self):
        self.h = list(_IV)
        self.h[0] ^= 0x01010040
        self.t = 0                                   # bytes compressed so far (128 bits: t[0] | t[1] << 64)
        self.buf = b""

    def _compress(self, block, last):
        m = struct.unpack("<16Q", block)
        v = self.h + list(_IV)
        v[12] ^= self.t & M64
        v[13] ^= self.t >> 64
        if last:
            v[14] ^= M64

        def g(a, b, c, d, x, y):
            v[a] = (v[a] + v[b] + x) & M64; v[d] = _rotr(v[d] ^ v[a], 32)
            v[c] = (v[c] + v[d]) & M64; v[b] = _rotr(v[b] ^ v[c], 24)
            v[a] = (v[a] + v[b] + y) & M64; v[d] = _rotr(v[d] ^ v[a], 16)
            v[c] = (v[c] + v[d]) & M64; v[b] = _rotr(v[b] ^ v[c], 63)
        for r in range(12):
            s = _SIGMA[r % 10]
            g(0, 4, 8, 12, m[s[0]], m[s[1]]); g(1, 5, 9, 13, m[s[2]], m[s[3]])
            g(2, 6, 10, 14, m[s[4]], m[s[5]]); g(3, 7, 11, 15, m[s[6]], m[s[7]])
            g(0, 5, 10, 15, m[s[8]], m[s[9]]); g(1, 6, 11, 12, m[s[10]], m[s[11]])
            g(2, 7, 8, 13, m[s[12]], m[s[13]]); g(3, 4, 9, 14, m[s[14]], m[s[15]])
        self.h = [self.h[i] ^ v[i] ^ v[i + 8] for i in range(8)]

    def update(self, data):
        data = self.buf + bytes(data)
        while len(data) > 128:
            self.t += 128
            self._compress(data[:128], False)
            data = data[128:]
        self.buf = data
        return self

    def state(self):
        """h[8], t[2], the 128-byte buffer (zero past its fill), the fill: little-endian u64."""
        return (struct.pack("<8Q", *self.h) + struct.pack("<2Q", self.t & M64, self.t >> 64) +
                self.buf.ljust(128, b"\0") + struct.pack("<Q", len(self.buf)))

    @classmethod
    def from_state(cls, st):
        assert len(st) == STATE_LEN
        b = cls()
        b.h = list(struct.unpack("<8Q", st[:64]))
        t0, t1 = struct.unpack("<2Q", st[64:80])
        b.t = t0 | t1 << 64
        fill = struct.unpack("<Q", st[208:])[0]
        assert fill <= 128
        b.buf = st[80:80 + fill]
        return b

    def digest(self):
        c = Blake2b()
        c.h, c.t = list(self.h), self.t + len(self.buf)
        c._compress(self.buf.ljust(128, b"\0"), True)
        return struct.pack("<8Q", *c.h)


def blake2b(data):
    return hashlib.blake2b(data, digest_size=64).digest()


# ---- compressed form -------------------------------------------------------------------------------------------------
def compress_g1(P):
    if P is None:
        return b"\x40" + bytes(31)
    b = bytearray(P[0].to_bytes(32, "big"))
    if p2.fq_negative(P[1]):
        b[0] |= 0x80
    return bytes(b)


def compress_g2(P):
    if P is None:
        return b"\x40" + bytes(63)
    (x0, x1), y = P
    b = bytearray(x1.to_bytes(32, "big") + x0.to_bytes(32, "big"))            # an Fq2 coordinate: c1 then c0
    if p2.fq2_negative(y):
        b[0] |= 0x80
    return bytes(b)


# ---- the sections of a ceremony file ---------------------------------------------------------------------------------
SECTION_GROUP = {2: 1, 3: 2, 4: 1, 5: 1, 6: 2}


def read_sections(ptau):
    """{2..6: [points]} of the bytes of a .ptau, and the bytes of its section 7."""
    ps = {t: lst[0] for t, lst in g16.read_binfile(ptau, "ptau", 1).items()}
    out = {}
    for t, grp in SECTION_GROUP.items():
        off, ln = ps[t]
        unit = 64 * grp
        rd = g16.g1_from_bytes if grp == 1 else g16.g2_from_bytes
        out[t] = [rd(ptau, off + unit * i) for i in range(ln // unit)]
    return out, ptau[ps[7][0]:ps[7][0] + ps[7][1]]


def hash_form(secs):
    return b"".join(b"".join((p2.hash_g1 if SECTION_GROUP[t] == 1 else p2.hash_g2)(P) for P in secs[t])
                    for t in (2, 3, 4, 5, 6))


def compressed_form(secs):
    return b"".join(b"".join((compress_g1 if SECTION_GROUP[t] == 1 else compress_g2)(P) for P in secs[t])
                    for t in (2, 3, 4, 5, 6))


def fresh_challenge(power):
    n = 1 << power
    secs = {2: [bn.G1_GEN] * (2 * n - 1), 3: [bn.G2_GEN] * n, 4: [bn.G1_GEN] * n, 5: [bn.G1_GEN] * n, 6: [bn.G2_GEN]}
    return blake2b(blake2b(b"") + hash_form(secs))


# ---- the key and the records ------------------------------------------------------------------------------------------
def g2_sp(k, challenge, g1_s, g1_sx):
    return p2.hash_to_g2(blake2b(bytes([k]) + challenge + p2.hash_g1(g1_s) + p2.hash_g1(g1_sx)))


def make_key(xs, g1_ss, challenge):
    """xs = (tau, alpha, beta), g1_ss their g1_s -> the nine points: six in G1 (g1_s, g1_sx per key), three in G2."""
    g1, g2 = [], []
    for k in range(3):
        sx = bn.g1_mul(g1_ss[k], xs[k])
        g1 += [g1_ss[k], sx]
        g2.append(bn.g2_mul(g2_sp(k, challenge, g1_ss[k], sx), xs[k]))
    return g1, g2


def beacon_secrets(beacon, exp):
    """Per key tau, alpha, beta: the secret, then g1_s, from one generator."""
    rng = p2.ChaCha(p2.beacon_key(beacon, exp))
    xs, ss = [], []
    for _ in range(3):
        xs.append(p2.fr_from_rng(rng))
        ss.append(p2.g1_from_rng(rng))
    return xs, ss


def params(type_, name=b"", exp=0, beacon=b""):
    out = b""
    if name:
        out += bytes([1, len(name)]) + name
    if type_ == 1:
        out += bytes([2, exp]) + bytes([3, len(beacon)]) + beacon
    return out


class Record:
    def __init__(self, points, key_g1, key_g2, partial, next_challenge, type_=0, name=b"", exp=0, beacon=b""):
        self.points, self.key_g1, self.key_g2 = points, key_g1, key_g2       # points: tauG1, tauG2, alphaG1, betaG1, betaG2
        self.partial, self.next_challenge = partial, next_challenge
        self.type, self.name, self.exp, self.beacon = type_, name, exp, beacon

    def to_bytes(self):
        t1, t2, a1, b1, b2 = self.points
        pr = params(self.type, self.name, self.exp, self.beacon)
        return (g16.g1_to_bytes(t1) + g16.g2_to_bytes(t2) + g16.g1_to_bytes(a1) + g16.g1_to_bytes(b1) +
                g16.g2_to_bytes(b2) + b"".join(g16.g1_to_bytes(P) for P in self.key_g1) +
                b"".join(g16.g2_to_bytes(P) for P in self.key_g2) + self.partial + self.next_challenge +
                struct.pack("<II", self.type, len(pr)) + pr)

    def response_hash(self):
        h = Blake2b.from_state(self.partial)
        h.update(b"".join(p2.hash_g1(P) for P in self.key_g1) + b"".join(p2.hash_g2(P) for P in self.key_g2))
        return h.digest()


def parse_record(b, at=0):
    """-> (Record, bytes consumed)"""
    pts = (g16.g1_from_bytes(b, at), g16.g2_from_bytes(b, at + 64), g16.g1_from_bytes(b, at + 192),
           g16.g1_from_bytes(b, at + 256), g16.g2_from_bytes(b, at + 320))
    k1 = [g16.g1_from_bytes(b, at + 448 + 64 * i) for i in range(6)]
    k2 = [g16.g2_from_bytes(b, at + 832 + 128 * i) for i in range(3)]
    partial = b[at + 1216:at + 1216 + STATE_LEN]
    nxt = b[at + 1432:at + 1496]
    type_, plen = struct.unpack_from("<II", b, at + 1496)
    pr = b[at + RECORD_FIXED:at + RECORD_FIXED + plen]
    name, exp, beacon, i = b"", 0, b"", 0
    while i < plen:
        tag = pr[i]
        if tag == 2:
            exp, i = pr[i + 1], i + 2
        elif tag in (1, 3):
            val = pr[i + 2:i + 2 + pr[i + 1]]
            name, beacon = (val, beacon) if tag == 1 else (name, val)
            i += 2 + pr[i + 1]
        else:
            raise ValueError("unknown tag")
    return Record(pts, k1, k2, partial, nxt, type_, name, exp, beacon), RECORD_FIXED + plen


def next_record(challenge, new_secs, xs, g1_ss, type_=0, name=b"", exp=0, beacon=b""):
    """The record of a contribution with secrets xs whose result is new_secs ({2..6: [points]}), after `challenge`."""
    k1, k2 = make_key(xs, g1_ss, challenge)
    h = Blake2b().update(challenge).update(compressed_form(new_secs))
    partial = h.state()
    h.update(b"".join(p2.hash_g1(P) for P in k1) + b"".join(p2.hash_g2(P) for P in k2))
    nxt = blake2b(h.digest() + hash_form(new_secs))
    pts = (new_secs[2][1], new_secs[3][1], new_secs[4][0], new_secs[5][0], new_secs[6][0])
    return Record(pts, k1, k2, partial, nxt, type_, name, exp, beacon)


def section7(records):
    return struct.pack("<I", len(records)) + b"".join(r.to_bytes() for r in records)
