"""Big-integer restatement of the ecdsa-sigs-parser step: secp256k1 public-key recovery in the ECDSA* form, Keccak-256,
Ethereum addresses with the EIP-55 checksum, the two JSON texts of the command, and a generator of signatures whose
answers are known by construction. Independent of the device code (plain Python integers) and of ethers / noble."""
import copy
import json
import random

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8
G = (GX, GY)

OK, BAD_V, BAD_SCALAR, HIGH_S, NOT_ON_CURVE, INFINITY, ADDRESS = range(7)


# ---- the curve: affine points as (x, y), infinity as None ------------------------------------------------------------
def on_curve(pt):
    return pt is not None and (pt[1] * pt[1] - pt[0] ** 3 - 7) % P == 0


def add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return (x, (lam * (a[0] - x) - a[1]) % P)


def neg(a):
    return None if a is None else (a[0], (P - a[1]) % P)


def _jdbl(p):
    x, y, z = p
    if z == 0 or y == 0:
        return (0, 1, 0)
    s = 4 * x * y * y % P
    m = 3 * x * x % P
    x3 = (m * m - 2 * s) % P
    return (x3, (m * (s - x3) - 8 * pow(y, 4, P)) % P, 2 * y * z % P)


def _jadd_affine(p, q):
    x1, y1, z1 = p
    if z1 == 0:
        return (q[0], q[1], 1)
    zz = z1 * z1 % P
    u2 = q[0] * zz % P
    s2 = q[1] * zz * z1 % P
    h = (u2 - x1) % P
    r = (s2 - y1) % P
    if h == 0:
        return _jdbl(p) if r == 0 else (0, 1, 0)
    hh = h * h % P
    hhh = h * hh % P
    v = x1 * hh % P
    x3 = (r * r - hhh - 2 * v) % P
    return (x3, (r * (v - x3) - y1 * hhh) % P, z1 * h % P)


def mul(k, pt):
    """k * pt by double-and-add in Jacobian coordinates (one inversion at the end)."""
    k %= N
    if pt is None or k == 0:
        return None
    acc = (0, 1, 0)
    for bit in bin(k)[2:]:
        acc = _jdbl(acc)
        if bit == "1":
            acc = _jadd_affine(acc, pt)
    if acc[2] == 0:
        return None
    zi = pow(acc[2], -1, P)
    return (acc[0] * zi * zi % P, acc[1] * zi * zi * zi % P)


def lift_x(x, odd):
    """The point with this x coordinate and this parity of y, or None when x^3 + 7 is not a square."""
    rhs = (x * x * x + 7) % P
    y = pow(rhs, (P + 1) // 4, P)
    if y * y % P != rhs:
        return None
    return (x, y if (y & 1) == int(odd) else P - y)


def verify(r, s, z, pub):
    if not (0 < r < N and 0 < s < N and on_curve(pub)):
        return False
    si = pow(s, -1, N)
    pt = add(mul(z * si % N, G), mul(r * si % N, pub))
    return pt is not None and pt[0] % N == r


# ---- Keccak ----------------------------------------------------------------------------------------------------------
_RC = [0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B,
       0x0000000080000001, 0x8000000080008081, 0x8000000000008009, 0x000000000000008A, 0x0000000000000088,
       0x0000000080008009, 0x000000008000000A, 0x000000008000808B, 0x800000000000008B, 0x8000000000008089,
       0x8000000000008003, 0x8000000000008002, 0x8000000000000080, 0x000000000000800A, 0x800000008000000A,
       0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008]
_M64 = (1 << 64) - 1


def _rol(v, n):
    n %= 64
    return ((v << n) | (v >> (64 - n))) & _M64 if n else v


def keccak_f1600(a):
    """a: 25 lanes, lane (x, y) at a[x + 5 y]; returns the permuted state."""
    a = list(a)
    for rnd in range(24):
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        for x in range(5):
            d = c[(x + 4) % 5] ^ _rol(c[(x + 1) % 5], 1)
            for y in range(5):
                a[x + 5 * y] ^= d
        # rho and pi along the single orbit of (x, y) -> (y, 2x + 3y), rotation (t + 1)(t + 2) / 2 at step t
        x, y = 1, 0
        cur = a[1]
        for t in range(24):
            x, y = y, (2 * x + 3 * y) % 5
            cur, a[x + 5 * y] = a[x + 5 * y], _rol(cur, (t + 1) * (t + 2) // 2)
        for y in range(5):
            row = a[5 * y:5 * y + 5]
            for x in range(5):
                a[x + 5 * y] = row[x] ^ (~row[(x + 1) % 5] & _M64 & row[(x + 2) % 5])
        a[0] ^= _RC[rnd]
    return a


def sponge256(msg, pad):
    """32-byte digest of the rate-136 sponge; pad 0x01: Keccak-256 (Ethereum), pad 0x06: SHA3-256."""
    rate = 136
    m = bytearray(msg)
    m.append(pad)
    while len(m) % rate:
        m.append(0)
    m[-1] |= 0x80
    a = [0] * 25
    for off in range(0, len(m), rate):
        for w in range(rate // 8):
            a[w] ^= int.from_bytes(m[off + 8 * w:off + 8 * w + 8], "little")
        a = keccak_f1600(a)
    return b"".join(v.to_bytes(8, "little") for v in a[:4])


def keccak256(msg):
    return sponge256(msg, 0x01)


def eth_address(pub):
    """The 20 address bytes of an uncompressed key (ethers.computeAddress without the checksum)."""
    return keccak256(pub[0].to_bytes(32, "big") + pub[1].to_bytes(32, "big"))[12:]


def checksum(addr20):
    """EIP-55 text of 20 address bytes."""
    text = addr20.hex()
    h = keccak256(text.encode()).hex()
    return "0x" + "".join(ch.upper() if ch in "abcdef" and int(h[i], 16) >= 8 else ch for i, ch in enumerate(text))


# ---- recovery --------------------------------------------------------------------------------------------------------
def recover(r, s, v, z, address20=None):
    """(status, r_prime, (x, y), derived address bytes). The first status that applies wins; statuses 1-5 give zeros,
    status 6 keeps what was derived. z: the message hash as a 256-bit integer; address20: the address claimed."""
    zero = (0, (0, 0), bytes(20))
    if v not in (27, 28):
        return (BAD_V,) + zero
    if not (0 < r < N and 0 < s < N):
        return (BAD_SCALAR,) + zero
    if s >= 1 << 255:
        return (HIGH_S,) + zero
    big_r = lift_x(r, v == 28)
    if big_r is None:
        return (NOT_ON_CURVE,) + zero
    ri = pow(r, -1, N)
    q = add(mul(s * ri % N, big_r), mul(-(z % N) * ri % N, G))
    if q is None:
        return (INFINITY,) + zero
    addr = eth_address(q)
    status = OK if address20 is None or bytes(address20) == addr else ADDRESS
    return status, big_r[1], q, addr


# ---- signatures with known answers -----------------------------------------------------------------------------------
def generate(count, seed, low_s=True):
    """count signatures without a scalar multiplication per entry: nonce points R_i = R_0 + i G and keys Q_i = Q_0 + i G
    walked by additions, z random, s = (z + r d) / k. With low_s an s >= 2^255 is replaced by n - s (and v flips, and so
    does r'). Each entry: dict(r, s, v, z, rprime, pub, address (20 bytes), d, k)."""
    rng = random.Random(seed)
    k = rng.randrange(1, N - count)
    d = rng.randrange(1, N - count)
    big_r, q = mul(k, G), mul(d, G)
    out = []
    for _ in range(count):
        r = big_r[0]
        assert 0 < r < N   # an x coordinate in [n, p) has probability 2^-128
        z = rng.getrandbits(256)
        s = pow(k, -1, N) * (z + r * d) % N
        assert s
        v, rprime = 27 + (big_r[1] & 1), big_r[1]
        if low_s and s >= 1 << 255:
            s, v, rprime = N - s, 55 - v, P - rprime
        out.append(dict(r=r, s=s, v=v, z=z, rprime=rprime, pub=q, address=eth_address(q), d=d, k=k))
        big_r, q, k, d = add(big_r, G), add(q, G), k + 1, d + 1
    return out


def sign(k, d, z):
    """One signature with nonce k and key d, low s: the entry generate() would give."""
    k %= N
    big_r, q = mul(k, G), mul(d, G)
    r = big_r[0] % N
    s = pow(k, -1, N) * (z + r * d) % N
    v, rprime = 27 + (big_r[1] & 1), big_r[1]
    if s >= 1 << 255:
        s, v, rprime = N - s, 55 - v, P - rprime
    return dict(r=r, s=s, v=v, z=z % (1 << 256), rprime=rprime, pub=q, address=eth_address(q), d=d, k=k)


# ---- the command's two texts -----------------------------------------------------------------------------------------
def hex32(v):
    return "0x%064x" % v


def signatures_json(entries, balances=None):
    """The input file of the parsing mode for generated entries (balance i + 1, every other one with the trailing n)."""
    out = []
    for i, e in enumerate(entries):
        bal = balances[i] if balances else "%d%s" % (i + 1, "n" if i % 2 == 0 else "")
        out.append({"signature": {"r": hex32(e["r"]), "s": hex32(e["s"]), "v": e["v"], "msghash": hex32(e["z"])},
                    "address": checksum(e["address"]), "balance": bal})
    return json.dumps(out)


def _big(v):
    return {"__bigint__": str(v)}


def parser_output_text(signatures_text, known=None):
    """What JSON.stringify(outputData, jsonReplacer, 2) of scripts/ecdsa_sigs_parser.ts writes for this input text.
    known: the generator's entries for this text, whose answers then stand in for a recovery per entry."""
    atts = []
    for i, e in enumerate(json.loads(signatures_text)):
        sig = e["signature"]
        r, s, z = int(sig["r"], 16), int(sig["s"], 16), int(sig["msghash"], 16)
        given = bytes.fromhex(e["address"][2:])
        if known is not None:
            assert (known[i]["r"], known[i]["s"], known[i]["z"], known[i]["v"]) == (r, s, z, sig["v"])
            status, rprime, pub, addr = OK, known[i]["rprime"], known[i]["pub"], known[i]["address"]
            status = OK if addr == given else ADDRESS
        else:
            status, rprime, pub, addr = recover(r, s, sig["v"], z, given)
        if status != OK or checksum(addr) != e["address"]:
            raise ValueError("entry %d: status %d" % (i, status))
        bal = e["balance"]
        atts.append({"signature": {"r": _big(r), "s": _big(s), "r_prime": _big(rprime),
                                   "pubkey": {"x": _big(pub[0]), "y": _big(pub[1])},
                                   "msghash": {"__uint8array__": list(z.to_bytes(32, "big"))}},
                     "accountData": {"address": _big(int.from_bytes(addr, "big")),
                                     "balance": _big(int(bal[:-1] if bal.endswith("n") else bal))}})
    return json.dumps({"accountAttestations": atts}, indent=2)


def limbs64(v):
    return [str((v >> (64 * i)) & _M64) for i in range(4)]


def layer_one_text(parser_text, start=0, end=-1):
    """What scripts/input_prep_for_layer_one.ts writes for the parser's output text and an index range."""
    atts = json.loads(parser_text)["accountAttestations"]
    if end == -1:
        end = len(atts)
    if start >= end:
        raise ValueError("startIndex %d must be less than endIndex %d" % (start, end))
    out = {"r": [], "s": [], "rprime": [], "pubkey": [], "msghash": []}
    for a in atts[start:end]:
        sig = a["signature"]
        out["r"].append(limbs64(int(sig["r"]["__bigint__"])))
        out["s"].append(limbs64(int(sig["s"]["__bigint__"])))
        out["rprime"].append(limbs64(int(sig["r_prime"]["__bigint__"])))
        out["pubkey"].append([limbs64(int(sig["pubkey"]["x"]["__bigint__"])), limbs64(int(sig["pubkey"]["y"]["__bigint__"]))])
        out["msghash"].append(limbs64(int.from_bytes(bytes(sig["msghash"]["__uint8array__"]), "big")))
    return json.dumps(out, indent=2)


def with_unknown_members(doc, bare=0):
    """A parsed-signatures document with members no reader of it knows: nested arrays and objects, strings with escapes,
    true / false / null, negative and exponent numbers, and under keys that begin with "extra" (which
    tools/host_text_check.cpp skips whole) keys with escapes and a __bigint__ that is not one of the file's. accountData
    comes before signature, and entry `bare` has its address as a bare number."""
    nest = {"flags": [True, False, None], "numbers": [-12, 2.5e-3, -1E+20, 0], "deep": [[1, [2, {"k": "v \" \\ \u00e9"}]], [], {}]}
    out = {"extra_head": {"accountAttestations": [{"__bigint__": "7"}], "k\"e\\y\u00e9": [[], {}, [[["x"]]]]}, "version": 3}
    atts = []
    for i, a in enumerate(doc["accountAttestations"]):
        data = copy.deepcopy(a["accountData"])
        if i == bare:
            data["address"] = {"__bigint__": int(data["address"]["__bigint__"])}
        data = dict({"extra_note": "quote \" backslash \\ e-acute \u00e9 brackets ]}["}, **data, label="it's \"mine\"", tags=nest)
        atts.append({"extra": [{"__bigint__": "8", "s\\": None}], "accountData": data, "meta": nest,
                     "signature": a["signature"]})
    out["accountAttestations"] = atts
    out["trailer"] = {"count": len(atts), "ok": True, "extra_tail": "\\"}
    return out
