"""Big-integer restatement of `ecdsa-sigs-parser sign` and `anon-set`: the RFC 6979 nonce (HMAC-SHA256 DRBG, section 3.2,
no extra entropy) with hashlib / hmac, ECDSA signing with low s on top of tests/secp_ref.py, the derived keys, the filler
accounts of the anonymity set, the key-file reader and the two output texts. Independent of the device code (plain Python
integers and the standard library's hashes) and of noble / ethers."""
import hashlib
import hmac

import secp_ref as sr

N, P, G = sr.N, sr.P, sr.G
OK, BAD_KEY, HIGH_X = 0, 1, 2


def be32(v):
    return int(v).to_bytes(32, "big")


# ---- RFC 6979 --------------------------------------------------------------------------------------------------------
def nonce_candidates(d, z):
    """The candidates k of section 3.2 for key d and the 256-bit message hash z, valid or not, one after the other."""
    x = be32(d)                       # int2octets
    h = be32(z - N if z >= N else z)  # bits2octets: bits2int is the identity at qlen = 256, then one subtraction
    v, k = b"\x01" * 32, b"\x00" * 32
    mac = lambda key, msg: hmac.new(key, msg, hashlib.sha256).digest()
    k = mac(k, v + b"\x00" + x + h)
    v = mac(k, v)
    k = mac(k, v + b"\x01" + x + h)
    v = mac(k, v)
    while True:
        v = mac(k, v)                 # tlen = qlen after one round
        yield int.from_bytes(v, "big")
        k = mac(k, v + b"\x00")
        v = mac(k, v)


def nonce(d, z, skip=0):
    """The candidate after `skip` refusals, whether or not it is in [1, n)."""
    gen = nonce_candidates(d, z)
    for _ in range(skip):
        next(gen)
    return next(gen)


# ---- k G, quickly ----------------------------------------------------------------------------------------------------
_ROWS = []


def mul_g(k):
    """k G for 0 < k < n. The tests sign some ten thousand times, and secp_ref.mul's double-and-add takes 1.6 ms: this one
    adds one entry of a table m 16^i G (m = 1 .. 15, plain unsigned digits) per non-zero nibble, in Jacobian coordinates.
    tests/test_sign_ref.py holds it against secp_ref.mul."""
    if not _ROWS:
        base = G
        for _ in range(64):
            row = [None, base]
            for _m in range(2, 16):
                row.append(sr.add(row[-1], base))
            _ROWS.append(row)
            base = sr.add(row[15], base)
    acc = (0, 1, 0)
    for i in range(64):
        m = (k >> (4 * i)) & 15
        if m:
            acc = sr._jadd_affine(acc, _ROWS[i][m])
    zi = pow(acc[2], -1, P)
    return (acc[0] * zi * zi % P, acc[1] * zi * zi * zi % P)


# ---- signing ---------------------------------------------------------------------------------------------------------
ZERO = dict(status=BAD_KEY, r=0, s=0, v=0, pub=(0, 0), address=bytes(20))


def sign(d, z, key=None):
    """dict(status, r, s, v, pub, address (20 bytes), k): what noble's sign(msghash, key, {canonical: true, recovered:
    true}) and ethers' Wallet give. z: the hash as a 256-bit integer. Status 1 (key zero or not below n) and 2 (the nonce
    point's x is not below n) come with zeros. key: public_key(d) when the caller has it already."""
    if not 0 < d < N:
        return dict(ZERO)
    key = key or public_key(d)
    pub = key["pub"]
    for k in nonce_candidates(d, z):
        if not 0 < k < N:
            continue
        big_r = mul_g(k)
        if big_r[0] >= N:
            return dict(ZERO, status=HIGH_X)
        r = big_r[0]
        s = pow(k, -1, N) * (z % N + r * d) % N
        if r == 0 or s == 0:
            continue
        bit = big_r[1] & 1
        if s > (N - 1) // 2:
            s, bit = N - s, bit ^ 1
        return dict(status=OK, r=r, s=s, v=27 + bit, pub=pub, address=key["address"], k=k)


def public_key(d):
    if not 0 < d < N:
        return dict(status=BAD_KEY, pub=(0, 0), address=bytes(20))
    pub = mul_g(d)
    return dict(status=OK, pub=pub, address=sr.eth_address(pub))


# ---- the edge cases of the device and host checks --------------------------------------------------------------------
def edge_keys():
    """Keys at the borders of the signed 4-bit recoding (digits 7, 8, 9 and 15 at the lowest, a middle and the top window,
    carries running through every window), of the halving at (n - 1) / 2, and of the range."""
    keys = [1, 2, 7, 8, 9, 15, 16]
    for i in (1, 31, 63):
        keys += [k for k in (8 * 16**i, 9 * 16**i, 16**i - 1) if k < N]
    keys += [int("8" * 64, 16), int("7" * 64, 16), (N - 1) // 2, (N + 1) // 2, 1 << 255, N - 2, N - 1]
    return list(dict.fromkeys(keys))   # (8 * 16^63 is 2^255, 16 - 1 is 15: once each)


INVALID_KEYS = [0, N, N + 1, (1 << 256) - 1]


def edge_hashes(rng):
    return [0, N, (1 << 256) - 1, rng.getrandbits(256)]


# ---- keys and accounts -----------------------------------------------------------------------------------------------
def derive_key(seed, i):
    """Key i of --generate-keys --seed: (SHA-256(seed || be64(i)) mod (n - 1)) + 1."""
    return int.from_bytes(hashlib.sha256(seed + i.to_bytes(8, "big")).digest(), "big") % (N - 1) + 1


def default_balance(d):
    return d % 1000


def read_key_file(text):
    """[(key, balance)] of a key file: <decimal or 0x-hex key>[,<decimal balance>] per line, blank lines and # comments
    skipped."""
    out = []
    for line in text.split("\n"):
        line = line.strip(" \t\r")
        if not line or line.startswith("#"):
            continue
        key, _, bal = line.partition(",")
        key = key.strip(" \t\r")
        d = int(key[2:], 16) if key[:2] in ("0x", "0X") else int(key, 10)
        out.append((d, int(bal.strip(" \t\r"), 10) if bal else default_balance(d)))
    return out


def key_file_text(keys):
    """What --write-keys writes."""
    return "".join("0x%064x\n" % d for d in keys)


def filler_account(seed, j):
    """Filler account j of the anonymity set: (address as an integer, balance)."""
    dig = sr.keccak256(seed + b"anon" + j.to_bytes(8, "big"))
    return int.from_bytes(dig[12:], "big"), int.from_bytes(dig[:8], "big") % 10**6


# ---- the two output texts --------------------------------------------------------------------------------------------
def signatures_text(entries):
    """JSON.stringify(data) of SignatureData[] for (r, s, v, z, address bytes, balance) entries, sorted by address: the
    spelling of the reference's tests/signatures_<n>.json."""
    parts = []
    for r, s, v, z, address, balance in sorted(entries, key=lambda e: e[4]):
        parts.append('{"signature":{"r":"%s","s":"%s","v":%d,"msghash":"%s"},"address":"%s","balance":"%dn"}'
                     % (sr.hex32(r), sr.hex32(s), v, sr.hex32(z), sr.checksum(address), balance))
    return "[" + ",".join(parts) + "]"


def sign_text(keys_and_balances, z):
    """The output of `sign` for these keys and this hash."""
    entries = []
    for d, bal in keys_and_balances:
        g = sign(d, z)
        assert g["status"] == OK
        entries.append((g["r"], g["s"], g["v"], z, g["address"], bal))
    return signatures_text(entries)


def anon_set_csv(accounts):
    """The CSV of tests/generate_anon_set.ts for (address as an integer, balance) pairs."""
    return "address,eth_balance\n" + "".join("0x%064x,%d\n" % a for a in sorted(accounts, key=lambda a: a[0]))


def anon_set_text(keys_and_balances, seed, total):
    """The output of `anon-set --num-addresses total`: the first min(total, keys) keys' accounts, then fillers."""
    owned = keys_and_balances[:total]
    accounts = [(int.from_bytes(public_key(d)["address"], "big"), bal) for d, bal in owned]
    accounts += [filler_account(seed, j) for j in range(total - len(owned))]
    return anon_set_csv(accounts)
