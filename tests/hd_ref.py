"""Big-integer restatement of the HD-wallet key sources (include/zkpoa_hd_wallet.h): BIP-32's master key and child-key
step for private and public parents, paths, the reading and (for the tests: with a zero fingerprint) the writing of
xprv / xpub strings, and BIP-39's seed. Independent of the device code: hashlib and hmac for SHA-512, HMAC and PBKDF2,
tests/secp_ref.py and tests/sign_ref.py for the curve, Keccak and the addresses. tests/test_hd_ref.py holds it against
the published vectors of tests/golden/hd/vectors.json."""
import hashlib
import hmac

import secp_ref as sr
import sign_ref as sg

N, P, G = sr.N, sr.P, sr.G
HARDENED = 1 << 31
OK, INVALID = 0, 1
XPRV, XPUB = 0x0488ADE4, 0x0488B21E
B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"

ZERO_CHILD = dict(status=INVALID, key=bytes(33), chain=bytes(32), pub=(0, 0), address=bytes(20))


def hmac512(key, msg):
    return hmac.new(key, msg, hashlib.sha512).digest()


# ---- key data ------------------------------------------------------------------------------------------------------------
def ser_p(pt):
    """The compressed point: 02 / 03 || x."""
    return bytes([2 + (pt[1] & 1)]) + pt[0].to_bytes(32, "big")


def priv_data(k):
    return b"\x00" + k.to_bytes(32, "big")


def is_private(key33):
    return key33[0] == 0


def point_of(key33):
    """The public point of 33 bytes of key data (either kind), or None when they are none."""
    if key33[0] == 0:
        k = int.from_bytes(key33[1:], "big")
        return sg.mul_g(k) if 0 < k < N else None
    if key33[0] not in (2, 3):
        return None
    x = int.from_bytes(key33[1:], "big")
    return sr.lift_x(x, key33[0] == 3) if x < P else None


# ---- the child-key step --------------------------------------------------------------------------------------------------
def tweak(parent33, il):
    """The second half of CKDpriv / CKDpub for a 256-bit IL: dict(status, key (33 B), pub, address). Invalid (status 1,
    zeros): IL >= n, a child key of 0, a child point at infinity -- and IL = 0 under either kind of parent (0 G has no
    affine form; the library refuses it on both sides so that an xprv and its xpub always tell the same)."""
    zero = {k: v for k, v in ZERO_CHILD.items() if k != "chain"}
    if not 0 < il < N:
        return dict(zero)
    if is_private(parent33):
        k = (il + int.from_bytes(parent33[1:], "big")) % N
        if k == 0:
            return dict(zero)
        pub = sg.mul_g(k)
        return dict(status=OK, key=priv_data(k), pub=pub, address=sr.eth_address(pub))
    pub = sr.add(sg.mul_g(il), point_of(parent33))
    if pub is None:
        return dict(zero)
    return dict(status=OK, key=ser_p(pub), pub=pub, address=sr.eth_address(pub))


def child(parent33, chain, i):
    """Child i of (key data, chain code): dict(status, key, chain, pub, address). A hardened child of a public parent does
    not exist: ValueError."""
    if i >= HARDENED:
        if not is_private(parent33):
            raise ValueError("a hardened child of a public key")
        data = parent33
    else:
        data = ser_p(point_of(parent33))
    big_i = hmac512(chain, data + i.to_bytes(4, "big"))
    out = tweak(parent33, int.from_bytes(big_i[:32], "big"))
    out["chain"] = big_i[32:] if out["status"] == OK else bytes(32)
    return out


def neuter(key33):
    return ser_p(point_of(key33))


# ---- seeds, paths, extended keys -----------------------------------------------------------------------------------------
def master(seed):
    big_i = hmac512(b"Bitcoin seed", seed)
    k = int.from_bytes(big_i[:32], "big")
    if not 0 < k < N:
        raise ValueError("no master key")
    return priv_data(k), big_i[32:]


def bip39_seed(mnemonic, passphrase=""):
    return hashlib.pbkdf2_hmac("sha512", mnemonic.encode(), b"mnemonic" + passphrase.encode(), 2048, 64)


def parse_path(path):
    """"m/44'/60'/0'/0" -> [indices]; ValueError for anything else."""
    parts = path.split("/")
    if parts[0] != "m" or len(parts) > 256:
        raise ValueError(path)
    out = []
    for part in parts[1:]:
        hard = part[-1:] in ("'", "h")
        digits = part[:-1] if hard else part
        if not digits or not digits.isascii() or not digits.isdigit() or int(digits) >= HARDENED:
            raise ValueError(path)
        out.append(int(digits) + (HARDENED if hard else 0))
    return out


def derive_path(key33, chain, path):
    for i in parse_path(path):
        c = child(key33, chain, i)
        if c["status"] != OK:
            raise ValueError("invalid child")
        key33, chain = c["key"], c["chain"]
    return key33, chain


def b58encode(raw):
    v = int.from_bytes(raw, "big")
    text = ""
    while v:
        v, r = divmod(v, 58)
        text = B58[r] + text
    return "1" * (len(raw) - len(raw.lstrip(b"\0"))) + text


def b58decode(text):
    v = 0
    for ch in text:
        v = v * 58 + B58.index(ch)        # ValueError for a character outside the alphabet
    zeros = len(text) - len(text.lstrip("1"))
    return bytes(zeros) + v.to_bytes((v.bit_length() + 7) // 8, "big")


def checksum4(raw):
    return hashlib.sha256(hashlib.sha256(raw).digest()).digest()[:4]


def serialize(key33, chain, depth=0, index=0, fingerprint=bytes(4), version=None):
    """The xprv / xpub string of key data. The fingerprint is a RIPEMD-160, which this restatement does not have: zeros by
    default, and a reader ignores the field."""
    if version is None:
        version = XPRV if is_private(key33) else XPUB
    raw = version.to_bytes(4, "big") + bytes([depth]) + fingerprint + index.to_bytes(4, "big") + chain + key33
    return b58encode(raw + checksum4(raw))


def parse_key(text):
    """-> (key data, chain code, depth, child index); ValueError for anything that is no xprv / xpub."""
    raw = b58decode(text)
    if len(raw) != 82 or checksum4(raw[:78]) != raw[78:]:
        raise ValueError("length or checksum")
    version, key33 = int.from_bytes(raw[:4], "big"), raw[45:78]
    if version not in (XPRV, XPUB) or (version == XPRV) != is_private(key33) or point_of(key33) is None:
        raise ValueError("version or key")
    return key33, raw[13:45], raw[4], int.from_bytes(raw[9:13], "big")


def hd_balance(address20):
    """The balance `sign`, `anon-set` give an HD account: its address as an integer, mod 1000."""
    return int.from_bytes(address20, "big") % 1000
