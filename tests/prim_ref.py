"""Big-int reference and input sets for the primitive-level device hooks (include/zkpoa_prover.h, zkpoa_field_prim /
zkpoa_curve_prim). Test infrastructure, written against oracle/py/bn254.py only: values are raw Montgomery-form
integers as the device holds them (lazy, in [0, 2p) unless an op allows more), results are compared mod p and
checked against the output range each primitive promises (csrc/bn254_field.hip.h, csrc/bn254_ec.hip.h)."""
from oracle.py import bn254 as bn
from oracle.py import groth16 as g16

Q, R, M = bn.Q, bn.R, bn.MONT_R

# name -> (op id, operands, results), as zkpoa_field_prim numbers them for Fq / Fr
FIELD_OPS = {
    "mul": (0, 2, 1), "sqr": (1, 1, 1), "add": (2, 2, 1), "sub": (3, 2, 1), "neg": (4, 1, 1), "neg_2p": (5, 1, 1),
    "dbl": (6, 1, 1), "canon": (7, 1, 1), "reduce_2p": (8, 1, 1), "inv": (9, 1, 1), "dot2": (10, 4, 1),
    "dot3": (11, 6, 1), "mul_pair": (12, 4, 2), "sqr_pair": (13, 2, 2), "dot2_pair": (14, 8, 2),
    "is_zero": (15, 1, 1), "eq": (16, 2, 1),
}
FQ2_OPS = {"mul": (0, 2), "sqr": (1, 1), "add": (2, 2), "sub": (3, 2), "neg": (4, 1), "inv": (5, 1)}
CURVE_OPS = {"add": 0, "add_affine": 1, "dbl": 2, "dbl_affine": 3, "mul_small": 4}


# ---- bytes <-> raw integers -------------------------------------------------------------------------
def pack(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def unpack(buf):
    return [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]


def pack2(vals):
    return b"".join(int(c).to_bytes(32, "little") for v in vals for c in v)


def unpack2(buf):
    v = unpack(buf)
    return [(v[i], v[i + 1]) for i in range(0, len(v), 2)]


# ---- input sets ------------------------------------------------------------------------------------
def edge_set(p):
    """Raw values in [0, 2p) where a lazy Montgomery layer goes wrong: the two representations of 0, 1 and -1, the
    ends of the range, limb boundaries, single-limb neighbours of p and 2p, saturated and bit-31-heavy limbs."""
    rm = M % p
    top2p = (2 * p) >> 224
    v = [0, 1, 2, p - 2, p - 1, p, p + 1, p + 2, 2 * p - 2, 2 * p - 1,
         rm, rm + p, p - rm, 2 * p - rm, M * M % p, (p - 1) // 2, (p + 1) // 2, 1 << 253, 1 << 254]
    for j in range(1, 8):
        v += [(1 << (32 * j)) - 1, 1 << (32 * j)]
    for j in range(8):
        v += [p + (1 << (32 * j)), p - (1 << (32 * j)), 2 * p - (1 << (32 * j))]
    v.append((top2p << 224) - 1)                        # largest below 2p with limbs 0..6 all 0xFFFFFFFF
    b31 = sum(0x80000000 << (32 * j) for j in range(7))
    for top in (0, 1, p >> 224, top2p - 1):
        v.append((top << 224) | b31)
        v.append((top << 224) | b31 | (b31 >> 1))
    out = sorted(set(v))
    assert all(0 <= x < 2 * p for x in out)
    return out


def uniform(rng, n, hi):
    return [rng.randrange(hi) for _ in range(n)]


def near_max(rng, n, top):
    """uniform in [top - 2^200, top)"""
    return [top - 1 - rng.randrange(1 << 200) for _ in range(n)]


# ---- field reference (raw Montgomery values in, residues mod p out) ---------------------------------
def field_ref(name, p, ops):
    """Expected results of FIELD_OPS[name] on operand lists `ops`: one list per result, values mod p (is_zero / ==:
    the exact 0 / 1 flag)."""
    ri = pow(M, -1, p)
    m2 = M * M % p
    z = list(zip(*ops))
    if name == "mul":
        return [[a * b * ri % p for a, b in z]]
    if name == "sqr":
        return [[a * a * ri % p for (a,) in z]]
    if name == "add":
        return [[(a + b) % p for a, b in z]]
    if name == "sub":
        return [[(a - b) % p for a, b in z]]
    if name in ("neg", "neg_2p"):
        return [[-a % p for (a,) in z]]
    if name == "dbl":
        return [[2 * a % p for (a,) in z]]
    if name in ("canon", "reduce_2p"):
        return [[a % p for (a,) in z]]
    if name == "inv":   # Montgomery form of (a/M)^-1 = M^2 / a, 0 -> 0 (the device takes a^(p-2))
        return [[pow(a, -1, p) * m2 % p if a % p else 0 for (a,) in z]]
    if name == "dot2":
        return [[(a0 * b0 + a1 * b1) * ri % p for a0, b0, a1, b1 in z]]
    if name == "dot3":
        return [[(a0 * b0 + a1 * b1 + a2 * b2) * ri % p for a0, b0, a1, b1, a2, b2 in z]]
    if name == "mul_pair":
        return [[a * b * ri % p for a, b, _, _ in z], [c * d * ri % p for _, _, c, d in z]]
    if name == "sqr_pair":
        return [[a * a * ri % p for a, _ in z], [b * b * ri % p for _, b in z]]
    if name == "dot2_pair":
        return [[(a0 * b0 + a1 * b1) * ri % p for a0, b0, a1, b1, _, _, _, _ in z],
                [(c0 * d0 + c1 * d1) * ri % p for _, _, _, _, c0, d0, c1, d1 in z]]
    if name == "is_zero":
        return [[int(a % p == 0) for (a,) in z]]
    if name == "eq":
        return [[int((a - b) % p == 0) for a, b in z]]
    raise KeyError(name)


def field_range(name, p):
    """(lo, hi): the raw result range [lo, hi] each primitive promises"""
    if name == "canon":
        return 0, p - 1
    if name == "neg_2p":
        return 1, 2 * p
    if name in ("is_zero", "eq"):
        return 0, 1
    return 0, 2 * p - 1


def field_mismatches(name, p, ops, outs, limit=5):
    """Every (result index, element index, operands, got, why) where a raw device result is wrong; [] if none."""
    want = field_ref(name, p, ops)
    lo, hi = field_range(name, p)
    bad = []
    for j, (w, g) in enumerate(zip(want, outs)):
        for i, (wv, gv) in enumerate(zip(w, g)):
            why = None
            if not lo <= gv <= hi:
                why = "out of range [%#x, %#x]" % (lo, hi)
            elif name in ("is_zero", "eq"):
                why = None if gv == wv else "flag"
            elif gv % p != wv:
                why = "value mod p"
            elif name == "neg" and ops[0][i] == 0 and gv != 0:
                why = "neg(0) != 0"
            if why:
                bad.append((j, i, [o[i] for o in ops], gv, why))
                if len(bad) >= limit:
                    return bad
    return bad


def fq2_ref(name, ops):
    """Fq2 ops on raw Montgomery (c0, c1) pairs -> residues mod Q per coordinate"""
    ri = pow(M, -1, Q)
    z = list(zip(*ops))
    if name in ("mul", "sqr"):
        out = []
        for t in z:
            a, b = (t[0], t[0]) if name == "sqr" else t
            out.append(((a[0] * b[0] - a[1] * b[1]) * ri % Q, (a[0] * b[1] + a[1] * b[0]) * ri % Q))
        return out
    if name == "add":
        return [((a[0] + b[0]) % Q, (a[1] + b[1]) % Q) for a, b in z]
    if name == "sub":
        return [((a[0] - b[0]) % Q, (a[1] - b[1]) % Q) for a, b in z]
    if name == "neg":
        return [(-a[0] % Q, -a[1] % Q) for (a,) in z]
    if name == "inv":
        out = []
        for (a,) in z:
            s = (a[0] * ri % Q, a[1] * ri % Q)
            if bn.FQ2.is_zero(s):
                out.append((0, 0))
            else:
                i0, i1 = bn.FQ2.inv(s)
                out.append((i0 * M % Q, i1 * M % Q))
        return out
    raise KeyError(name)


# ---- curve reference ---------------------------------------------------------------------------------
def curve_field(group):
    return bn.FQ if group == 1 else bn.FQ2


def coord_map(v, f):
    """apply f to a G1 coordinate (int) or to each component of a G2 coordinate (pair)"""
    return f(v) if isinstance(v, int) else tuple(f(c) for c in v)


def coord_ints(v):
    return [v] if isinstance(v, int) else list(v)


def to_mont(v):
    return coord_map(v, lambda c: c * M % Q)


def from_mont(v):
    ri = pow(M, -1, Q)
    return coord_map(v, lambda c: c * ri % Q)


def affine_bytes(group, P):
    return g16.g1_to_bytes(P) if group == 1 else g16.g2_to_bytes(P)


def affine_list(group, buf):
    size = 64 if group == 1 else 128
    fn = g16.g1_from_bytes if group == 1 else g16.g2_from_bytes
    return [fn(buf, off) for off in range(0, len(buf), size)]


def xyzz_of(group, P, lam, lazy=(False, False, False, False)):
    """Raw XYZZ (Montgomery) of the affine point P (standard form) with scale lam: (x lam^2, y lam^3, lam^2, lam^3).
    lazy[i]: coordinate i gets + p on every component (still < 2p: the device's other representation)."""
    F = curve_field(group)
    lam = lam if group == 1 else (lam, 0) if isinstance(lam, int) else lam
    l2 = F.sqr(lam)
    l3 = F.mul(l2, lam)
    coords = [to_mont(c) for c in (F.mul(P[0], l2), F.mul(P[1], l3), l2, l3)]
    return tuple(coord_map(c, lambda v: v + Q) if lz else c for c, lz in zip(coords, lazy))


def xyzz_inf(group, rng, zz_rep):
    """an XYZZ infinity: zz (and zzz) raw 0 or raw p (G2: that in c0, the other one in c1), garbage x and y"""
    def g():
        return rng.randrange(2 * Q) if group == 1 else (rng.randrange(2 * Q), rng.randrange(2 * Q))
    z = zz_rep if group == 1 else (zz_rep, Q - zz_rep)
    return (g(), g(), z, z)


def xyzz_bytes(points):
    return b"".join(pack(c for v in pt for c in coord_ints(v)) for pt in points)


def xyzz_list(group, buf):
    vals = unpack(buf)
    if group == 1:
        return [tuple(vals[i:i + 4]) for i in range(0, len(vals), 4)]
    return [tuple((vals[i + 2 * j], vals[i + 2 * j + 1]) for j in range(4)) for i in range(0, len(vals), 8)]


def xyzz_mismatch(group, got, want):
    """None if the raw XYZZ `got` is the affine point `want` (None = infinity) with every coordinate component in
    [0, 2p), else why not"""
    F = curve_field(group)
    if any(not 0 <= c < 2 * Q for v in got for c in coord_ints(v)):
        return "coordinate out of [0, 2p)"
    x, y, zz, zzz = (from_mont(v) for v in got)
    if want is None:
        return None if F.is_zero(zz) else "not infinity"
    if F.is_zero(zz):
        return "infinity"
    if not F.eq(F.mul(F.sqr(zz), zz), F.sqr(zzz)):
        return "ZZ^3 != ZZZ^2"
    if not (F.eq(F.mul(x, F.inv(zz)), want[0]) and F.eq(F.mul(y, F.inv(zzz)), want[1])):
        return "wrong point"
    return None
