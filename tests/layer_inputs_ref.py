"""Restatements, in Python big-ints, of what the layer-two / layer-three input steps and the Pedersen check compute:

  * circomlibjs `poseidon(inputs, initState, nOut)` at every width t = 2..17, with a Grain generator of its own (the
    oracle's fixes t = 3, R_P = 57), and the sponge scripts/input_prep_for_layer_two.ts:46-79 builds from it;
  * the ed25519 commitment of scripts/lib/pedersen_commitment.ts (extended coordinates, `pointAdd`, `pointEqual`),
    its 85-bit chunks and `formatScalarPower`.

Both are pinned by the reference's committed files (tests/golden/layer_inputs/) in tests/test_layer_inputs.py before
anything is compared with them.
"""
import functools

import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
R_F = 8
R_P = [56, 57, 56, 60, 60, 63, 64, 63, 60, 66, 60, 65, 70, 60, 64, 68]          # circomlib, t = 2..17


# ---- Grain LFSR (generate_parameters_grain.sage), 18 steps per Python operation ---------------------------------------
def _shrunk_bits(t, r_p, want):
    """The first `want` or more output bits of the self-shrinking generator seeded with (GF(p), x^5, 254, t, 8, r_p)."""
    seed = []
    for val, width in ((1, 2), (0, 4), (254, 12), (t, 12), (R_F, 10), (r_p, 10)):
        seed += [(val >> b) & 1 for b in range(width - 1, -1, -1)]
    seed += [1] * (80 - len(seed))
    s = sum(b << i for i, b in enumerate(seed))                                  # bit i = the i-th oldest bit
    blocks = (160 + 4 * want + 4096) // 18 + 1                                   # 4 raw bits per output bit on average
    while True:
        raw = np.empty(blocks, dtype=np.int64)
        x = s
        for k in range(blocks):                                                  # taps 62, 51, 38, 23, 13, 0: 18 new bits
            new = (x ^ (x >> 13) ^ (x >> 23) ^ (x >> 38) ^ (x >> 51) ^ (x >> 62)) & 0x3FFFF
            x = (x >> 18) | (new << 62)
            raw[k] = new
        bits = ((raw[:, None] >> np.arange(18)) & 1).astype(np.uint8).ravel()[160:]    # 160 steps are discarded
        bits = bits[:len(bits) // 2 * 2].reshape(-1, 2)
        out = bits[bits[:, 0] == 1, 1]                                           # a 0 discards the bit that follows it
        if len(out) >= want:
            return out
        blocks *= 2


@functools.lru_cache(maxsize=None)
def poseidon_params(t):
    """(round constants [(8 + R_P) * t], MDS matrix t x t) of circomlib's Poseidon of width t."""
    r_p = R_P[t - 2]
    n_const = (R_F + r_p) * t
    want = 254 * (2 * n_const + 8 * t + 64)
    while True:
        bits = _shrunk_bits(t, r_p, want)
        chunks = np.packbits(np.concatenate([np.zeros((len(bits) // 254, 2), np.uint8),
                                             bits[:len(bits) // 254 * 254].reshape(-1, 254)], axis=1), axis=1)
        vals = iter(int.from_bytes(row.tobytes(), "big") for row in chunks)
        try:
            C = []
            while len(C) < n_const:                                              # rejection sampling
                v = next(vals)
                if v < R:
                    C.append(v)
            while True:                                                          # Cauchy matrix over 2t reduced elements
                xy = [next(vals) % R for _ in range(2 * t)]
                if len(set(xy)) == 2 * t and all((xy[i] + xy[t + j]) % R for i in range(t) for j in range(t)):
                    break
            return C, [[pow(xy[i] + xy[t + j], R - 2, R) for j in range(t)] for i in range(t)]
        except StopIteration:
            want *= 2


def poseidon(inputs, init_state=0, n_out=1):
    """circomlibjs poseidon(inputs, initState, nOut) -> the first n_out state elements (a list)."""
    t = len(inputs) + 1
    assert 2 <= t <= 17 and 1 <= n_out <= t
    C, M = poseidon_params(t)
    r_p = R_P[t - 2]
    state = [init_state % R] + [x % R for x in inputs]
    for r in range(R_F + r_p):
        state = [(a + C[r * t + i]) % R for i, a in enumerate(state)]
        if r < R_F // 2 or r >= R_F // 2 + r_p:
            state = [pow(a, 5, R) for a in state]
        else:
            state[0] = pow(state[0], 5, R)
        state = [sum(M[i][j] * a for j, a in enumerate(state)) % R for i in range(t)]
    return state[:n_out]


def poseidon_sponge(inputs):
    """poseidonSponge of input_prep_for_layer_two.ts: 16 inputs per round, the previous round's state[0] as the initial
    state, state[1] of the last round -- whose inputs are read at i * lastRoundLength (:67, :71), not at i * 16."""
    n = len(inputs)
    assert n > 0
    rounds, last = n // 16, 16
    if n % 16:
        rounds, last = rounds + 1, n % 16
    h = 0
    for i in range(rounds):
        if i == rounds - 1:
            return poseidon(inputs[i * last:i * last + last], h, 2)[1]
        h = poseidon(inputs[i * 16:i * 16 + 16], h, 1)[0]


def x_limbs(x):
    return [(x >> (64 * k)) & (2 ** 64 - 1) for k in range(4)]


# ---- ed25519, as scripts/lib/pedersen_commitment.ts -------------------------------------------------------------------
P = 2 ** 255 - 19
D = 37095705934669439343138083508754565189542113879843219016388785533085940283555
GEN_G = (15112221349535400772501151409588531511454012693041857206046113283949847762202,
         46316835694926478169428394003475163141307993866256225615783033603165251855960,
         1,
         46827403850823179245072216630277197565144205554125654976674165829533817101731)
GEN_H = (33610936965734216034622052748864527785054979741013463956582067314415336407764,
         39037926758455103342491841394431773648115673280860795116462000885017926418697,
         44972472311651602601636560056538958210842501314939311016992875096561375476462,
         25285931357802837959040485138497351343220742265312934020814563180777586254493)


def point_add(p, q):
    a = (p[1] - p[0]) * (q[1] - q[0]) % P
    b = (p[1] + p[0]) * (q[1] + q[0]) % P
    c = 2 * p[3] * q[3] * D % P
    d = 2 * p[2] * q[2] % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f, g * h, f * g, e * h)


def point_mul(s, p):
    q = (0, 1, 1, 0)
    while s > 0:
        if s & 1:
            q = point_add(q, p)
        p = point_add(p, p)
        s >>= 1
    return q


def pedersen_commitment(secret, blinding):
    first = tuple(v % P for v in point_mul(secret, GEN_G))
    second = tuple(v % P for v in point_mul(blinding, GEN_H))
    return tuple(v % P for v in point_add(first, second))


def dechunk_to_point(signals):
    return tuple(sum(int(c) << (85 * k) for k, c in enumerate(signals[3 * i:3 * i + 3])) for i in range(4))


def point_equal(p, q):
    return (p[0] * q[2] - q[0] * p[2]) % P == 0 and (p[1] * q[2] - q[1] * p[2]) % P == 0


def chunks85(v):
    return [str((v >> (85 * k)) & (2 ** 85 - 1)) for k in range(3)]


def format_scalar_power(k):
    """formatScalarPower for k < 2^255: the bytes of k, least significant first, bit by bit, padded or cut to 255."""
    assert 0 <= k < 2 ** 255
    return [str((k >> i) & 1) for i in range(255)]
