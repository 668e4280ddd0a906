"""secp256k1 recovery, Keccak-256 and Ethereum addresses on the device (zkpoa_ecdsa_star, zkpoa_keccak256,
zkpoa_eth_address) and the ecdsa-sigs-parser command, against tests/secp_ref.py. Every entry's every output and status
is compared; nothing is left out of a comparison."""
import hashlib
import json
import random
import subprocess

import pytest

import secp_limb_ref as lr
import secp_ref as sr
import sign_ref as sg
from test_secp_ref import fixture_text, sigs_bin  # noqa: F401  (sigs_bin is a fixture)

pytestmark = pytest.mark.gpu

N, P = sr.N, sr.P
ZEROS = (0, (0, 0), bytes(20))


def be(v):
    return int(v).to_bytes(32, "big")


def run(ctx, cases):
    """cases: (r, s, v, z, address20) -> [(status, r', (x, y), derived address)] from the device."""
    n = len(cases)
    rp, pk, ad, st = ctx.ecdsa_star(b"".join(be(c[0]) for c in cases), b"".join(be(c[1]) for c in cases),
                                    b"".join(be(c[3]) for c in cases), bytes(c[2] for c in cases),
                                    b"".join(c[4] for c in cases))
    assert (len(rp), len(pk), len(ad), len(st)) == (32 * n, 64 * n, 20 * n, n)
    ints = lambda b, i: int.from_bytes(b[32 * i:32 * i + 32], "big")
    return [(st[i], ints(rp, i), (ints(pk, 2 * i), ints(pk, 2 * i + 1)), ad[20 * i:20 * i + 20]) for i in range(n)]


def case_of(e, **change):
    c = dict(r=e["r"], s=e["s"], v=e["v"], z=e["z"], address=e["address"])
    c.update(change)
    return (c["r"], c["s"], c["v"], c["z"], c["address"])


def with_s(k, d, s):
    """A signature by key d with nonce k whose s is the one asked for (z follows from it)."""
    big_r = sr.mul(k, sr.G)
    r = big_r[0]
    z = (s * k - r * d) % N
    return (r, s, 27 + (big_r[1] & 1), z, sr.eth_address(sr.mul(d, sr.G)))


def first_non_residue():
    r = 1
    while sr.lift_x(r, False) is not None:
        r += 1
    return r


def on_curve_from(x):
    while sr.lift_x(x, False) is None:
        x += 1
    return x


def edge_cases():
    rng = random.Random(11)
    d, k = rng.randrange(1, N), rng.randrange(1, N)
    good = sr.sign(k, d, rng.getrandbits(256))
    big_r = sr.mul(k, sr.G)
    s_inf = rng.randrange(1, 1 << 255)
    cases = {
        "k=1": case_of(sr.sign(1, d, rng.getrandbits(256))),
        "k=n-1": case_of(sr.sign(N - 1, d, rng.getrandbits(256))),
        "k=2": case_of(sr.sign(2, d, rng.getrandbits(256))),
        "z=0": case_of(sr.sign(k, d, 0)),
        "z>=n": case_of(sr.sign(k, d, N + 5)),
        "z=2^256-1": case_of(sr.sign(k, d, (1 << 256) - 1)),
        "s=1": with_s(k, d, 1),
        "s=2^255-1": with_s(k, d, (1 << 255) - 1),
        "s=2^255": with_s(k, d, 1 << 255),
        "s=n-1": with_s(k, d, N - 1),
        "r=0": case_of(good, r=0),
        "r=n": case_of(good, r=N),
        "s=0": case_of(good, s=0),
        "s=n": case_of(good, s=N),
        "r non-residue": case_of(good, r=first_non_residue()),
        "r=p-1": case_of(good, r=P - 1),
        "r=p-1-n": case_of(good, r=P - 1 - N),
        "infinity": (big_r[0], s_inf, 27 + (big_r[1] & 1), s_inf * k % N, good["address"]),
        "address": case_of(good, address=bytes([good["address"][0] ^ 1]) + good["address"][1:]),
        "address last byte": case_of(good, address=good["address"][:19] + bytes([good["address"][19] ^ 0x80])),
        "d=1": case_of(sr.sign(k, 1, rng.getrandbits(256))),
        "d=n-1": case_of(sr.sign(k, N - 1, rng.getrandbits(256))),
    }
    for v in (0, 1, 26, 29):
        cases["v=%d" % v] = case_of(good, v=v)
    # Limbs at the 2^32-word borders. A recovered key with a zero or all-ones limb cannot be found by filtering
    # generated keys (2^-27 per key); the carry chains of the folds are driven through the operands instead: any r
    # that is an x coordinate, with any s and z, recovers some key, which the restatement computes as well.
    ones, alt = (1 << 256) - 1, int("ffffffff00000000" * 4, 16)
    patterns = [alt >> 1, (alt >> 33), 1 << 32, (1 << 224) - 1, ((1 << 255) - 1) ^ ((1 << 64) - 1) << 96, (1 << 128) + (1 << 32) - 1,
                N - (1 << 32), (1 << 32) + 977, ones >> 2]
    for i, pat in enumerate(patterns):
        r = on_curve_from(pat % N)
        s = patterns[(i + 3) % len(patterns)] % (1 << 255) or 1
        z = patterns[(i + 5) % len(patterns)] | (1 << 255 if i % 2 else 0)
        cases["limbs %d" % i] = (r, s, 27 + i % 2, z, bytes(20))
    return cases


EDGES = edge_cases()
EXPECTED_STATUS = {"s=2^255": sr.HIGH_S, "s=n-1": sr.HIGH_S, "r=0": sr.BAD_SCALAR, "r=n": sr.BAD_SCALAR, "s=0": sr.BAD_SCALAR,
                   "s=n": sr.BAD_SCALAR, "r non-residue": sr.NOT_ON_CURVE, "r=p-1": sr.BAD_SCALAR, "infinity": sr.INFINITY,
                   "address": sr.ADDRESS, "address last byte": sr.ADDRESS, "v=0": sr.BAD_V, "v=1": sr.BAD_V, "v=26": sr.BAD_V,
                   "v=29": sr.BAD_V}


def test_edges(ctx):
    names = list(EDGES)
    cases = []
    want = []
    for name in names:
        r, s, v, z, addr = EDGES[name]
        exp = sr.recover(r, s, v, z, addr)
        if name.startswith("limbs") or name == "r=p-1-n":   # no address is known beforehand: hand in the one derived
            if exp[0] == sr.ADDRESS:
                addr = exp[3]
                exp = (sr.OK,) + exp[1:]
        elif name in EXPECTED_STATUS:
            assert exp[0] == EXPECTED_STATUS[name], name
        else:
            assert exp[0] == sr.OK, name
        if exp[0] in (sr.BAD_V, sr.BAD_SCALAR, sr.HIGH_S, sr.NOT_ON_CURVE, sr.INFINITY):
            assert exp[1:] == ZEROS
        cases.append((r, s, v, z, addr))
        want.append(exp)
    assert sum(w[0] == sr.OK for w in want) >= 15
    got = run(ctx, cases)
    for name, g, w in zip(names, got, want):
        assert g == w, name
    # each case alone as well: a batch of one lane, and no neighbour to lean on
    for name in ("k=1", "k=n-1", "infinity", "z>=n"):
        i = names.index(name)
        assert run(ctx, [cases[i]]) == [want[i]], name


def test_steered_inner_scalars(ctx):
    """The scalars inside a recovery, u2 = s / r and u1 = -z / r, are random whatever r, s and z are; here they are
    chosen (tests/secp_limb_ref.py: s = u2 r, z = -u1 r, R = k G for small and large k): both at the borders of the
    signed recoding and of the halving, with R among the entries of the ladder's shared table of G, so that its additions
    double, cancel and pass through infinity. Combinations whose s is 0 or not below 2^255 must be refused as such."""
    steered = lr.steered_recoveries()
    want = [exp for _, _, exp in steered]
    statuses = [w[0] for w in want]
    assert statuses.count(sr.OK) >= 60 and {sr.BAD_SCALAR, sr.HIGH_S, sr.INFINITY} <= set(statuses)
    assert set(statuses) <= {sr.OK, sr.BAD_SCALAR, sr.HIGH_S, sr.INFINITY}
    for (_, (r, s, v, z, _), _), w in zip(steered, want):
        assert w[0] == (sr.BAD_SCALAR if s == 0 else sr.HIGH_S if s >= 1 << 255 else w[0])
        if w[0] != sr.OK:
            assert w[1:] == ZEROS
    got = run(ctx, [c for _, c, _ in steered])
    bad = [name for (name, _, _), g, w in zip(steered, got, want) if g != w]
    assert bad[:10] == []


@pytest.fixture(scope="module")
def pool():
    """4099 generated signatures with known answers, every fifth one spoilt in a known way: (cases, expected)."""
    entries = sr.generate(4099, seed=21)
    cases, want = [], []
    for i, e in enumerate(entries):
        ok = (sr.OK, e["rprime"], e["pub"], e["address"])
        kind = (i // 5) % 5 if i % 5 == 2 else -1
        if kind == 0:
            cases.append(case_of(e, v=e["v"] + 2))
            want.append((sr.BAD_V,) + ZEROS)
        elif kind == 1:
            cases.append(case_of(e, s=N - e["s"], v=55 - e["v"]))   # the high twin of a low s
            want.append((sr.HIGH_S,) + ZEROS)
        elif kind == 2:
            cases.append(case_of(e, r=0))
            want.append((sr.BAD_SCALAR,) + ZEROS)
        elif kind == 3:
            wrong = bytes([e["address"][7] ^ 0x10 if j == 7 else b for j, b in enumerate(e["address"])])
            cases.append(case_of(e, address=wrong))
            want.append((sr.ADDRESS,) + ok[1:])
        elif kind == 4:
            cases.append(case_of(e, s=N))
            want.append((sr.BAD_SCALAR,) + ZEROS)
        else:
            cases.append(case_of(e))
            want.append(ok)
    return entries, cases, want


def test_pool_is_what_recover_says(pool):
    """The expectations of the batch tests, spot-checked against the restatement's recovery (no device)."""
    _, cases, want = pool
    for i in list(range(0, 40)) + [4098]:
        r, s, v, z, addr = cases[i]
        assert sr.recover(r, s, v, z, addr) == want[i], i


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4099])
def test_batch_shapes(ctx, pool, n):
    _, cases, want = pool
    got = run(ctx, cases[:n])
    assert len(got) == n
    bad = [i for i in range(n) if got[i] != want[i]]
    assert bad == []


def test_reference_vector_on_the_device(ctx):
    (entry,) = json.loads(fixture_text("signatures_1.json"))
    want = json.loads(fixture_text("layer_one_input.json"))
    sig = entry["signature"]
    given = bytes.fromhex(entry["address"][2:])
    ((status, rprime, pub, addr),) = run(ctx, [(int(sig["r"], 16), int(sig["s"], 16), sig["v"], int(sig["msghash"], 16), given)])
    assert status == 0 and addr == given
    assert sr.limbs64(rprime) == want["rprime"][0]
    assert [sr.limbs64(pub[0]), sr.limbs64(pub[1])] == want["pubkey"][0]


@pytest.mark.parametrize("length", [0, 1, 40, 64, 135, 136, 137, 272])
def test_keccak256(ctx, length):
    rng = random.Random(length)
    msgs = [bytes(rng.randrange(256) for _ in range(length)) for _ in range(130)]
    got = ctx.keccak256(b"".join(msgs) if length else 130, length)
    assert len(got) == 32 * 130
    for i, m in enumerate(msgs):
        assert got[32 * i:32 * i + 32] == sr.keccak256(m), i
    if length == 0:
        assert got[:32].hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"


def test_keccak256_refuses_long_messages(zk, ctx):
    with pytest.raises(zk.ZkpoaError):
        ctx.keccak256(bytes(4097), 4097)
    assert ctx.keccak256(bytes(4096), 4096) == sr.keccak256(bytes(4096))


def test_eth_address(ctx, pool):
    entries = pool[0][:257]
    addr, text = ctx.eth_address(b"".join(be(e["pub"][0]) + be(e["pub"][1]) for e in entries))
    assert addr == b"".join(e["address"] for e in entries)
    assert text == [sr.checksum(e["address"]) for e in entries]
    v = json.loads(fixture_text("layer_one_input.json"))["pubkey"][0]
    x, y = (sum(int(l) << (64 * i) for i, l in enumerate(c)) for c in v)
    assert ctx.eth_address(be(x) + be(y))[1] == ["0x668e97bfD9851AF354C0508D6C180dDc68244826"]
    assert ctx.eth_address(b"") == (b"", [])


# ---- the executable -----------------------------------------------------------------------------------------------------
def parse(sigs_bin, tmp_path, text, long_options=True):
    src, out = tmp_path / "signatures.json", tmp_path / "parsed.json"
    src.write_text(text)
    argv = [sigs_bin, "--signatures", str(src), "--output-path", str(out)] if long_options else [sigs_bin, "-s", str(src), "-o", str(out)]
    return subprocess.run(argv, capture_output=True, text=True, timeout=120), out


def test_command_on_the_reference_vector(sigs_bin, tmp_path):
    text = fixture_text("signatures_1.json")
    rc, out = parse(sigs_bin, tmp_path, text)
    assert rc.returncode == 0, rc.stderr
    assert out.read_text() == sr.parser_output_text(text)
    assert rc.stdout.splitlines() == ["Parsing 1 ECDSA signatures..",
                                      "Successfully parsed ECDSA signatures and converted them to ECDSA* signatures"]
    l1 = tmp_path / "layer_one_input.json"
    rc = subprocess.run([sigs_bin, "layer-one-input", "-i", str(out), "-o", str(l1)], capture_output=True, text=True, timeout=120)
    assert rc.returncode == 0, rc.stderr
    assert l1.read_text() == fixture_text("layer_one_input.json")


def test_command_on_a_generated_file(sigs_bin, tmp_path, pool):
    entries = pool[0][:300]
    text = sr.signatures_json(entries)
    rc, out = parse(sigs_bin, tmp_path, text, long_options=False)
    assert rc.returncode == 0, rc.stderr
    assert out.read_text() == sr.parser_output_text(text, known=entries)
    assert rc.stdout.splitlines()[0] == "Parsing 300 ECDSA signatures.."


@pytest.mark.parametrize("what", ["address", "lower case", "v", "s"])
def test_command_stops_at_a_bad_entry(sigs_bin, tmp_path, pool, what):
    entries = pool[0][:40]
    doc = json.loads(sr.signatures_json(entries))
    given = doc[17]["address"]
    if what == "address":
        flip = "1" if given[9] != "1" else "2"
        doc[17]["address"] = given[:9] + flip + given[10:]
    elif what == "lower case":   # the reference compares with the EIP-55 text: an all-lower-case address differs
        doc[17]["address"] = given.lower()
        assert doc[17]["address"] != given
    elif what == "v":
        doc[17]["signature"]["v"] = 29
    else:
        doc[17]["signature"]["s"] = sr.hex32(N - entries[17]["s"])
    rc, out = parse(sigs_bin, tmp_path, json.dumps(doc))
    assert rc.returncode == 1
    lines = rc.stderr.strip().splitlines()
    assert len(lines) == 1 and "entry 17:" in lines[0]
    if what in ("address", "lower case"):
        assert doc[17]["address"] in lines[0] and given in lines[0]
    assert not out.exists()
    assert list(tmp_path.iterdir()) == [tmp_path / "signatures.json"]


def test_command_on_no_signatures(sigs_bin, tmp_path):
    rc, out = parse(sigs_bin, tmp_path, "[]")
    assert rc.returncode == 0, rc.stderr
    assert out.read_text() == '{\n  "accountAttestations": []\n}'


def test_commands_across_a_round_of_the_writer(sigs_bin, tmp_path):
    """65537 entries: the writers of both commands begin a second round of 2^16 for the last one. The parser derives
    every address again from its signature and refuses a mismatch, so its exit status checks all of the sign file."""
    n = (1 << 16) + 1
    sigs, parsed = tmp_path / "signatures.json", tmp_path / "parsed.json"
    for argv in ([sigs_bin, "sign", "--generate-keys", str(n), "--seed", "round", "--message", "m", "--output-path", str(sigs)],
                 [sigs_bin, "--signatures", str(sigs), "--output-path", str(parsed)]):
        rc = subprocess.run(argv, capture_output=True, text=True, timeout=120)
        assert rc.returncode == 0, rc.stderr
    given, got = json.loads(sigs.read_text()), json.loads(parsed.read_text())["accountAttestations"]
    assert len(given) == n and len(got) == n
    for i in (n - 2, n - 1):
        assert [int(got[i]["signature"][k]["__bigint__"]) for k in "rs"] == [int(given[i]["signature"][k], 16) for k in "rs"], i


def test_second_launch_of_one_lane(ctx):
    """2^18 + 1 signatures made by zkpoa_ecdsa_sign: the recovery's second launch holds the last one alone."""
    n = (1 << 18) + 1
    seed, h = b"slab", hashlib.sha256(b"slab").digest()
    keys = ctx.secp256k1_derive_keys(seed, 0, n)
    r, s, v, pk, ad, st = ctx.ecdsa_sign(keys, h, 0)
    assert st == bytes(n)
    rp, pk2, ad2, st2 = ctx.ecdsa_star(r, s, h * n, v, ad)
    assert st2 == bytes(n)
    assert pk2 == pk and ad2 == ad
    i, z = n - 1, int.from_bytes(h, "big")
    d = sg.derive_key(seed, i)
    assert keys[32 * i:] == be(d)
    want = sg.sign(d, z)
    assert (want["status"], be(want["r"]), be(want["s"]), want["v"]) == (0, r[32 * i:], s[32 * i:], v[i])
    assert sr.recover(want["r"], want["s"], want["v"], z, want["address"]) == \
        (sr.OK, int.from_bytes(rp[32 * i:], "big"), (int.from_bytes(pk2[64 * i:64 * i + 32], "big"), int.from_bytes(pk2[64 * i + 32:], "big")),
         ad2[20 * i:])
    assert want["pub"] == (int.from_bytes(pk[64 * i:64 * i + 32], "big"), int.from_bytes(pk[64 * i + 32:], "big")) and want["address"] == ad[20 * i:]
