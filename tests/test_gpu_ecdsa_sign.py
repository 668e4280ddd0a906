"""Signing on the device (zkpoa_sha256_batch, zkpoa_secp256k1_pubkey, zkpoa_secp256k1_derive_keys, zkpoa_rfc6979_nonce,
zkpoa_ecdsa_sign) and the `sign` and `anon-set` modes of ecdsa-sigs-parser, against tests/sign_ref.py. Every output of
every lane is compared. The oracle's answers for the 4099-key pool are computed once and shared."""
import hashlib
import json
import random
import subprocess

import pytest

import secp_ref as sr
import sign_ref as sg
from test_secp_ref import sigs_bin  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

N = sr.N
be = sg.be32
ints = lambda b, i: int.from_bytes(b[32 * i:32 * i + 32], "big")


def device_sign(ctx, keys, hashes, stride=None):
    """keys, hashes: integers (hashes: one for all with stride 0, or one per key) -> [dict as sign_ref.sign gives]."""
    n = len(keys)
    if stride is None:
        stride = 32
    r, s, v, pk, ad, st = ctx.ecdsa_sign(b"".join(be(d) for d in keys), b"".join(be(z) for z in hashes), stride)
    assert (len(r), len(s), len(v), len(pk), len(ad), len(st)) == (32 * n, 32 * n, n, 64 * n, 20 * n, n)
    return [dict(status=st[i], r=ints(r, i), s=ints(s, i), v=v[i], pub=(ints(pk, 2 * i), ints(pk, 2 * i + 1)),
                 address=ad[20 * i:20 * i + 20]) for i in range(n)]


def device_pubkey(ctx, keys):
    n = len(keys)
    pk, ad, st = ctx.secp256k1_pubkey(b"".join(be(d) for d in keys))
    assert (len(pk), len(ad), len(st)) == (64 * n, 20 * n, n)
    return [dict(status=st[i], pub=(ints(pk, 2 * i), ints(pk, 2 * i + 1)), address=ad[20 * i:20 * i + 20]) for i in range(n)]


def want_sign(d, z, key=None):
    g = dict(sg.sign(d, z, key))
    g.pop("k", None)
    return g


@pytest.mark.parametrize("length", [0, 1, 55, 56, 63, 64, 65, 119, 120, 128])
def test_sha256(ctx, length):
    rng = random.Random(length)
    msgs = [bytes(rng.randrange(256) for _ in range(length)) for _ in range(300)]
    got = ctx.sha256(b"".join(msgs) if length else 300, length)
    assert len(got) == 32 * 300
    for i, m in enumerate(msgs):
        assert got[32 * i:32 * i + 32] == hashlib.sha256(m).digest(), i


def test_sha256_limits(zk, ctx):
    with pytest.raises(zk.ZkpoaError):
        ctx.sha256(bytes(4097), 4097)
    assert ctx.sha256(bytes(4096), 4096) == hashlib.sha256(bytes(4096)).digest()
    assert ctx.sha256(b"", 7) == b""


@pytest.mark.parametrize("skip", [0, 1, 2])
def test_rfc6979_nonce(ctx, skip):
    rng = random.Random(3)
    keys = [1, N - 1, rng.randrange(1, N)]
    hashes = [0, N - 1, N, N + 1, (1 << 256) - 1, rng.getrandbits(256)]
    pairs = [(d, z) for d in keys for z in hashes]
    got = ctx.rfc6979_nonce(b"".join(be(d) for d, _ in pairs), b"".join(be(z) for _, z in pairs), skip)
    assert len(got) == 32 * len(pairs)
    for i, (d, z) in enumerate(pairs):
        assert ints(got, i) == sg.nonce(d, z, skip), (hex(d), hex(z))


def test_rfc6979_nonce_arguments(zk, ctx):
    assert ctx.rfc6979_nonce(b"", b"") == b""
    with pytest.raises(zk.ZkpoaError):
        ctx.rfc6979_nonce(be(1), be(1), 65)


def test_edge_keys(ctx):
    rng = random.Random(7)
    pairs = [(d, z) for d in sg.edge_keys() for z in sg.edge_hashes(rng)]
    assert len(pairs) == 84
    got = device_sign(ctx, [d for d, _ in pairs], [z for _, z in pairs])
    for (d, z), g in zip(pairs, got):
        assert g == want_sign(d, z), (hex(d), hex(z))
    keys = sg.edge_keys()
    for d, g in zip(keys, device_pubkey(ctx, keys)):
        assert g == sg.public_key(d), hex(d)
    # each alone as well: a batch of one lane
    for d, z in (pairs[0], pairs[-1]):
        assert device_sign(ctx, [d], [z]) == [want_sign(d, z)]


def test_invalid_keys(ctx):
    keys = sg.INVALID_KEYS
    for g in device_sign(ctx, keys, [5] * len(keys)):
        assert g == sg.ZERO
    for g in device_pubkey(ctx, keys):
        assert g == dict(status=1, pub=(0, 0), address=bytes(20))


def test_public_vector(ctx):
    z = int.from_bytes(hashlib.sha256(b"Satoshi Nakamoto").digest(), "big")
    assert ints(ctx.rfc6979_nonce(be(1), be(z)), 0) == 0x8f8a276c19f4149656b280621e358cce24f5f52542772691ee69063b74f15d15
    (g,) = device_sign(ctx, [1], [z])
    assert (g["status"], g["r"], g["s"], g["v"]) == (0, 0x934b1ea10a4b3c1757e2b0c017d0b6143ce3c9a7e6a4a49860d7a6ab210ee3d8,
                                                     0x2442ce9d2b916064108014783e923ec36b49743e2ffa1c4496f01a512aafd9e5, 28)
    assert g["pub"] == sr.G


def test_stride_argument(zk, ctx):
    with pytest.raises(zk.ZkpoaError):
        ctx.ecdsa_sign(be(1), be(1), 16)
    with pytest.raises(zk.ZkpoaError):
        ctx.ecdsa_sign(be(1), be(1) * 2, 64)


@pytest.fixture(scope="module")
def pool():
    """4099 keys, invalid ones at 31 and 2049, with one hash each and one hash for all: (keys, hashes, common hash, the
    oracle's answers per key, the oracle's answers with the common hash)."""
    rng = random.Random(17)
    keys = [rng.randrange(1, N) for _ in range(4099)]
    keys[31], keys[2049] = 0, N
    hashes = [rng.getrandbits(256) for _ in keys]
    common = rng.getrandbits(256)
    pubs = [sg.public_key(d) for d in keys]
    each = [want_sign(d, z, p) for d, z, p in zip(keys, hashes, pubs)]
    same = [want_sign(d, common, p) for d, p in zip(keys, pubs)]
    return keys, hashes, common, each, same, pubs


@pytest.mark.parametrize("stride", [0, 32])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4099])
def test_batch_shapes(ctx, pool, n, stride):
    keys, hashes, common, each, same, pubs = pool
    got = device_sign(ctx, keys[:n], hashes[:n] if stride else [common], stride)
    want = (each if stride else same)[:n]
    assert len(got) == n
    assert [i for i in range(n) if got[i] != want[i]] == []
    if n > 31:
        assert got[31] == sg.ZERO and got[30]["status"] == 0 and got[32]["status"] == 0
    if n == 4099:
        assert device_pubkey(ctx, keys) == pubs


def test_derived_keys(ctx):
    for seed, first, n in ((b"", 0, 70), (b"seed", 250, 300), (bytes(range(60)), (1 << 40) - 3, 65)):
        got = ctx.secp256k1_derive_keys(seed, first, n)
        assert [ints(got, i) for i in range(n)] == [sg.derive_key(seed, first + i) for i in range(n)]
    assert ctx.secp256k1_derive_keys(b"x", 0, 0) == b""


def test_round_trip_through_recovery(ctx, pool):
    """257 signatures from zkpoa_ecdsa_sign go through zkpoa_ecdsa_star: all recover the signing key."""
    keys, hashes = pool[0][32:289], pool[1][32:289]
    r, s, v, pk, ad, st = ctx.ecdsa_sign(b"".join(be(d) for d in keys), b"".join(be(z) for z in hashes), 32)
    assert st == bytes(257)
    rp, pk2, ad2, st2 = ctx.ecdsa_star(r, s, b"".join(be(z) for z in hashes), v, ad)
    assert st2 == bytes(257) and pk2 == pk and ad2 == ad


def test_second_launch_of_one_lane(ctx):
    """2^20 + 1 keys: the second launch of zkpoa_ecdsa_sign and of zkpoa_secp256k1_pubkey holds the last one alone."""
    n = (1 << 20) + 1
    seed, h = b"slab", hashlib.sha256(b"slab").digest()
    keys = ctx.secp256k1_derive_keys(seed, 0, n)
    r, s, v, pk, ad, st = ctx.ecdsa_sign(keys, h, 0)
    assert st == bytes(n)
    assert ctx.secp256k1_pubkey(keys) == (pk, ad, bytes(n))
    rp, pk2, ad2, st2 = ctx.ecdsa_star(r, s, h * n, v, ad)
    assert st2 == bytes(n)
    assert pk2 == pk and ad2 == ad
    i = n - 1
    d = sg.derive_key(seed, i)
    assert keys[32 * i:] == be(d)
    assert dict(status=st[i], r=ints(r, i), s=ints(s, i), v=v[i], pub=(ints(pk, 2 * i), ints(pk, 2 * i + 1)), address=ad[20 * i:]) == \
        want_sign(d, int.from_bytes(h, "big"))


# ---- the commands ------------------------------------------------------------------------------------------------------
def run(argv):
    return subprocess.run([str(a) for a in argv], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def key_file():
    """65 keys over 70-odd lines: decimal and hex spellings, balances, comments, blank lines, stray blanks."""
    rng = random.Random(23)
    lines = ["# custody keys", ""]
    for i in range(65):
        d = rng.randrange(1, N) if i else 1
        spelling = [str(d), "0x%x" % d, "0X%064X" % d][i % 3]
        if i % 4 == 1:
            spelling += ",%d" % rng.randrange(10**30)
        elif i % 4 == 2:
            spelling = "  " + spelling + " , 0\r"
        lines.append(spelling)
        if i % 16 == 5:
            lines += ["", "# a comment, with a comma"]
    text = "\n".join(lines)          # the last line has no newline
    return text, sg.read_key_file(text)


def test_sign_command(sigs_bin, tmp_path, key_file):
    text, keys = key_file
    assert len(keys) == 65
    (tmp_path / "keys.txt").write_text(text, newline="")
    out = tmp_path / "signatures.json"
    for how, value, z in (("--message", "my message to sign", int.from_bytes(hashlib.sha256(b"my message to sign").digest(), "big")),
                          ("--msghash", sr.hex32((1 << 256) - 5), (1 << 256) - 5)):
        rc = run([sigs_bin, "sign", "--keys", tmp_path / "keys.txt", how, value, "--output-path", out])
        assert rc.returncode == 0, rc.stderr
        want = sg.sign_text(keys, z)
        assert out.read_text() == want
        parsed = tmp_path / "parsed.json"
        rc = run([sigs_bin, "--signatures", out, "--output-path", parsed])
        assert rc.returncode == 0, rc.stderr
        assert parsed.read_text() == sr.parser_output_text(want)
        assert sorted(p.name for p in tmp_path.iterdir()) == ["keys.txt", "parsed.json", "signatures.json"]


def test_sign_command_generates_keys(sigs_bin, tmp_path):
    out, keys_out, again = tmp_path / "signatures.json", tmp_path / "keys.txt", tmp_path / "again.json"
    rc = run([sigs_bin, "sign", "--generate-keys", 4099, "--seed", "rehearsal", "--message=hello", "-o", out, "--write-keys", keys_out])
    assert rc.returncode == 0, rc.stderr
    keys = [sg.derive_key(b"rehearsal", i) for i in range(4099)]
    assert keys_out.read_text() == sg.key_file_text(keys)
    z = int.from_bytes(hashlib.sha256(b"hello").digest(), "big")
    assert out.read_text() == sg.sign_text([(d, sg.default_balance(d)) for d in keys], z)
    rc = run([sigs_bin, "sign", "--keys", keys_out, "--message", "hello", "--output-path", again])
    assert rc.returncode == 0, rc.stderr
    assert again.read_bytes() == out.read_bytes()


@pytest.mark.parametrize("total", [32, 64, 300])
def test_anon_set_command(sigs_bin, tmp_path, key_file, total):
    text, keys = key_file
    keys = keys[:64]
    (tmp_path / "keys.txt").write_text("\n".join(text.split("\n")[:-1]) + "\n", newline="")
    assert sg.read_key_file((tmp_path / "keys.txt").read_text()) == keys
    out = tmp_path / "anonymity_set.csv"
    rc = run([sigs_bin, "anon-set", "--keys", tmp_path / "keys.txt", "--num-addresses", total, "--output-path", out])
    assert rc.returncode == 0, rc.stderr
    assert out.read_text() == sg.anon_set_text(keys, b"", total)
    # derived keys: the seed also names the filler accounts
    rc = run([sigs_bin, "anon-set", "--generate-keys", 64, "--seed", "s1", "-n", total, "-o", out])
    assert rc.returncode == 0, rc.stderr
    derived = [sg.derive_key(b"s1", i) for i in range(64)]
    assert out.read_text() == sg.anon_set_text([(d, sg.default_balance(d)) for d in derived], b"s1", total)


def test_chain_sign_parse_merkle(zk, sigs_bin, tmp_path):
    """sign -> the parsing mode -> merkle-tree on the anon-set file: the proofs list all 64 owned addresses."""
    sigs, parsed, csv, out = tmp_path / "signatures.json", tmp_path / "parsed.json", tmp_path / "anonymity_set.csv", tmp_path / "build"
    out.mkdir()
    source = ["--generate-keys", 64, "--seed", "chain"]
    for argv in ([sigs_bin, "sign"] + source + ["--message", "chain", "--output-path", sigs],
                 [sigs_bin, "--signatures", sigs, "--output-path", parsed],
                 [sigs_bin, "anon-set"] + source + ["--num-addresses", 300, "--output-path", csv],
                 [zk.MERKLE_BIN, "--anon-set", csv, "--poa-input-data", parsed, "--output-dir", out]):
        rc = run(argv)
        assert rc.returncode == 0, rc.stderr
    leaves = json.loads((out / "merkle_proofs.json").read_text())["leaves"]
    owned = sorted(int.from_bytes(sg.public_key(sg.derive_key(b"chain", i))["address"], "big") for i in range(64))
    assert [int(l["address"]["__bigint__"]) for l in leaves] == owned


@pytest.mark.parametrize("case", ["key 0", "key n", "malformed", "balance", "M=0", "both sources", "no source", "no output", "no message",
                                  "both messages", "seed without generate", "unknown option"])
def test_command_errors(sigs_bin, tmp_path, case):
    good = tmp_path / "good.txt"
    good.write_text("5\n6\n")
    bad = tmp_path / "bad.txt"
    out = tmp_path / "out.file"
    sign = [sigs_bin, "sign", "--message", "m", "--output-path", out]
    anon = [sigs_bin, "anon-set", "--num-addresses", "10", "--output-path", out]
    status, needle = 2, "Usage:"
    if case in ("key 0", "key n", "malformed", "balance"):
        bad.write_text("# first\n7\n" + {"key 0": "0x00", "key n": str(N), "malformed": "12x4", "balance": "9,1e3"}[case] + "\n8\n")
        status, needle = 1, "Error: key 3: "
        argvs = [sign + ["--keys", bad], anon + ["--keys", bad]]
    elif case == "M=0":
        argvs = [[sigs_bin, "anon-set", "--keys", good, "--num-addresses", "0", "--output-path", out]]
    elif case == "both sources":
        argvs = [sign + ["--keys", good, "--generate-keys", "3", "--seed", "s"], anon + ["--keys", good, "--generate-keys", "3", "--seed", "s"]]
    elif case == "no source":
        argvs = [sign, anon]
    elif case == "no output":
        argvs = [[sigs_bin, "sign", "--keys", good, "--message", "m"], [sigs_bin, "anon-set", "--keys", good, "--num-addresses", "4"],
                 [sigs_bin, "anon-set", "--keys", good, "--output-path", out]]
    elif case == "no message":
        argvs = [[sigs_bin, "sign", "--keys", good, "--output-path", out]]
    elif case == "both messages":
        argvs = [sign + ["--keys", good, "--msghash", sr.hex32(1)]]
    elif case == "seed without generate":
        argvs = [sign + ["--keys", good, "--seed", "s"], sign + ["--generate-keys", "3"]]
    else:
        argvs = [sign + ["--keys", good, "--frobnicate", "1"], sign + ["--keys", good, "--msghash"]]
    before = sorted(p.name for p in tmp_path.iterdir())
    for argv in argvs:
        rc = run(argv)
        assert rc.returncode == status, (argv, rc.stderr)
        lines = rc.stderr.strip().splitlines()
        if status == 1:
            assert len(lines) == 1 and lines[0].startswith(needle), rc.stderr
        else:
            assert lines[0].startswith("error: ") and needle in rc.stderr
        assert sorted(p.name for p in tmp_path.iterdir()) == before
