"""The Fr NTT (csrc/ntt.hip.h) at every pass plan, form and tile size, bit for bit against the C oracle.

zkpoa_ntt reaches the natural-order form only (DIF passes, the last one storing at the bit-reversed position);
zkpoa_ntt_form reaches the three the prover and the split chain run: plain DIF, plain DIT and the coset chain
DIF(w^-1) -> DIT(w) with the shift folded into the first DIT pass, each over a batch of vectors a stride apart.
References are tests/ntt_ref.py's (pinned on the CPU by tests/test_ntt_ref.py); oracle transforms are cached, so a
vector that several tests share is transformed once."""
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import ntt_ref as nf
from conftest import ROOT
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

S1, S2 = 0x9e3779b97f4a7c15 << 131 | 5, nf.R - 0xdeadbeef     # the scale factors that make a batch's vectors differ


# ---- shared inputs and oracle results --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _x(k):
    return nf.uniform_bytes(1 << k, 1000 + k)


@functools.lru_cache(maxsize=None)
def _y(k):
    return nf.uniform_bytes(1 << k, 2000 + k)


@functools.lru_cache(maxsize=None)
def _ntt(k, inverse):
    return co.ntt(_x(k), k, inverse)


@functools.lru_cache(maxsize=None)
def _unscaled(k, inverse):
    """the transform of _x(k) as ntt_dif / ntt_dit leave it: the oracle's 1/n of the inverse undone"""
    return nf.scale(_ntt(k, True), 1 << k) if inverse else _ntt(k, False)


@functools.lru_cache(maxsize=None)
def _coset(k):
    return nf.coset_ref(_x(k), k)


@functools.lru_cache(maxsize=None)
def _coset_batch(k):
    """three different vectors and their odd-coset images: x, a multiple of x and, while the oracle is cheap, an
    independent vector (above 2^16 another multiple: the chain is linear)"""
    x, cx = _x(k), _coset(k)
    if k <= 16:
        return (x, nf.scale(x, S1), _y(k)), (cx, nf.scale(cx, S1), nf.coset_ref(_y(k), k))
    return (x, nf.scale(x, S1), nf.scale(x, S2)), (cx, nf.scale(cx, S1), nf.scale(cx, S2))


@functools.lru_cache(maxsize=None)
def _edges(k):
    E = nf.edge_vectors(k, random.Random(300 + k))
    return {name: (v, co.ntt(v, k), co.ntt(v, k, inverse=True), nf.coset_ref(v, k)) for name, v in E.items()}


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_vectors():
    yield
    for f in (_x, _y, _ntt, _unscaled, _coset, _coset_batch, _edges):
        f.cache_clear()


def _same(got, want, what):
    """bit-exact, and on a mismatch the first differing element index (its rows and columns in the failing pass say
    which pass and stage)"""
    if got == want:
        return
    assert len(got) == len(want), "%s: %d bytes for %d" % (what, len(got), len(want))
    a = np.frombuffer(got, dtype=np.uint64).reshape(-1, 4)
    b = np.frombuffer(want, dtype=np.uint64).reshape(-1, 4)
    bad = np.flatnonzero((a != b).any(axis=1))
    i = int(bad[0])
    pytest.fail("%s: %d of %d elements differ, first at %d (%#x): got %s want %s"
                % (what, len(bad), len(a), i, i, got[32 * i:32 * i + 32].hex(), want[32 * i:32 * i + 32].hex()))


# ---- strided batches ------------------------------------------------------------------------------------------
def _marker(i, count):
    return bytes((0xA5 + 17 * i + j) & 0xFF for j in range(32 * count))


def _strided(vecs, n, stride):
    """the vectors `stride` elements apart, the elements between them filled with a marker pattern"""
    buf = bytearray()
    for i, v in enumerate(vecs):
        assert len(v) == 32 * n
        buf += v
        if i + 1 < len(vecs):
            buf += _marker(i, stride - n)
    return bytes(buf)


def _check_strided(got, wants, n, stride, what):
    assert len(got) == 32 * ((len(wants) - 1) * stride + n)
    for i, w in enumerate(wants):
        at = 32 * i * stride
        _same(got[at:at + 32 * n], w, "%s, vector %d of %d" % (what, i, len(wants)))
        if i + 1 < len(wants):
            assert got[at + 32 * n:at + 32 * stride] == _marker(i, stride - n), "%s: the gap after vector %d changed" % (what, i)


# ---- the natural-order form: every pass plan ------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("k", range(22))
def test_natural_every_plan(ctx, k, inverse):
    """One pass of B = 1..11 stages (k <= 11), then a strided second pass of B = k - 11 rows x 2^(22 - k) columns for
    every k = 12..21 (down to 2 columns), on input uniform over the whole of [0, r)."""
    _same(ctx.ntt(_x(k), k, inverse), _ntt(k, inverse), "zkpoa_ntt k=%d inverse=%d" % (k, inverse))


@pytest.mark.parametrize("inverse", [False, True])
def test_natural_2p22(ctx, inverse):
    """Three passes (11 + 6 + 5); the last boundary has no direct table (17 + 5 > 21): the two-level twiddle lookup."""
    _same(ctx.ntt(_x(22), 22, inverse), _ntt(22, inverse), "zkpoa_ntt k=22 inverse=%d" % inverse)


# ---- edge vectors --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 5, 11, 12, 16])
def test_edge_vectors(ctx, k):
    """Constant, delta, alternating, geometric, all r - 1, near-r and whole-range inputs: exact zeros (u - v with
    u == v must be stored as canonical 0), single non-zero outputs, the top of the range; through zkpoa_ntt in both
    directions and through the coset chain."""
    for name, (v, fwd, inv, coset) in _edges(k).items():
        _same(ctx.ntt(v, k), fwd, "%s k=%d forward" % (name, k))
        _same(ctx.ntt(v, k, inverse=True), inv, "%s k=%d inverse" % (name, k))
        _same(ctx.ntt_form(v, k, 2), coset, "%s k=%d to_odd_coset" % (name, k))


# ---- plain DIF / DIT -----------------------------------------------------------------------------------------
def _dif_dit(ctx, k, inverse):
    n = 1 << k
    x, X = _x(k), _unscaled(k, inverse)
    # three different vectors out of one oracle transform: x, a multiple of x, a multiple of x with negated indices
    vecs = [x, nf.scale(x, S1), nf.negate_index(nf.scale(x, S2), k)]
    wants = [X, nf.scale(X, S1), nf.negate_index(nf.scale(X, S2), k)]
    assert len(set(vecs)) == 3
    tag = "k=%d inverse=%d" % (k, inverse)
    _same(ctx.ntt_form(x, k, 0, inverse), nf.permute(X, k), "ntt_dif " + tag)
    _same(ctx.ntt_form(nf.permute(x, k), k, 1, inverse), X, "ntt_dit " + tag)
    got = ctx.ntt_form(_strided(vecs, n, n + 5), k, 0, inverse, batch=3, stride=n + 5)
    _check_strided(got, [nf.permute(w, k) for w in wants], n, n + 5, "ntt_dif batch 3 " + tag)
    got = ctx.ntt_form(_strided([nf.permute(v, k) for v in vecs], n, n + 5), k, 1, inverse, batch=3, stride=n + 5)
    _check_strided(got, wants, n, n + 5, "ntt_dit batch 3 " + tag)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("k", [0, 1, 3, 8, 11, 12, 14, 17, 21])
def test_dif_dit_forms(ctx, k, inverse):
    """ntt_dif = the oracle's transform in bit-reversed order, ntt_dit on bit-reversed input = the oracle's transform
    (no 1/n in either: the oracle's is undone by one oracle multiplication by n); alone and as a batch of three
    different vectors n + 5 elements apart whose gaps must come back unchanged."""
    _dif_dit(ctx, k, inverse)


def test_dit_2p22_tw_lookup(ctx):
    """The DIT boundary-twiddle load without a direct table (the third pass of 2^22)."""
    _same(ctx.ntt_form(nf.permute(_x(22), 22), 22, 1), _ntt(22, False), "ntt_dit k=22")


# ---- the coset chain --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2, 3, 8, 11, 12, 13, 16, 19])
def test_coset_form(ctx, k):
    """ntt_to_odd_coset as the prover calls it (batch = 3, grid.y striding), contiguous and n + 5 apart: the pre-scale
    index bitrev_k(p) into the two-level table with Lc = (k + 1) / 2 at odd and even k."""
    n = 1 << k
    vecs, wants = _coset_batch(k)
    assert len(set(vecs)) == 3
    for stride in (n, n + 5):
        got = ctx.ntt_form(_strided(vecs, n, stride), k, 2, batch=3, stride=stride)
        _check_strided(got, wants, n, stride, "to_odd_coset k=%d stride=n+%d" % (k, stride - n))


# ---- the forced tile size (read once per process) ------------------------------------------------------------
_CHILD_NATURAL = (1, 2, 3, 10, 11, 12, 15, 19, 20)
_CHILD_COSET = (11, 12, 20)
_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as entry
c = entry.load_package().Context(0)
src, dst = sys.argv[2], sys.argv[3]
def read(name):
    with open(src + "/" + name, "rb") as f:
        return f.read()
def write(name, data):
    with open(dst + "/" + name, "wb") as f:
        f.write(data)
for k in %r:
    x = read("x%%d" %% k)
    write("f%%d" %% k, c.ntt(x, k))
    write("i%%d" %% k, c.ntt(x, k, inverse=True))
for k in %r:
    write("c%%d" %% k, c.ntt_form(read("b%%d" %% k), k, 2, batch=3))
c.close()
""" % (_CHILD_NATURAL, _CHILD_COSET)


def test_forced_tile_in_a_child(ctx, tmp_path):
    """ZKPOA_NTT_TILE=10 (the 1024-element tile plan that k >= 23 takes by default: here k = 11 is a B = 1 second pass,
    k = 19 the 2-column pass, k = 20 the three-pass 10 + 5 + 5 plan of 2^26). It is read once per process: a fresh
    child, under a time limit of its own, its exit status checked. Its outputs equal the oracle's and, bit for bit,
    the default path's in this process."""
    want = {}
    for k in _CHILD_NATURAL:
        (tmp_path / ("x%d" % k)).write_bytes(_x(k))
        want["f%d" % k], want["i%d" % k] = _ntt(k, False), _ntt(k, True)
        _same(ctx.ntt(_x(k), k), want["f%d" % k], "default path k=%d forward" % k)
        _same(ctx.ntt(_x(k), k, inverse=True), want["i%d" % k], "default path k=%d inverse" % k)
    for k in _CHILD_COSET:
        vecs, wants = _coset_batch(k)
        (tmp_path / ("b%d" % k)).write_bytes(b"".join(vecs))
        want["c%d" % k] = b"".join(wants)
        _same(ctx.ntt_form(b"".join(vecs), k, 2, batch=3), want["c%d" % k], "default path k=%d to_odd_coset" % k)
    for tag, env in (("tile10", {"ZKPOA_NTT_TILE": "10"}),):
        out = tmp_path / tag
        out.mkdir()
        rc = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-s", "-c", _CHILD, ROOT, str(tmp_path), str(out)],
                            env=dict(os.environ, **env), capture_output=True, text=True)
        # 124 / 137 = the time limit, 134 / 139 = abort / fault, anything else non-zero = the library's error: stop here
        assert rc.returncode == 0, "%s: exit %d\n%s" % (tag, rc.returncode, rc.stderr[-2000:])
        for name, w in want.items():
            _same((out / name).read_bytes(), w, "%s %s" % (tag, name))


# ---- one engine, many sizes --------------------------------------------------------------------------------------
def test_interleaved_sizes_share_one_engine(zk):
    """A fresh context taken through k = 17, 12, 17, 22, 12: the table cache serves a size that comes back, and the
    natural form's grow-only scratch buffer grows (12 -> 17 -> 22) and is reused by the smaller sizes after it."""
    c = zk.Context(0)
    try:
        seen = {}
        for step, k in enumerate((17, 12, 17, 22, 12)):
            for inverse in (False, True):
                got = c.ntt(_x(k), k, inverse)
                _same(got, _ntt(k, inverse), "step %d k=%d inverse=%d" % (step, k, inverse))
                assert seen.setdefault((k, inverse), got) == got
    finally:
        c.close()


# ---- the hook's own argument checks --------------------------------------------------------------------------
def test_ntt_form_rejections(ctx, zk):
    data = _x(3) + _y(3)            # room for the two vectors of the stride case: only the library refuses it
    for what, args, kw in (("log_n > 28", (29, 0), {}), ("unknown form", (3, 3), {}), ("unknown form", (3, -1), {}),
                           ("batch == 0", (3, 0), {"batch": 0}), ("stride < n", (3, 0), {"batch": 2, "stride": 7})):
        with pytest.raises(zk.ZkpoaError, match=r"\): ntt_form: "):
            ctx.ntt_form(data, *args, **kw)
    _same(ctx.ntt(_x(3), 3), _ntt(3, False), "zkpoa_ntt after the rejections")
    _same(ctx.ntt_form(_x(3), 3, 2), _coset(3), "to_odd_coset after the rejections")
