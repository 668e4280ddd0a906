"""The reference of tests/test_gpu_ntt.py checked without a GPU: tests/ntt_ref.py's orderings, its odd-coset
reference against oracle/py/groth16.py's ifft -> shift -> fft, and the C oracle's transform against the closed forms
of the edge vectors (arithmetic, not the oracle against itself), so a wrong reference fails here and not only on
the GPU box."""
import random

import numpy as np
import pytest

import ntt_ref as nf
from oracle import c_oracle as co
from oracle.py import bn254 as bn
from oracle.py import groth16 as g16

R = nf.R


@pytest.mark.parametrize("k", [0, 1, 2, 5, 9])
def test_bitrev_perm_and_permute(k):
    n = 1 << k
    rev = nf.bitrev_perm(k)
    assert rev.tolist() == [int(format(i, "0%db" % k)[::-1], 2) if k else 0 for i in range(n)]
    x = nf.pack(range(100, 100 + n))
    y = nf.permute(x, k)
    assert nf.unpack(y) == [100 + int(r) for r in rev]
    assert nf.permute(y, k) == x
    assert (k < 2) == (y == x)


def test_uniform_bytes_is_canonical_and_spans_the_field():
    v = nf.unpack(nf.uniform_bytes(4000, 1))
    assert len(v) == 4000 and all(0 <= e < R for e in v)
    assert max(v) > R - (R >> 6) and min(v) < (R >> 6) and sum(e >= 1 << 253 for e in v) > 400
    assert nf.uniform_bytes(4000, 1) == nf.pack(v) and nf.uniform_bytes(4000, 2) != nf.pack(v)


@pytest.mark.parametrize("k", range(8))
def test_coset_ref_vs_py_oracle(k):
    rng = random.Random(k)
    x = [rng.randrange(R) for _ in range(1 << k)]
    assert nf.unpack(nf.coset_ref(nf.pack(x), k)) == g16.to_odd_coset(x)


@pytest.mark.parametrize("k", [0, 3, 6])
def test_scale_and_negate_index_identities(k):
    """the two identities that make a batch of different vectors out of one oracle transform"""
    n = 1 << k
    x = nf.uniform_bytes(n, 40 + k)
    s = 0x1234567 << 200
    assert nf.unpack(nf.scale(x, s)) == [v * s % R for v in nf.unpack(x)]
    xr = nf.negate_index(x, k)
    assert nf.unpack(xr) == [nf.unpack(x)[-i % n] for i in range(n)]
    for inverse in (False, True):
        X = co.ntt(x, k, inverse)
        assert co.ntt(nf.scale(x, s), k, inverse) == nf.scale(X, s)
        assert co.ntt(xr, k, inverse) == nf.negate_index(X, k)


def test_edge_vector_closed_forms_at_k5():
    k, n = 5, 32
    info = {}
    E = nf.edge_vectors(k, random.Random(5), info)
    c, m = info["c"], info["m"]
    assert m % 2 == 1 and 0 < m < n and 0 < c < R
    assert all(len(v) == 32 * n and all(e < R for e in nf.unpack(v)) for v in E.values())
    assert len(E) == 10 and len(set(E.values())) == 10
    assert min(nf.unpack(E["near_r"])) >= R - (1 << 200) and max(nf.unpack(E["uniform"])) > 1 << 252
    w = bn.fr_root_of_unity(k)
    ninv = pow(n, -1, R)

    def fwd(name):
        return nf.unpack(co.ntt(E[name], k))

    def inv(name):
        return nf.unpack(co.ntt(E[name], k, inverse=True))

    def single(at, v):
        return [v if j == at else 0 for j in range(n)]
    assert fwd("zero") == inv("zero") == [0] * n
    assert fwd("constant") == single(0, n * c % R) and inv("constant") == single(0, c)
    assert fwd("all_r_minus_1") == single(0, -n % R)
    for name, at in (("delta_0", 0), ("delta_mid", n // 2), ("delta_last", n - 1)):
        assert fwd(name) == [c * pow(w, at * j, R) % R for j in range(n)]
        assert inv(name) == [c * ninv * pow(w, -at * j, R) % R for j in range(n)]
    assert fwd("alternating") == single(n // 2, n * c % R) and inv("alternating") == single(n // 2, c)
    assert fwd("geometric") == single((n - m) % n, n * c % R) and inv("geometric") == single(m, c)
    # the oracle's transform is the naive sum
    assert fwd("uniform") == bn.ntt_naive(nf.unpack(E["uniform"]))
    assert inv("near_r") == bn.ntt_naive(nf.unpack(E["near_r"]), inverse=True)


@pytest.mark.parametrize("k", [0, 1])
def test_edge_vectors_smallest_sizes(k):
    E = nf.edge_vectors(k, random.Random(k))
    assert len(E) == 10 and all(len(v) == 32 << k for v in E.values())
    assert np.frombuffer(E["zero"], dtype=np.uint8).sum() == 0
