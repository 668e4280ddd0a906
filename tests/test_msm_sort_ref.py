"""tests/msm_sort_ref.py against itself and against small cases worked by hand. No GPU, none of the project's code."""
import numpy as np
import pytest

import msm_sort_ref as ref

R, HALF = ref.R, ref.HALF


@pytest.mark.parametrize("c", range(4, 26))
def test_recoding_of_the_edge_scalars(c):
    """for every width: the signed digits reassemble to the scalar mod r, no magnitude exceeds Nb, and nothing is carried
    out of the top window"""
    nb = 1 << (c - 1)
    edges = ref.edge_scalars(c)
    assert {0, 1, 2, R - 1, R - 2, HALF, HALF + 1, (1 << (3 * c)) - 1, 1 << 253, (1 << 253) - 1} <= set(edges)
    assert all(0 <= s < R for s in edges)
    for s in edges:
        digits, carry = ref.recode(s, c)
        assert len(digits) == ref.windows(c) and carry == 0, s
        assert all(0 <= mag <= nb and (mag or not sign) for mag, sign in digits), s
        assert ref.digits_value(digits, c) % R == s, s


@pytest.mark.parametrize("c", [4, 13, 22])
def test_the_wanted_edges_are_among_them(c):
    nb = 1 << (c - 1)
    # 2^(3c) - 1: the lowest digit 2^c - 1 becomes -1 and carries; the next two become 2^c, that is 0, and carry on
    digits, _ = ref.recode((1 << (3 * c)) - 1, c)
    assert digits[:4] == [(1, 1), (0, 0), (0, 0), (1, 0)]          # zero digits that carried in and out
    # all digits Nb: nothing carries; all digits Nb + 1: every digit carries, magnitudes Nb - 1 then Nb - 2 ...
    all_nb = sum(nb << (c * w) for w in range(3))
    assert ref.recode(all_nb, c)[0][:4] == [(nb, 0)] * 3 + [(0, 0)]
    all_nb1 = sum((nb + 1) << (c * w) for w in range(3))
    assert ref.recode(all_nb1, c)[0][:4] == [(nb - 1, 1), (nb - 2, 1), (nb - 2, 1), (1, 0)]
    edges = set(ref.edge_scalars(c))
    assert any(ref.recode(s, c)[0][:3] == [(nb, 0)] * 3 for s in edges)
    assert any(ref.recode(s, c)[0][:3] == [(nb - 1, 1), (nb - 2, 1), (nb - 2, 1)] for s in edges)


def test_normalisation_boundary():
    assert ref.normalise(HALF) == (HALF, 0) and ref.normalise(HALF + 1) == (HALF, 1)
    assert ref.normalise(R - 1) == (1, 1) and ref.normalise(0) == (0, 0)
    # r - 1 is -1: one entry, magnitude 1, negative, in the lowest window
    assert ref.recode(R - 1, 7)[0][0] == (1, 1) and not any(m for m, _ in ref.recode(R - 1, 7)[0][1:])


def test_entries_by_hand():
    """c = 4 (Nb = 8): 0x19 = digits 9, 1 -> (-7, carry), 2; r - 1 -> -1; 0 -> nothing; 8 -> +8 (the top bucket)"""
    scal = [0x19, R - 1, 0, 8]
    b, p = ref.entries(scal, 4, merged=False)
    assert sorted(zip(b.tolist(), p.tolist())) == sorted([(6, 0 | ref.SIGN), (8 + 1, 0), (0, 1 | ref.SIGN), (7, 3)])
    b, p = ref.entries(scal, 4, merged=True)
    assert sorted(zip(b.tolist(), p.tolist())) == sorted([(6, 0 | ref.SIGN), (1, 4 + 0), (0, 1 | ref.SIGN), (7, 3)])


def test_sort_result_by_hand():
    """five scalars equal to 1, one equal to r - 1, two equal to 3, piece length 4 at c = 4: bucket 0 holds 6 entries = a
    piece of 4 and one of 2, bucket 2 holds 2"""
    res = ref.sort_result([1] * 5 + [R - 1] + [3] * 2, 4, False, 4)
    assert res["W"] == 64 and res["TB"] == 64 * 8
    assert res["counts"][:4].tolist() == [6, 0, 2, 0] and res["counts"].sum() == 8
    assert res["off0"][:4].tolist() == [0, 6, 6, 8] and res["off0"][-1] == 8 and len(res["off0"]) == 513
    assert res["po_a"][:4].tolist() == [0, 2, 2, 3] and res["po_a"][-1] == 3
    assert (res["total_entries"], res["max_count"], res["total1"]) == (8, 6, 3)
    assert res["pbkt"].tolist() == [0, 0, 2] and res["piece_len"].tolist() == [4, 2, 2]
    assert res["len_hist"].tolist() == [0, 0, 2, 0, 1]
    assert res["keys"].tolist() == sorted([(0 << 32) | i for i in range(5)] + [(0 << 32) | 5 | ref.SIGN] +
                                          [(2 << 32) | 6, (2 << 32) | 7])
    empty = ref.sort_result([], 9, True, 32)
    assert empty["TB"] == 256 and empty["total1"] == 0 and empty["max_count"] == 0 and not empty["counts"].any()
    assert empty["len_hist"].tolist() == [0] * 33 and len(empty["keys"]) == 0 and len(empty["pbkt"]) == 0


def test_density_by_hand():
    d = ref.density([])
    assert d[0] == d[4] == 64.0 and d[25] == 11.0 and d[31] == 9.0
    d = ref.density([0, 1, R - 1, 1 << 32, HALF + 1])       # bit lengths 0, 1, 1, 33, 253
    assert d[4] == (0 + 1 + 1 + 9 + 64) / 5 and d[25] == (0 + 1 + 1 + 2 + 11) / 5 and d[3] == 64.0 and d[26] == 10.0
    assert HALF.bit_length() == 253
