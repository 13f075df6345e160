"""tests/sgm_ref.py against itself: the window form (numpy, what the device tests use) and the direct O(L^2) form give the
same bits, and the properties the definition implies hold exactly."""
import numpy as np
import pytest

import sgm_ref as G
import twoview_mrf_cases as TC


def _vol(w, h, L, seed, integer=False):
    return TC.volume(w, h, L, seed=seed, integer=integer)


@pytest.mark.parametrize("smax", [0.5, 1.0, 2.0, 2.5, 4.0])
def test_window_form_and_direct_form_are_the_same_bits(smax):
    for (w, h, L), lam, integer in (((9, 7, 13), 0.25, False), ((5, 6, 4), 3.0, True), ((1, 4, 2), 1.0, False), ((6, 1, 7), 0.5, False),
                                    ((3, 3, 3), 0.0, False)):
        C, _ = _vol(w, h, L, seed=w + 10 * h + L, integer=integer)
        a = G.aggregate(C, lam, smax)
        b = G.aggregate_direct(C, lam, smax)
        tag = "%dx%dx%d smax %g lambda %g" % (w, h, L, smax, lam)
        for k in range(8):
            assert G.same_bits(a["paths"][k], b["paths"][k]), (tag, k)
        assert G.same_bits(a["S"], b["S"]) and np.array_equal(a["labels"], b["labels"]), tag
        assert np.isfinite(a["S"]).all()


def test_lambda_zero_sums_the_data_costs():
    """lambda = 0: M = g, L_r = C + 0 = C, so S is C added up popcount(mask) times.  On the integer volumes every partial
    sum is exact, whatever the count; on volumes rounded to float32 (29 spare bits) the sums of 4 and 8 terms are exact."""
    Ci, _ = _vol(9, 7, 13, seed=5, integer=True)
    for mask in (0x01, 0x0F, 0xA5, 0x7F, 0xFF):
        r = G.aggregate(Ci, 0.0, 2.0, mask)
        assert G.same_bits(r["S"], G.popcount(mask) * Ci), hex(mask)
        assert np.array_equal(r["labels"], np.argmin(Ci, axis=2))
    Cf, _ = _vol(9, 7, 13, seed=6)
    Cf = Cf.astype(np.float32).astype(np.float64)
    for mask in (0x0F, 0xFF):
        r = G.aggregate(Cf, 0.0, 2.0, mask)
        assert G.same_bits(r["S"], G.popcount(mask) * Cf), hex(mask)
        assert np.array_equal(r["labels"], np.argmin(Cf, axis=2))


def test_one_row_image():
    """h = 1: a direction with dy != 0 has no predecessor anywhere"""
    C, _ = _vol(11, 1, 9, seed=3)
    r = G.aggregate(C)
    for k in range(8):
        if G.DIRS[k][1] != 0:
            assert G.same_bits(r["paths"][k], C), k
        else:
            assert not G.same_bits(r["paths"][k], C), k


def test_mirror_in_x_swaps_directions():
    C, _ = _vol(9, 7, 13, seed=8)
    a = G.aggregate(C)
    b = G.aggregate(np.ascontiguousarray(C[:, ::-1]))
    for k, m in ((0, 1), (1, 0), (4, 7), (7, 4), (5, 6), (6, 5), (2, 2), (3, 3)):
        assert G.same_bits(b["paths"][k][:, ::-1], a["paths"][m]), (k, m)


def test_sum_of_single_directions_is_the_full_sum():
    C, _ = _vol(9, 7, 13, seed=9)
    full = G.aggregate(C)
    S = None
    for k in range(8):
        one = G.aggregate(C, mask=1 << k)
        assert G.same_bits(one["S"], full["paths"][k])
        S = one["S"].copy() if S is None else S + one["S"]
    assert G.same_bits(S, full["S"])


def test_changes_labels_and_has_exact_ties():
    """the default term regularises (labels differ from the per-pixel argmin) and the integer volume ties"""
    C, _ = _vol(33, 21, 64, seed=4, integer=True)
    r = G.aggregate(C)
    assert (r["labels"] != np.argmin(C, axis=2)).any()
    two = np.sort(r["S"], axis=2)[..., :2]
    assert (two[..., 0] == two[..., 1]).any()
    again = G.aggregate(C)
    assert G.same_bits(again["S"], r["S"]) and again["energy"] == r["energy"]
