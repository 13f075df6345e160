"""CPU checks of the hole filling (TwoViewStereo::filterInvalidPixels / weightedMedian): the restatement on hand-written
rows with the expected values written out, and the library's device header srh_filter.hpp compiled for the host against
the restatement's loop and std::make_heap / std::pop_heap."""
import numpy as np

import filter_ref as F
import oracle_ffi as O

inf, nan = np.inf, np.nan


def _row(vals, gap=2):
    return F.gap_fill(np.array([vals], dtype=np.float64), gap)[0]


def _eq(got, want):
    want = np.array(want, dtype=np.float64)
    assert F.same_bits(got, want), (got, want)


def test_runs_of_length_1_2_3():
    # length 1: the single pixel gets the right value; length 2: left | right; length 3 (end - start = 2): kept
    _eq(_row([1, inf, 2, inf, inf, 3, inf, inf, inf, 4]), [1, 2, 2, 2, 3, 3, inf, inf, inf, 4])


def test_runs_at_row_start_and_end():
    _eq(_row([inf, 5, 6]), [5, 5, 6])              # left value = pixel 0 itself (inf): takes the right one
    _eq(_row([inf, inf, 5]), [5, 5, 5])
    _eq(_row([5, 6, inf]), [5, 6, 6])              # right value NaN past the end: takes the left one
    _eq(_row([inf, inf]), [nan, nan])              # neither: NaN fill
    _eq(_row([inf]), [nan])


def test_nan_neighbours_and_nan_pixels():
    _eq(_row([nan, inf, 7]), [nan, 7, 7])
    _eq(_row([7, inf, nan, 1]), [7, 7, nan, 1])
    _eq(_row([nan, inf, nan]), [nan, nan, nan])
    _eq(_row([1, nan, 2]), [1, nan, 2])            # NaN is never gap-filled
    _eq(_row([1, -inf, 2]), [1, 2, 2])             # std::isinf: -inf too


def test_gap_width_0_and_5():
    _eq(_row([1, inf, 2], gap=0), [1, inf, 2])
    _eq(_row([1, inf, inf, inf, inf, inf, 2], gap=5), [1, 1, 1, 2, 2, 2, 2])
    _eq(_row([1, inf, inf, inf, inf, 2], gap=5), [1, 1, 1, 2, 2, 2])
    _eq(_row([1] + [inf] * 6 + [2], gap=5), [1] + [inf] * 6 + [2])


def _flat_window(R=1):
    ws = 2 * R + 1
    return np.full((ws, ws), nan), np.ones((ws, ws))


def test_median_with_one_kept_tap_is_nan():
    d, w = _flat_window()
    d[0, 0] = 3.0
    assert np.isnan(F.weighted_median(d, w, 1.0, 10.0))


def test_median_excludes_depths_outside_range():
    d, w = _flat_window()
    d[0, 0], d[0, 1] = 3.0, 20.0                   # 20 > max_depth: one kept tap
    assert np.isnan(F.weighted_median(d, w, 1.0, 10.0))
    d[0, 1] = 0.5                                  # < min_depth
    assert np.isnan(F.weighted_median(d, w, 1.0, 10.0))
    d[0, 1] = 4.0                                  # two equal weights: the larger pops first and ends the loop
    assert F.weighted_median(d, w, 1.0, 10.0) == 4.0
    d[0, 2] = 2.0                                  # 4 (1 < 2), 3 (2 >= 1): 3
    assert F.weighted_median(d, w, 1.0, 10.0) == 3.0
    w[0, 0] = 1e-11                                # a weight <= 1e-10 is not kept
    assert F.weighted_median(d, w, 1.0, 10.0) == 4.0


def test_median_on_a_map():
    # uniform image: every geodesic weight in the image is exp(0) = 1
    h, w = 5, 6
    rgba = np.full((h, w, 4), 100, np.uint8)
    mask = np.ones((h, w), np.uint8)
    mask[0, 0] = 0
    d = np.full((h, w), nan)
    d[2, 2], d[2, 3], d[3, 3] = 2.0, 3.0, 4.0
    d[4, 5] = inf
    op = O.params_twoview(min_depth=1.0, max_depth=10.0, window_radius=1)
    out = F.filter_map(rgba, mask, d, op, 2)
    assert np.isnan(out[0, 0])                     # mask not WHITE
    assert out[2, 2] == 2.0 and out[3, 3] == 4.0    # finite: kept
    assert out[3, 2] == 3.0                        # window holds 2, 3, 4
    assert np.isnan(out[1, 1])                     # one kept tap (2)
    assert out[1, 2] == 3.0                        # 2 and 3: the larger
    assert np.isnan(out[4, 5])                     # no kept tap


def test_library_gap_fill_matches_the_row_loop():
    rng = np.random.default_rng(7)
    for gap in (0, 1, 2, 3, 5, 40):
        d = rng.choice(np.array([1.0, 2.5, 3.0, inf, -inf, nan]), size=(40, 57), p=[.15, .15, .1, .45, .05, .1])
        assert F.same_bits(F.lib_gap_fill(d, gap), F.gap_fill(d, gap)), gap
    d = np.full((3, 9), inf)
    for gap in (2, 9, 10):
        assert F.same_bits(F.lib_gap_fill(d, gap), F.gap_fill(d, gap)), gap


def test_library_replay_matches_std_heap():
    assert F.lib().fr_heap_check(12345, 4000) == 0
