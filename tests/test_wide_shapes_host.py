"""The table of tests/wide_shapes.py on the CPU oracle alone: what tests/test_gpu_wide_shapes.py compares the device with
is worth comparing with.  No GPU."""
import functools

import numpy as np
import pytest

import cases
import oracle_ffi as O
import wide_shapes as WS
from stereoreconstruction_amd import capi

DIRECTIONS = ((0, 1), (1, 0))


@functools.lru_cache(maxsize=None)
def _oracle(shape, general):
    """both directions at r = 2 adaptive (the candidates do not depend on the window): (case, [(depth, diag)] * 2)"""
    case = WS.wide_twoview(*shape, 2, 0, general=general)
    imgs, ocams, op = cases.oracle_inputs(case)
    return case, [WS.oracle_wta(O, imgs, ocams, op, r, o) for r, o in DIRECTIONS]


def test_the_limit_is_the_headers():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stereo_recon_hip.h")).read()
    assert re.search(r"#define\s+SRH_MAX_VIEW_DIM\s+32767\b", text)
    assert WS.M == capi.MAX_VIEW_DIM == 32767
    # the table reaches the limit in both directions, just past the powers of two on the way
    for k, powers in ((0, (2048, 4096, 8192, 16384)), (1, (2048, 8192, 16384))):
        sides = sorted(s[k] for s in WS.TWOVIEW_SHAPES)
        assert sides[-1] == WS.M
        for p2 in powers:
            assert any(p2 < v < 2 * p2 for v in sides), (k, p2)


@pytest.mark.parametrize("shape", WS.GENERAL_SHAPES, ids=WS.shape_id)
def test_general_rig_keeps_half_of_the_pixels(shape):
    """at least half of the reference pixels have a finite oracle depth, in both directions"""
    case, out = _oracle(shape, True)
    (Kl, Rl, tl), (Kr, Rr, tr) = case["views"][0][2], case["views"][1][2]
    assert np.abs(Rl - Rr).max() > 1e-9                                # (not a row-aligned rig: the dense plan declines it)
    for (ref, oth), (depth, diag) in zip(DIRECTIONS, out):
        share = np.isfinite(depth).mean()
        print("%s %d>%d: finite %d of %d (%.2f), n_eval %d" % (case["name"], ref, oth, np.isfinite(depth).sum(), depth.size, share, diag["n_eval"]))
        assert share >= 0.5, (case["name"], ref, oth, share)


@pytest.mark.parametrize("shape", WS.TWOVIEW_SHAPES, ids=WS.shape_id)
def test_rectified_shapes_have_candidates_both_ways(shape):
    case, out = _oracle(shape, False)
    for (ref, oth), (depth, diag) in zip(DIRECTIONS, out):
        assert diag["n_eval"] > 0 and np.isfinite(depth).any(), (case["name"], ref, oth)


@pytest.mark.parametrize("general", [False, True], ids=["rectified", "general"])
@pytest.mark.parametrize("shape", WS.TWOVIEW_SHAPES, ids=WS.shape_id)
def test_first_and_last_pixel(shape, general):
    """the builder's arrays are h x w, the oracle's maps too, the first pixel is (0, 0) and the last (w - 1, h - 1), and
    winners lie inside the other view up to its last column and row"""
    if general and shape not in WS.GENERAL_SHAPES:
        return
    w, h, D = shape
    case, out = _oracle(shape, general)
    for rgba, mask, _, _, _ in case["views"]:
        assert rgba.shape == (h, w, 4) and mask.shape == (h, w)
    imgs, _, op = cases.oracle_inputs(case)
    assert all((im.w, im.h) == (w, h) for im in imgs) and op.num_depth_levels == D
    ref_x, ref_y, win_x, win_y = [], [], [], []
    for depth, diag in out:
        assert depth.shape == (h, w) and diag["win_xy"].shape == (h, w, 2)
        ys, xs = np.nonzero(diag["win_xy"][..., 0] >= 0)
        win = diag["win_xy"][ys, xs]
        assert win[:, 0].min() >= 0 and win[:, 0].max() <= w - 1 and win[:, 1].min() >= 0 and win[:, 1].max() <= h - 1
        ref_x.append(xs); ref_y.append(ys); win_x.append(win[:, 0]); win_y.append(win[:, 1])
    # reference pixels with a winner, and the winners themselves: from the first row and column to the last (over the two
    # directions: left to right the first column of a rectified pair has no candidate, right to left the last has none)
    for v, last in ((ref_x, w - 1), (ref_y, h - 1), (win_x, w - 1), (win_y, h - 1)):
        v = np.concatenate(v)
        assert v.min() == 0 and v.max() == last, (case["name"], v.min(), v.max(), last)
