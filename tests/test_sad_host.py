"""CPU checks of the SAD matching cost (TwoViewStereo::cost_sad): the restatement (tests/sad_restatement.cpp) against a
numpy statement on hand-built windows, the library's export of srh_twoview_pair_costs and its "cost" option, and a
subclass of the host class that calls the protected cost_sad, compiled without a device."""
import os
import subprocess

import numpy as np
import pytest

import oracle_ffi as O
import sad_ref as S
from stereoreconstruction_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "stereoreconstruction_amd", "host")
LIBDIR = os.path.join(ROOT, "stereoreconstruction_amd")


def _gray(rgb):
    r, g, b = (float(v) for v in rgb)
    return 0.11 * r + 0.59 * g + 0.3 * b                    # RGBA::toGray, as sro_to_gray


def _np_cost_sad(lrgba, lmask, rrgba, rmask, wts, op, x1, y1, x2, y2):
    """cost_sad in plain Python floats (IEEE double): sample() on the left, pixel() on the right."""
    R = op.window_radius
    h, w = lrgba.shape[:2]
    s, tw, n = 0.0, 0.0, 0
    for row in range(-R, R + 1):
        for col in range(-R, R + 1):
            xl, yl, xr, yr = x1 + col, y1 + row, x2 + col, y2 + row
            if not (0 <= xl < w and 0 <= yl < h and lmask[yl, xl] == 1):
                continue
            if not (0 <= xr < w and 0 <= yr < h and rmask[yr, xr] == 1):
                continue
            if not (xl + 1 < w and yl + 1 < h):                # sample() at integer coordinates
                continue
            wt = float(wts[row + R, col + R])
            if wt > op.weight_cutoff:
                d = abs(_gray(lrgba[yl, xl, :3]) - _gray(rrgba[yr, xr, :3]))
                s += wt * (d if d < op.max_color_diff else op.max_color_diff)
                tw += wt
                n += 1
    if n <= 4 or tw <= 1e-10:
        return op.bad_ret
    return s / tw


def _images(w=9, h=7, seed=3):
    rng = np.random.default_rng(seed)
    l = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    r = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    return l, r, np.ones((h, w), np.uint8), np.ones((h, w), np.uint8)


def _both(l, lm, r, rm, wts, op, x1, y1, x2, y2):
    got = S.cost_sad(O.OImage(l, lm), O.OImage(r, rm), wts, op, x1, y1, x2, y2)
    want = _np_cost_sad(l, lm, r, rm, wts, op, x1, y1, x2, y2)
    assert S.same_bits(np.float64(got), np.float64(want)), (got, want)
    return got


def test_difference_clamped_at_max_color_diff():
    l, r, lm, rm = _images()
    l[..., :3] = 255                                          # gray 255 against 0: |diff| = 255 > 120
    r[..., :3] = 0
    op = O.params_twoview(window_radius=1)
    wts = np.ones((3, 3))
    assert _both(l, lm, r, rm, wts, op, 3, 3, 4, 3) == 120.0
    r[..., :3] = 200                                          # |255 - 200| = 55 < 120: not clamped
    assert _both(l, lm, r, rm, wts, op, 3, 3, 4, 3) == pytest.approx(55.0, abs=1e-9)


def test_four_pixels_is_bad_ret_five_is_not():
    l, r, lm, rm = _images()
    op = O.params_twoview(window_radius=1)
    wts = np.ones((3, 3))
    x1, y1 = 3, 3
    lm[:] = 0
    lm[y1, x1 - 1:x1 + 2] = 1                                # 3 taps of the middle row
    lm[y1 - 1, x1] = 1                                       # + 1: numPixels == 4
    assert _both(l, lm, r, rm, wts, op, x1, y1, 4, 3) == op.bad_ret
    lm[y1 + 1, x1] = 1                                       # 5
    assert _both(l, lm, r, rm, wts, op, x1, y1, 4, 3) != op.bad_ret


def test_total_weight_at_most_1e10_is_bad_ret():
    l, r, lm, rm = _images()
    op = O.params_twoview(window_radius=1, weight_cutoff=1e-13)
    wts = np.full((3, 3), 1e-11)                             # 9 taps: 9e-11 <= 1e-10
    assert _both(l, lm, r, rm, wts, op, 3, 3, 4, 3) == op.bad_ret
    wts[:] = 2e-11                                           # 1.8e-10 > 1e-10
    assert _both(l, lm, r, rm, wts, op, 3, 3, 4, 3) != op.bad_ret
    op2 = O.params_twoview(window_radius=1)                  # the default cut-off 1e-10 drops every tap of 1e-11
    assert _both(l, lm, r, rm, np.full((3, 3), 1e-11), op2, 3, 3, 4, 3) == op2.bad_ret


def test_last_column_counts_on_the_right_not_on_the_left():
    w, h = 9, 7
    l, r, lm, rm = _images(w, h)
    op = O.params_twoview(window_radius=1)
    wts = np.arange(1.0, 10.0).reshape(3, 3)
    # right window on the last column: pixel() is valid there, so its taps count
    got = _both(l, lm, r, rm, wts, op, 3, 3, w - 2, 3)
    # the same costs without the right view's last column (its mask cleared) must differ
    rm2 = rm.copy()
    rm2[:, w - 1] = 0
    assert not S.same_bits(np.float64(got), np.float64(_both(l, lm, r, rm2, wts, op, 3, 3, w - 2, 3)))
    # left window on the last column: sample() is not valid there, the taps are skipped -- clearing the left mask of that
    # column changes nothing
    a = _both(l, lm, r, rm, wts, op, w - 2, 3, 3, 3)
    lm2 = lm.copy()
    lm2[:, w - 1] = 0
    assert S.same_bits(np.float64(a), np.float64(_both(l, lm2, r, rm, wts, op, w - 2, 3, 3, 3)))
    # ... and the same for the last row
    b = _both(l, lm, r, rm, wts, op, 3, h - 2, 3, h - 2)
    lm3 = lm.copy()
    lm3[h - 1, :] = 0
    assert S.same_bits(np.float64(b), np.float64(_both(l, lm3, r, rm, wts, op, 3, h - 2, 3, h - 2)))


def test_random_windows_match_numpy():
    rng = np.random.default_rng(11)
    for R in (1, 2, 5):
        w, h = 24, 19
        l, r, lm, rm = _images(w, h, seed=R)
        lm[rng.random((h, w)) < 0.15] = 0
        rm[rng.random((h, w)) < 0.15] = 0
        op = O.params_twoview(window_radius=R)
        for _ in range(60):
            wts = rng.random((2 * R + 1, 2 * R + 1))
            wts[rng.random(wts.shape) < 0.1] = 0.0
            x1, y1 = int(rng.integers(0, w)), int(rng.integers(0, h))
            x2, y2 = int(rng.integers(-2, w + 2)), int(rng.integers(-2, h + 2))
            _both(l, lm, r, rm, wts, op, x1, y1, x2, y2)


def test_library_exports_pair_costs_and_cost_constants():
    L = capi.lib()
    assert hasattr(L, "srh_twoview_pair_costs")
    assert "srh_twoview_pair_costs" in capi.EXPORTS
    assert (capi.COST_NCC, capi.COST_SAD) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "stereo_recon_hip.h")).read()
    assert "SRH_COST_SAD = 1" in hdr and '"cost"' in hdr


def test_host_subclass_calling_cost_sad_compiles_without_gpu(tmp_path):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "host_sad_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + HOST,
                           os.path.join(ROOT, "tests", "host_sad_test.cpp"),
                           os.path.join(HOST, "libstereo_recon_host.a"),
                           "-L" + LIBDIR, "-lstereo_recon_hip", "-Wl,-rpath," + LIBDIR, "-o", exe])
    assert os.path.exists(exe)
