"""The shape table of tests/small_shapes.py against the CPU oracle alone: every shape gives the reference something to
compute, the three classes of a depth map occur, and the groups the GPU tests rely on are not empty."""
import functools

import numpy as np

import cases
import oracle_ffi as O
import small_shapes as SS


@functools.lru_cache(maxsize=None)
def _oracle_twoview(shape, radius, kind):
    case = SS.small_twoview(*shape, radius, kind)
    imgs, ocams, op = cases.oracle_inputs(case)
    return [O.twoview_wta(imgs[r], imgs[o], ocams[r], ocams[o], op, want_diag=True) for r, o in ((0, 1), (1, 0))]


def test_every_twoview_shape_gives_the_oracle_work():
    classes = np.zeros(3, np.int64)
    for radius, kind in SS.TWOVIEW_KINDS:
        for shape in SS.TWOVIEW_SHAPES:
            for k, (depth, diag) in enumerate(_oracle_twoview(shape, radius, kind)):
                classes += [np.isfinite(depth).sum(), np.isposinf(depth).sum(), np.isnan(depth).sum()]
                if shape[0] >= 2:
                    assert np.isfinite(depth).any(), (shape, radius, k)
                    assert diag["n_eval"] > 0, (shape, radius, k)
    print("finite %d, +INF %d, NaN %d" % tuple(classes))
    assert (classes > 0).all()


def test_a_one_column_view_has_no_candidate_right_to_left():
    for radius, kind in SS.TWOVIEW_KINDS:
        for shape in ((1, 1, 2), (1, 9, 2)):
            depth, diag = _oracle_twoview(shape, radius, kind)[1]
            assert np.isnan(depth).all() and diag["n_eval"] == 0


def test_the_example_shape_of_the_table():
    depth, diag = _oracle_twoview((33, 9, 40), 5, 1)[0]
    assert (np.isfinite(depth).sum(), np.isposinf(depth).sum(), np.isnan(depth).sum()) == (255, 42, 0)
    assert diag["n_eval"] == 7857


def test_mvs_shapes_have_estimates_and_peaks():
    with_peaks = 0
    for shape in SS.MVS_SHAPES:
        case = SS.small_mvs(*shape, 1, False)
        imgs, ocams, op = cases.oracle_inputs(case)
        neigh = O.mvs_neighbours(ocams, op)
        every_view = True
        for v in range(3):
            depth, peaks, _ = O.mvs_initial_estimate(imgs, ocams, v, neigh[v], op, want_peaks=True)
            white = case["views"][v][1] == 1
            assert white.any(), (shape, v)
            assert np.isfinite(depth[white]).all(), (shape, v)
            every_view &= bool((peaks[..., 1] > 0).any())
        with_peaks += every_view
    print("%d of %d MVS shapes have a peak above zero in every view" % (with_peaks, len(SS.MVS_SHAPES)))
    assert with_peaks >= 6


def test_the_shape_groups_are_not_empty():
    assert any(D > w for w, h, D in SS.TWOVIEW_SHAPES)
    for radius, _ in SS.TWOVIEW_KINDS:
        for g in ("w<=2r", "h<=2r", "D>w", "tile edge"):
            assert any(g in SS.groups(s, radius) for s in SS.TWOVIEW_SHAPES), (radius, g)
    assert {w for w, _, _ in SS.TWOVIEW_SHAPES} >= set(SS.TILE_EDGE_WIDTHS)
