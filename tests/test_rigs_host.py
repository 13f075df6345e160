"""The rig table of tests/rig_cases.py is worth comparing with -- no GPU.

 * rig_is_row_aligned (srh_twoview_row_aligned) answers the table's `proposed` column, in both orders, and where it says yes
   its fx_bx is the other view's fx times the baseline;
 * the template scan's bound (srh_tscan_bound, host arithmetic) passes exactly the pixels of the table's `template` column;
 * the CPU oracle finds something on every rig: both directions, at r = 5 geodesic and r = 2 adaptive, evaluate candidates,
   leave a finite depth at half of the pixels or more, and on a proposed rig every winner lies on its reference pixel's row;
   on `cx_plus` winners lie on both sides of x.
The exact replay of the template scan's bound over these rigs is tests/test_tscan_bound_host.py."""
import numpy as np
import pytest

import cases
import oracle_ffi as O
import rig_cases as RC
from stereoreconstruction_amd import capi

W, H, D = 100, 24, 24
# a condition on the INPUTS (measured: 0.71 or better): a table change that breaks it changes the rig, not the floor
FINITE_SHARE = 0.5


@pytest.mark.parametrize("name", list(RC.RIGS))
def test_rig_test_answers_the_table(name):
    case = RC.rig_twoview(name, W, H, D)
    cams, p = cases.hip_inputs(case)
    ca, cb, unit, scale = RC.rig_cameras(name, W, H)
    base = np.linalg.norm(-ca[1].T @ ca[2] + cb[1].T @ cb[2])
    assert abs(base - unit) <= 1e-9 * unit
    for a, b in ((0, 1), (1, 0)):
        yes, fx_bx = capi.twoview_row_aligned(cams[a], cams[b])
        assert yes == RC.RIGS[name]["proposed"], (name, a, b)
        if yes:
            want = case["views"][b][2][0][0, 0] * base
            assert abs(fx_bx - want) <= 1e-9 * want, (name, a, b, fx_bx, want)


@pytest.mark.parametrize("name", RC.PROPOSED)
def test_the_bound_passes_the_pixels_the_table_says(name):
    """srh_tscan_bound at EVERY pixel against the template pixel of a band of all rows: the table's `template` column, which
    tests/test_gpu_rigs.py::test_tiers expects the device's tiers to follow (a tile goes by the bound when all its pixels pass)"""
    case = RC.rig_twoview(name, W, H, D)
    cams, p = cases.hip_inputs(case)
    tx, ty = W // 2, H // 2
    for ref, oth in ((0, 1), (1, 0)):
        passes = np.array([[capi.tscan_bound(cams[ref], cams[oth], p, (tx, ty), (x, y))["passes"] for x in range(W)] for y in range(H)], bool)
        print("%s %d>%d: the bound passes %d of %d pixels" % (case["name"], ref, oth, passes.sum(), passes.size))
        want = dict(all=np.ones((H, W), bool), none=np.zeros((H, W), bool), column=np.arange(W)[None, :].repeat(H, 0) == tx)
        assert np.array_equal(passes, want[RC.RIGS[name]["template"]]), (name, ref, oth, int(passes.sum()))


@pytest.mark.parametrize("radius,kind", [(5, 1), (2, 0)], ids=["r5_geodesic", "r2_adaptive"])
@pytest.mark.parametrize("name", list(RC.RIGS))
def test_the_oracle_finds_depths_on_every_rig(name, radius, kind):
    case = RC.rig_twoview(name, W, H, D, radius, kind)
    imgs, ocams, op = cases.oracle_inputs(case)
    rows = np.arange(H)[:, None]
    for ref, oth in ((0, 1), (1, 0)):
        depth, diag = O.twoview_wta(imgs[ref], imgs[oth], ocams[ref], ocams[oth], op, want_diag=True)
        share = np.isfinite(depth).mean()
        print("%s %d>%d: n_eval %d, finite share %.2f" % (case["name"], ref, oth, diag["n_eval"], share))
        assert diag["n_eval"] > 0 and share >= FINITE_SHARE, (name, ref, oth, diag["n_eval"], share)
        has = diag["win_xy"][..., 0] >= 0
        assert has.any()
        if RC.RIGS[name]["proposed"]:
            assert (diag["win_xy"][..., 1] == rows)[has].all(), (name, ref, oth)
        if name == "cx_plus":
            dx = (diag["win_xy"][..., 0] - np.arange(W)[None, :])[has]
            assert dx.min() < 0 < dx.max(), (name, ref, oth, dx.min(), dx.max())
