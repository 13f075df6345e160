"""The override table of tests/constants_cases.py on the CPU oracle alone: every entry moves what its witness says it
moves, by at least the minimum share, so that the device test of the same entry (tests/test_gpu_constants.py) is not
vacuous; the share written next to the entry is the one measured here.  Branch entries are checked on the kernels'
`sdiv` predicate, the hole filling's premise on its own."""
import math

import numpy as np
import pytest

import constants_cases as CC

# the literal next to an entry is the measured share to this many points (the oracle is deterministic; libm's exp may
# move a tie on another machine)
LITERAL_TOL = 0.015


@pytest.mark.parametrize("e", [e for e in CC.ENTRIES + CC.SAD_ENTRIES if e.witness != "branch"], ids=CC.entry_id)
def test_the_override_moves_its_witness_on_the_oracle(e):
    share = CC.measured_share(e)
    print("%s: witness %s, share %.4f (table: %.3f)" % (CC.entry_id(e), e.witness, share, e.share))
    assert share >= CC.MIN_SHARE, "%s moves %.2f %% of its witness: a vacuous case" % (CC.entry_id(e), 100 * share)
    assert abs(share - e.share) <= LITERAL_TOL, "%s: the table says %.3f, the oracle %.4f" % (CC.entry_id(e), e.share, share)


def test_values_that_move_nothing_stay_out_of_the_table():
    """measured on the oracle: geodesic_iters 5 is 3, bad_ret alone meets no candidate, max_color_diff >= 3 clamps nothing;
    peak_threshold 0.8 adds no peak on mvs_geodesic (every score is above 0.98) and 0.99 removes 0.2 % of the lists"""
    for case, witness, over in (("geodesic_rect", "depth", dict(geodesic_iters=5)), ("geodesic_rect", "depth", dict(bad_ret=2.0)),
                                ("geodesic_masks", "depth", dict(max_color_diff=3.0)), ("mvs_geodesic", "peaks", dict(peak_threshold=0.8))):
        assert CC.measured_share(CC._e(case, witness, 0.0, **over)) == 0.0, (case, over)
        assert not [e for e in CC.ENTRIES if e.case == case and dict(e.over) == over]
    assert CC.measured_share(CC._e("mvs_geodesic", "peaks", 0.0, peak_threshold=0.99)) < CC.MIN_SHARE
    # the SAD clamp is per tap: 40 grey levels clamp nothing that wins
    assert CC.measured_share(CC._e("geodesic_masks", "sad", 0.0, max_color_diff=40.0)) == 0.0


def test_peak_entries_move_no_depth_or_say_so():
    """peak_threshold 0.995 and top_k 3 leave view 0's depth map alone (the best peak stays): only the lists can tell"""
    d = CC.default_entry("mvs_geodesic")
    for e in CC.entries(witness="peaks"):
        moved = CC.depth_share(CC.oracle_mvs(e, 0)[0], CC.oracle_mvs(d, 0)[0])
        print("%s: depth share %.4f" % (CC.entry_id(e), moved))
        if dict(e.over).get("peak_threshold") != 0.9976:
            assert moved == 0.0, CC.entry_id(e)


def test_the_clamp_and_the_fill_meet_candidates():
    """what the table says about WHERE the constants act, on the oracle's winning costs: max_color_diff 0.3 is the
    runner-up's or the winner's cost at many pixels; bad_ret 0.02 is a winner's cost under weight_cutoff 0.7 and a common
    value among random pairs on masked views"""
    e = CC._e("geodesic_masks", "depth", 0.109, max_color_diff=0.3)
    _, diag = CC.oracle_twoview(e, 0)
    on_clamp = (diag["min_cost"] == 0.3) | (diag["second_cost"] == 0.3)
    print("max_color_diff 0.3: %.3f of the pixels have the clamp as winner's or runner-up's cost" % on_clamp.mean())
    assert on_clamp.mean() > 0.05
    # bad_ret: the winner's cost where every candidate's window is left without a tap above the cut-off ...
    e = CC._e("geodesic_rect", "depth", 0.742, weight_cutoff=0.7, bad_ret=0.02)
    assert e in CC.ENTRIES
    _, diag = CC.oracle_twoview(e, 0)
    fill = diag["min_cost"] == 0.02
    print("geodesic_rect bad_ret 0.02 / weight_cutoff 0.7: the winner's cost at %d pixels (%.4f)" % (fill.sum(), fill.mean()))
    assert fill.mean() > 0.005
    # ... and a common value among the costs of random pairs (srh_twoview_pair_costs, the label volume) on masked views
    import sad_ref as S
    for e in CC.entries(case=("geodesic_masks", "adaptive_masks"), has=("bad_ret",)):
        imgs, cams, p = CC.oracle_inputs(e)
        xy = CC.pairs(e)
        ncc = S.pair_costs_ncc(imgs[0], imgs[1], p, xy)
        sad = S.pair_costs_sad(imgs[0], imgs[1], p, xy)
        print("%s: bad_ret is %.3f of %d random NCC pair costs, %.3f of the SAD ones; %.3f of the NCC ones sit on the clamp" % (
            CC.entry_id(e), (ncc == p.bad_ret).mean(), len(xy), (sad == p.bad_ret).mean(), (ncc == p.max_color_diff).mean()))
        assert (ncc == p.bad_ret).mean() > 0.05 and (sad == p.bad_ret).mean() > 0.05
        assert ((ncc != p.bad_ret) & (ncc != p.max_color_diff)).mean() > 0.15        # (and enough ordinary costs next to it)


def test_branch_entries_switch_the_windows_kernels_branch():
    assert CC.sdiv({}), "the defaults take the shared-divisor branch"
    branch = CC.entries(witness="branch")
    assert len(branch) == 2
    for e in branch:
        assert not CC.sdiv(dict(e.over)), CC.entry_id(e)
    assert not CC.sdiv(dict(geodesic_sigma=-50.0)) and not CC.sdiv(dict(geodesic_init=-100.0)) and not CC.sdiv(dict(geodesic_init=0.0))
    # ... and every other geodesic entry of the table runs the fast branch with ANOTHER divisor or start value
    fast = [e for e in CC.entries(has=("geodesic_sigma", "geodesic_init")) if CC.sdiv(dict(e.over))]
    assert {dict(e.over).get("geodesic_sigma") for e in fast} >= {7.3, 400.0, 0.5, 1e6}
    assert any(dict(e.over).get("geodesic_init") == 30.0 for e in fast)
    # at sigma 5e-4 every weight but the centre's underflows to 0: every NCC cost is NaN -> the clamp
    e = CC._e("geodesic_rect", "branch", None, geodesic_sigma=5e-4)
    _, diag = CC.oracle_twoview(e, 0)
    seen = diag["min_cost"][np.isfinite(diag["min_cost"])]
    assert seen.size and np.isin(seen, (120.0, 1000.0)).all() and (seen == 120.0).mean() > 0.9


def test_the_medians_premise():
    assert CC.median_premise({}) and CC.median_premise(dict(geodesic_sigma=7.3)) and CC.median_premise(dict(geodesic_iters=1))
    assert not CC.median_premise(dict(geodesic_init=30.0)) and abs(math.exp(-30.0 / 50.0) - 0.55) < 0.01
    assert not CC.median_premise(dict(geodesic_sigma=-50.0)) and not CC.median_premise(dict(geodesic_init=-100.0))
    assert not CC.median_premise(dict(geodesic_sigma=1e6))
