"""TwoViewStereo's MRF stage on the CPU: tests/twoview_mrf_restatement.cpp (the yardstick of tests/test_gpu_twoview_mrf.py)
held against itself and against exact optima.  PARITY UNPINNED -- no compiled reference exists for this stage; what is
checked is that the restatement is the energy and the optimiser the header describes:
  * the direct O(L^2) message and the windowed one the kernel uses give identical bits (messages, labels, energies);
  * on chains (1 x N, N x 1) TRW-S is exact: the final energy equals the dynamic-programming optimum;
  * on grids small enough to enumerate: optimum <= final energy <= initial energy;
  * min_energy_drop = -1, max_iters = k makes k + 1 sweeps;
  * the library exports the new entry points and its defaults are the reference's constants."""
import itertools

import numpy as np
import pytest

import twoview_mrf_cases as TC
import twoview_mrf_ref as R


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("smooth_max", [0.5, 1.0, 2.0, 2.5, 4.0])
@pytest.mark.parametrize("lam", [0.25, 1.0, 7.5, 0.0])
def test_direct_and_windowed_messages_are_the_same_bits(smooth_max, lam):
    for (w, h, L, integer, seed) in [(9, 7, 10, False, 1), (9, 7, 10, True, 2), (5, 6, 3, True, 3), (4, 5, 65, False, 4),
                                     (1, 9, 2, True, 5), (6, 1, 7, False, 6)]:
        costs, _ = TC.volume(w, h, L, seed=seed, integer=integer)
        kw = dict(smooth_max=smooth_max, lambda_=lam, min_energy_drop=-1.0, max_iters=2)
        a = R.optimize(costs, form=R.DIRECT, **kw)
        b = R.optimize(costs, form=R.WINDOWED, **kw)
        assert a["iterations"] == b["iterations"] == 3
        assert np.array_equal(a["labels"], b["labels"])
        assert _same(a["messages"], b["messages"]), (w, h, L, integer)
        assert a["energy_final"] == b["energy_final"] and a["lower_bound"] == b["lower_bound"]
        assert _same(a["depth"], b["depth"])


def test_random_volumes_with_negative_and_large_costs():
    rng = np.random.default_rng(7)
    costs = rng.normal(scale=50.0, size=(6, 8, 12))
    costs[rng.uniform(size=costs.shape) < 0.1] = 11000.0
    for sm in (1.0, 2.0, 3.5):
        a = R.optimize(costs, form=R.DIRECT, smooth_max=sm, lambda_=3.0)
        b = R.optimize(costs, form=R.WINDOWED, smooth_max=sm, lambda_=3.0)
        assert np.array_equal(a["labels"], b["labels"]) and _same(a["messages"], b["messages"])
        assert a["iterations"] == b["iterations"]


def _chain_optimum(costs, lam, smax):
    """Dynamic programming over a chain of nodes: costs (n, L)."""
    n, L = costs.shape
    k = np.arange(L)
    V = lam * np.minimum(np.abs(k[:, None] - k[None, :]).astype(np.float64), smax)
    best = costs[0].copy()
    for i in range(1, n):
        best = costs[i] + (best[:, None] + V).min(axis=0)
    return best.min()


@pytest.mark.parametrize("shape", [(1, 23), (17, 1), (1, 2), (1, 1)])
@pytest.mark.parametrize("integer", [False, True])
def test_chains_reach_the_dynamic_programming_optimum(shape, integer):
    w, h = shape
    L = 9
    costs, _ = TC.volume(w, h, L, seed=w * 7 + h, integer=integer, mask_frac=1.0)
    lam, smax = (2.0, 2.0) if integer else (3.25, 2.5)
    r = R.optimize(costs, form=R.WINDOWED, lambda_=lam, smooth_max=smax, min_energy_drop=-1.0, max_iters=3)
    want = _chain_optimum(costs.reshape(-1, L), lam, smax)
    assert abs(r["energy_final"] - want) <= 1e-9 * max(1.0, abs(want)), (r["energy_final"], want)
    assert abs(R.energy(costs, r["labels"], lam, smax) - r["energy_final"]) == 0.0


@pytest.mark.parametrize("w,h,L", [(3, 2, 3), (2, 2, 4), (2, 3, 3)])
def test_enumerable_grids_are_bounded_by_the_optimum(w, h, L):
    for seed, integer in ((1, False), (2, True), (3, False)):
        costs, _ = TC.volume(w, h, L, seed=seed, integer=integer, mask_frac=1.0, fill_frac=0.1)
        lam, smax = 4.0, 2.0
        r = R.optimize(costs, lambda_=lam, smooth_max=smax, min_energy_drop=0.0)
        opt = min(R.energy(costs, np.array(lab, np.int32).reshape(h, w), lam, smax)
                  for lab in itertools.product(range(L), repeat=w * h))
        assert opt <= r["energy_final"] + 1e-9
        assert r["energy_final"] <= r["energy_initial"] + 1e-9
        assert r["lower_bound"] <= opt + 1e-9                  # TRW-S's bound is one


@pytest.mark.parametrize("k", [0, 1, 4])
def test_a_negative_energy_drop_makes_max_iters_plus_one_sweeps(k):
    costs, _ = TC.volume(8, 6, 5, seed=3)
    r = R.optimize(costs, min_energy_drop=-1.0, max_iters=k)
    assert r["iterations"] == k + 1
    # the default rule stops as soon as a sweep gains no more than 5
    d = R.optimize(costs)
    assert 1 <= d["iterations"] <= 51


def test_depth_from_label_and_fill_value():
    # twoviewstereo.cpp:981-985: t = label/(D - 1), t /= 5 - 4t, depth = min(1 - t) + max t
    assert R.depth_from_label(0, 64, 1.5, 9.0) == 1.5
    assert R.depth_from_label(63, 64, 1.5, 9.0) == 9.0
    t = (10 / 63.0) / (5 - 4 * (10 / 63.0))
    assert R.depth_from_label(10, 64, 1.5, 9.0) == 1.5 * (1 - t) + 9.0 * t
    assert R.fill_value(5, 1000.0) == 11000.0
    costs, mask = TC.volume(7, 5, 6, seed=1)
    r = R.optimize(costs, mask=mask, min_depth=2.0, max_depth=5.0)
    assert np.isnan(r["depth"][mask == 0]).all() and np.isfinite(r["depth"][mask == 1]).all()


def test_the_library_exports_the_mrf_stage_and_its_defaults():
    from stereoreconstruction_amd import capi
    L = capi.lib()
    for name in ("srh_twoview_mrf_params_defaults", "srh_twoview_label_costs", "srh_twoview_mrf_optimize", "srh_twoview_mrf",
                 "srh_twoview_compute_mrf", "srh_twoview_mrf_dims", "srh_twoview_mrf_state"):
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    m = capi.twoview_mrf_params()
    assert (m.smooth_exp, m.smooth_max, m.lambda_, m.max_iters, m.min_energy_drop) == (1, 2.0, 0.25, 50, 5.0)
    assert capi.twoview_mrf_params(**{"lambda": 0.5}).lambda_ == 0.5
    with pytest.raises(AttributeError):
        capi.twoview_mrf_params(beta=1.0)
