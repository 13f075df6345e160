"""The profile entries of the label-volume stages' one-view entry points (srh_profile_*): which kernels a call brackets,
under which names and how often.  profiles/*_timing.py read these names and divide by these counts, and nothing else in the
suite looks at them.  The several-views forms record none: their kernels run on streams of their own, and a profile entry is
a pair of events on the context's stream."""
import numpy as np
import pytest

import cases
import mrf_cases
import oracle_ffi as O
import twoview_mrf_cases as TC
from stereoreconstruction_amd import capi
from test_gpu_mrf import _upload_blank_view

pytestmark = pytest.mark.gpu

W, H, K, L = 12, 9, 3, 5
MVS_DIRS = ["+1,0", "-1,0", "0,+1", "0,-1", "+1,+1", "-1,-1", "+1,-1", "-1,+1"]


def _counts(ctx, call):
    """{profile entry: launches} of one call; the session's context is left with profiling off"""
    ctx.synchronize()
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        result = call()
        return result, {name: n for name, (_, n) in ctx.profile().items() if n}
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()


def _peaks_on_device(ctx):
    import torch
    peaks, mask = mrf_cases.peaks_case(W, H, K=K, seed=2)
    _upload_blank_view(ctx, 0, mask)
    pk = torch.from_numpy(np.ascontiguousarray(peaks)).to("cuda:0")
    torch.cuda.synchronize()
    return pk


def test_mvs_mrf_estimate(hip_ctx):
    pk = _peaks_on_device(hip_ctx)
    info, got = _counts(hip_ctx, lambda: hip_ctx.mvs_mrf_estimate(0, K, pk.data_ptr()))
    it = info["iterations"]
    assert it >= 1
    assert got == {"mrf_data_kernel": 1, "mrf_pass_kernel": it, "mrf_energy_kernel": it + 1, "mrf_depth_kernel": 1}


def test_mvs_sgm_estimate(hip_ctx):
    pk = _peaks_on_device(hip_ctx)
    mask = 0b00100101
    info, got = _counts(hip_ctx, lambda: hip_ctx.mvs_sgm_estimate(0, K, pk.data_ptr(), capi.mvs_sgm_params(path_mask=mask)))
    assert info["paths"] == 3
    want = {"mvs_sgm_path_kernel[%s]" % d: 1 for k, d in enumerate(MVS_DIRS) if mask >> k & 1}
    want.update({"mvs_sgm_readoff_kernel": 1, "mrf_data_kernel": 1, "mrf_energy_kernel": 1})
    assert got == want


def test_twoview_mrf_optimize(hip_ctx):
    import torch
    costs, mask = TC.volume(W, H, L)
    _upload_blank_view(hip_ctx, 0, mask)
    vol = torch.from_numpy(np.ascontiguousarray(costs)).to("cuda:0")
    torch.cuda.synchronize()
    p = capi.params_twoview(num_depth_levels=L)
    info, got = _counts(hip_ctx, lambda: hip_ctx.twoview_mrf_optimize(0, p, L, vol.data_ptr()))
    it = info["iterations"]
    assert it >= 1
    assert got == {"twoview_mrf_pass_kernel": it, "twoview_mrf_energy_kernel": it + 1, "twoview_mrf_depth_kernel": 1}


def test_twoview_sgm(hip_ctx):
    mask = np.ones((H, W), dtype=np.uint8)
    _upload_blank_view(hip_ctx, 0, mask)
    _upload_blank_view(hip_ctx, 1, mask)
    p = capi.params_twoview(num_depth_levels=L)
    info, got = _counts(hip_ctx, lambda: hip_ctx.twoview_sgm(0, 1, p))
    assert info["paths"] == 8
    want = {"twoview_sgm_path_kernel[%s]" % d: 1 for d in MVS_DIRS}
    want.update({"twoview_label_costs_kernel": 1, "twoview_sgm_readoff_kernel": 1, "twoview_mrf_energy_kernel": 1})
    assert got == want


def test_the_several_views_forms_record_nothing(hip_ctx):
    case = cases.get_mvs("mvs_geodesic", w=48, h=36, D=20, nviews=3)
    _, ocams, op = cases.oracle_inputs(case)
    neigh = O.mvs_neighbours(ocams, op)
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    for v in range(2):
        hip_ctx.mvs_initial_estimate_peaks(v, neigh[v], p)
    infos, got = _counts(hip_ctx, lambda: hip_ctx.mvs_sgm_estimate_views([0, 1]))
    assert [i["paths"] for i in infos] == [8, 8] and got == {}
    infos, got = _counts(hip_ctx, lambda: hip_ctx.mvs_mrf_estimate_views([0, 1]))
    assert all(i["iterations"] >= 1 for i in infos) and got == {}
