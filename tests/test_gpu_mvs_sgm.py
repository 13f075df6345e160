"""MultiViewStereo's semi-global aggregation over the top-K peak labels on the device (srh_mvs_sgm_estimate,
srh_mvs_initial_estimate_sgm, srh_mvs_sgm_estimate_views, srh_mvs_sgm_state; csrc/srh_mvs_sgm.hip) against the CPU
restatement tests/mvs_sgm_ref.py (itself checked in tests/test_mvs_sgm_ref.py).  NOT IN THE REFERENCE: the definition is
the header's.  The restatement is always fed the device's own data costs (srh_mvs_sgm_state), as the MRF tests do.

What must hold:
  * data costs: within 4 ulp of lambda*np.exp(-beta*cost), and the bits srh_mvs_mrf_state reports after an MRF run;
  * every single direction and several masks: S and the depth map bit for bit, the labels identical, depth untouched where
    the mask is not WHITE and +INF where "unknown" or a placeholder won, info.paths = the bits set, the energy within 1e-10
    relative (the device sums it as a tree, the restatement in order: the tolerance of test_gpu_mrf.py);
  * the entry points built on it give the same bits; the refusals of the MRF branch and of TwoViewStereo's aggregation."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import cases
import mrf_cases
import mvs_sgm_ref as G
import oracle_ffi as O
from stereoreconstruction_amd import capi
from test_gpu_mrf import _upload_blank_view

pytestmark = pytest.mark.gpu

GRIDS = [(1, 1, 9), (1, 37, 9), (53, 1, 9), (7, 16, 9), (3, 17, 9), (40, 28, 9), (100, 70, 9), (33, 35, 4), (20, 33, 15), (21, 19, 1)]
GRID_IDS = ["%dx%d-K%d" % g for g in GRIDS]
BEFORE = -7.0

_refs = {}


class _Device:
    """a peaks buffer on the device and a blank view of its size in slot 0"""

    def __init__(self, ctx, peaks, mask):
        import torch
        self.ctx, self.peaks, self.mask = ctx, peaks, mask
        self.h, self.w, self.K, _ = peaks.shape
        _upload_blank_view(ctx, 0, mask)
        self.buf = torch.from_numpy(np.ascontiguousarray(peaks)).to("cuda:0")
        torch.cuda.synchronize()

    def run(self, **over):
        self.ctx.upload_depth(0, np.full((self.h, self.w), BEFORE))
        info = self.ctx.mvs_sgm_estimate(0, self.K, self.buf.data_ptr(), capi.mvs_sgm_params(**over))
        assert self.ctx.mvs_sgm_dims() == (self.w, self.h, self.K)
        labels, D, S = self.ctx.mvs_sgm_state(self.w, self.h, self.K)
        return info, labels, D, S, self.ctx.download_depth(0)

    def unchanged(self):
        return np.array_equal(self.buf.cpu().numpy(), self.peaks)


def _ulps(a, b):
    return np.abs(a.view(np.int64) - b.view(np.int64))


def _ref_kw(over):
    kw = dict(over)
    if "lambda" in kw:
        kw["lam"] = kw.pop("lambda")
    kw.pop("path_mask", None)
    return kw


def _ref(key, peaks, mask, D, **over):
    """the restatement of all 8 directions on the device's data costs, computed once per case and shared (never modified)"""
    if key not in _refs:
        _refs[key] = (D.copy(), G.aggregate(peaks, D=D, view_mask=mask, depth=np.full(mask.shape, BEFORE), **_ref_kw(over)))
    D0, full = _refs[key]
    assert G.same_bits(D, D0), "the device's data costs changed between runs"
    return full


def _ref_for_mask(peaks, mask, D, full, path_mask, psi_u=0.002):
    paths = {k: full["paths"][k] for k in range(8) if path_mask >> k & 1}
    return G.finish(D, np.ascontiguousarray(peaks[..., 1]), paths, psi_u, path_mask, mask, np.full(mask.shape, BEFORE))


def _check(got, ref, peaks, mask, path_mask, tag):
    info, labels, D, sums, depth = got
    K = peaks.shape[2]
    neq = np.argwhere(sums.view(np.uint64) != ref["S"].view(np.uint64))
    assert len(neq) == 0, "%s: %d sums differ, first %s: %r vs %r" % (tag, len(neq), neq[:3].tolist(), sums[tuple(neq[0])], ref["S"][tuple(neq[0])])
    bad = np.argwhere(labels != ref["labels"])
    assert len(bad) == 0, "%s: %d labels differ, first at (y, x) = %s" % (tag, len(bad), bad[:5].tolist())
    assert np.array_equal(depth.view(np.uint64), ref["depth"].view(np.uint64)), tag
    assert (depth[mask != 1] == BEFORE).all(), tag
    z = np.concatenate([peaks[..., 1], np.full(mask.shape + (1,), -1.0)], axis=2)
    chosen = np.take_along_axis(z, labels[..., None].astype(np.int64), axis=2)[..., 0]
    sel = mask == 1
    assert np.isposinf(depth[sel & (chosen < 0)]).all() and np.array_equal(depth[sel & (chosen > 0)], chosen[sel & (chosen > 0)]), tag
    assert info["paths"] == G.popcount(path_mask), (tag, info)
    print("%s: energy %.17g (device) %.17g (restatement)" % (tag, info["energy"], ref["energy"]))
    assert abs(info["energy"] - ref["energy"]) <= 1e-10 * max(1.0, abs(ref["energy"])), (tag, info["energy"], ref["energy"])


def _case(w, h, K):
    return mrf_cases.peaks_case(w, h, K=K, seed=w * 131 + h, fill=0.6)


@pytest.mark.parametrize("w,h,K", [(40, 28, 9), (33, 35, 4), (20, 33, 15), (21, 19, 1)], ids=["40x28-K9", "33x35-K4", "20x33-K15", "21x19-K1"])
def test_data_costs(hip_ctx, w, h, K):
    peaks, mask = _case(w, h, K)
    dev = _Device(hip_ctx, peaks, mask)
    for over in (dict(), {"beta": 3.0, "lambda": 0.75, "phi_u": 0.25}):
        _, _, D, _, _ = dev.run(**over)
        lam, beta = over.get("lambda", 1.0), over.get("beta", 1.0)
        want = np.where(peaks[..., 1] < 0, lam, lam * np.exp(-beta * peaks[..., 0]))
        assert _ulps(D[..., :K], want).max() <= 4
        assert (D[..., K] == over.get("phi_u", 0.5)).all()
        # the very bits of the MRF branch's data costs on the same peaks (and its state and ours do not disturb each other)
        hip_ctx.mvs_mrf_estimate(0, K, dev.buf.data_ptr(), capi.mrf_params(max_iters=0, **over))
        _, Dm, _ = hip_ctx.mvs_mrf_state(w, h, K)
        assert G.same_bits(D, Dm)
        assert G.same_bits(hip_ctx.mvs_sgm_state(w, h, K)[1], D)
    assert dev.unchanged()


@pytest.mark.parametrize("w,h,K", GRIDS, ids=GRID_IDS)
def test_single_directions_and_masks(hip_ctx, w, h, K):
    peaks, mask = _case(w, h, K)
    dev = _Device(hip_ctx, peaks, mask)
    full = None
    for path_mask in [1 << k for k in range(8)] + [0x0F, 0xFF, 0xA5]:
        tag = "%dx%d K %d mask 0x%02X" % (w, h, K, path_mask)
        got = dev.run(path_mask=path_mask)
        if full is None:
            full = _ref((w, h, K), peaks, mask, got[2])
        assert G.same_bits(got[2], _refs[(w, h, K)][0]), tag
        ref = full if path_mask == 0xFF else _ref_for_mask(peaks, mask, got[2], full, path_mask)
        if G.popcount(path_mask) == 1:
            assert G.same_bits(ref["S"], full["paths"][path_mask.bit_length() - 1])
        _check(got, ref, peaks, mask, path_mask, tag)
    assert dev.unchanged()


@pytest.mark.parametrize("w,h", [(2049, 3), (3, 2049)])
def test_long_lines_and_many_short_ones(hip_ctx, w, h):
    """lines of 2049 pixels (the chunks of loads in flight turn over 512 times) beside 2051 diagonals of at most 3"""
    peaks, mask = mrf_cases.peaks_case_fast(w, h, K=9, seed=w, fill=0.6)
    got = _Device(hip_ctx, peaks, mask).run()
    ref = G.aggregate(peaks, D=got[2], view_mask=mask, depth=np.full((h, w), BEFORE))
    _check(got, ref, peaks, mask, 0xFF, "%dx%d" % (w, h))


def test_more_lines_than_one_wave_of_workgroups(hip_ctx):
    """320x240, all paths: 559 diagonal lines, 16 to a workgroup"""
    peaks, mask = mrf_cases.peaks_case_fast(320, 240, K=9, seed=11, fill=0.6)
    got = _Device(hip_ctx, peaks, mask).run()
    ref = G.aggregate(peaks, D=got[2], view_mask=mask, depth=np.full((240, 320), BEFORE))
    _check(got, ref, peaks, mask, 0xFF, "320x240")
    assert (ref["labels"] != np.argmin(got[2], axis=2)).sum() > 100         # it regularises


@pytest.mark.parametrize("over", [dict(phi_u=2.0), dict(psi_u=0.0), {"lambda": 0.0}, dict(beta=3.0)],
                         ids=["phi_u=2", "psi_u=0", "lambda=0", "beta=3"])
def test_other_parameters(hip_ctx, over):
    for (w, h, K) in ((40, 28, 9), (33, 35, 4)):
        peaks, mask = (mrf_cases.peaks_case_fast(40, 28, K=9, seed=40 * 131 + 28, fill=0.6) if K == 9 else _case(w, h, K))
        got = _Device(hip_ctx, peaks, mask).run(**over)
        ref = G.aggregate(peaks, D=got[2], view_mask=mask, depth=np.full((h, w), BEFORE), psi_u=over.get("psi_u", 0.002))
        _check(got, ref, peaks, mask, 0xFF, "%r %dx%d" % (over, w, h))
        if "phi_u" in over and K == 9:
            two = np.sort(ref["S"], axis=2)[..., :2]                    # the lowest-index rule decides these pixels
            assert (two[..., 0] == two[..., 1]).sum() > 10


def test_after_a_real_initial_estimate(hip_ctx):
    import torch
    case = cases.get_mvs("mvs_geodesic", w=48, h=36, D=20, nviews=3)
    imgs, ocams, op = cases.oracle_inputs(case)
    neigh = O.mvs_neighbours(ocams, op)
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    K = p.top_k
    plain = []
    for v in range(3):
        hip_ctx.mvs_initial_estimate(v, neigh[v], p)
        plain.append(hip_ctx.download_depth(v))
    # peaks, then the aggregation = srh_mvs_initial_estimate_sgm; against the restatement on the device's peaks
    one = []
    for v in range(3):
        pk = torch.zeros((36, 48, K, 2), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        hip_ctx.mvs_initial_estimate(v, neigh[v], p, peaks_dev=pk.data_ptr())
        hip_ctx.synchronize()
        info = hip_ctx.mvs_sgm_estimate(v, K, pk.data_ptr())
        labels, D, S = hip_ctx.mvs_sgm_state(48, 36, K)
        depth = hip_ctx.download_depth(v)
        mask = case["views"][v][1]
        ref = G.aggregate(pk.cpu().numpy(), D=D, view_mask=mask, depth=np.full((36, 48), np.inf))
        assert G.same_bits(S, ref["S"]) and np.array_equal(labels, ref["labels"])
        assert G.same_bits(depth, ref["depth"])                      # INF outside the mask: computeInitialEstimate left it there
        assert abs(info["energy"] - ref["energy"]) <= 1e-10 * max(1.0, abs(ref["energy"]))
        if v == 0:
            assert np.isfinite(depth[mask == 1]).any()
        hip_ctx.upload_depth(v, np.full((36, 48), -9.0))
        info2 = hip_ctx.mvs_initial_estimate_sgm(v, neigh[v], p)
        assert info2 == info and G.same_bits(hip_ctx.download_depth(v), depth)
        assert G.same_bits(hip_ctx.mvs_sgm_state(48, 36, K)[2], S)
        one.append((info, depth))
    # all views side by side: each view the bits of its single-view run; twice the same
    for rep in range(2):
        for v in range(3):
            hip_ctx.upload_depth(v, np.full((36, 48), -9.0))
            hip_ctx.mvs_initial_estimate_peaks(v, neigh[v], p)
        infos = hip_ctx.mvs_sgm_estimate_views([0, 1, 2])
        for v in range(3):
            assert infos[v] == one[v][0], (rep, v, infos[v], one[v][0])
            assert G.same_bits(hip_ctx.download_depth(v), one[v][1])
    with pytest.raises(capi.StereoHipError):
        hip_ctx.mvs_sgm_dims()                                           # the per-view runs leave no state
    # a subset, in another order, with other directions
    infos = hip_ctx.mvs_sgm_estimate_views([2, 0], capi.mvs_sgm_params(path_mask=0x0F))
    assert [i["paths"] for i in infos] == [4, 4]
    # a view listed twice (every view has kept peaks here): refused before anything is queued
    for v in range(3):
        hip_ctx.upload_depth(v, np.full((36, 48), -9.0))
    for twice in ([0, 0], [2, 0, 2]):
        with pytest.raises(capi.StereoHipError) as e:
            hip_ctx.mvs_sgm_estimate_views(twice)
        assert e.value.code == capi.SRH_E_INVALID and "twice" in str(e.value), (twice, str(e.value))
    for v in range(3):
        assert (hip_ctx.download_depth(v) == -9.0).all()
    # a cancel flag set before the call: nothing is written
    flag = C.c_int(1)
    try:
        hip_ctx.set_hooks(cancel_flag=flag)
        with pytest.raises(capi.StereoHipError) as e:
            hip_ctx.mvs_sgm_estimate_views([0, 1, 2])
        assert e.value.code == capi.SRH_E_CANCELLED
    finally:
        hip_ctx.set_hooks()
    for v in range(3):
        assert (hip_ctx.download_depth(v) == -9.0).all()
    # the plain estimate is what it was
    for v in range(3):
        hip_ctx.mvs_initial_estimate(v, neigh[v], p)
        assert G.same_bits(hip_ctx.download_depth(v), plain[v])


def test_refusals(hip_ctx):
    import torch
    peaks, mask = mrf_cases.peaks_case(12, 9, K=3, seed=2)
    _upload_blank_view(hip_ctx, 0, mask)
    pk = torch.from_numpy(np.ascontiguousarray(np.concatenate([peaks] * 6, axis=2))).to("cuda:0")   # room for any K below
    torch.cuda.synchronize()

    def run(K=3, slot=0, **over):
        return hip_ctx.mvs_sgm_estimate(slot, K, pk.data_ptr(), capi.mvs_sgm_params(**over))

    for K in (0, 16):
        with pytest.raises(capi.StereoHipError) as e:
            run(K)
        assert e.value.code == capi.SRH_E_UNSUPPORTED, K
    for over in ({"lambda": -1.0}, dict(phi_u=-0.5), dict(psi_u=-1e-3), dict(beta=float("inf")), dict(beta=float("nan")),
                 dict(path_mask=0), dict(path_mask=0x100), dict(path_mask=0x1FF), dict(path_mask=-1)):
        with pytest.raises(capi.StereoHipError) as e:
            run(**over)
        assert e.value.code == capi.SRH_E_INVALID, over
    with pytest.raises(capi.StereoHipError) as e:
        hip_ctx.mvs_sgm_estimate(0, 3, 0)                                # NULL peaks
    assert e.value.code == capi.SRH_E_INVALID
    with pytest.raises(capi.StereoHipError):
        run(slot=41)                                                     # no such view
    L = capi.lib()
    p = capi.params_mvs()
    nb = np.array([1], np.int32)
    assert L.srh_mvs_sgm_estimate(hip_ctx._h, 0, 3, C.c_void_p(pk.data_ptr()), None, None) == capi.SRH_E_INVALID
    assert L.srh_mvs_initial_estimate_sgm(hip_ctx._h, 0, nb.ctypes.data_as(capi.c_int32_p), 1, C.byref(p), None, None) == capi.SRH_E_INVALID
    assert L.srh_mvs_sgm_estimate_views(hip_ctx._h, nb.ctypes.data_as(capi.c_int32_p), 1, None, None) == capi.SRH_E_INVALID
    assert L.srh_mvs_sgm_estimate_views(None, nb.ctypes.data_as(capi.c_int32_p), 1, C.byref(capi.mvs_sgm_params()), None) == capi.SRH_E_INVALID
    # (a view listed twice: test_after_a_real_initial_estimate, where the views have kept peaks)
    with pytest.raises(capi.StereoHipError) as e:
        hip_ctx.mvs_sgm_estimate_views([0])                              # no kept peaks
    assert e.value.code == capi.SRH_E_INVALID and "peaks" in str(e.value)
    with pytest.raises(capi.StereoHipError):
        hip_ctx.mvs_sgm_estimate_views([0], capi.mvs_sgm_params(path_mask=0))
    # state: a finished run, then wrong dimensions
    info = run()
    assert info["paths"] == 8 and hip_ctx.mvs_sgm_dims() == (12, 9, 3)
    for dims in ((12, 9, 4), (9, 12, 3), (12, 8, 3)):
        with pytest.raises(capi.StereoHipError):
            hip_ctx.mvs_sgm_state(*dims)
    assert L.srh_mvs_sgm_state(None, 12, 9, 3, None, None, None) == capi.SRH_E_INVALID
    assert L.srh_mvs_sgm_state(hip_ctx._h, 12, 9, 3, None, None, None) == capi.SRH_OK
    # an upload of a view of that size forgets the state
    _upload_blank_view(hip_ctx, 0, mask)
    with pytest.raises(capi.StereoHipError):
        hip_ctx.mvs_sgm_dims()
    with pytest.raises(capi.StereoHipError):
        hip_ctx.mvs_sgm_state(12, 9, 3)
    # a device that is too small: refused before anything runs, the message names the bytes
    peaks, mask = mrf_cases.peaks_case_fast(100, 70, K=9, seed=3)
    _upload_blank_view(hip_ctx, 0, mask)
    big = torch.from_numpy(peaks).to("cuda:0")
    torch.cuda.synchronize()
    hip_ctx.upload_depth(0, np.full((70, 100), -3.0))
    try:
        hip_ctx.set_option("mem_limit_mb", 2)                            # depths, data costs and sums are 0.9 MB each
        with pytest.raises(capi.StereoHipError) as e:
            hip_ctx.mvs_sgm_estimate(0, 9, big.data_ptr())
        assert e.value.code == capi.SRH_E_DEVICE and "bytes" in str(e.value) and str(100 * 70 * 16 * 8) in str(e.value)
    finally:
        hip_ctx.set_option("mem_limit_mb", 0)
    assert (hip_ctx.download_depth(0) == -3.0).all()
    # a cancel flag set before the call
    flag = C.c_int(1)
    try:
        hip_ctx.set_hooks(cancel_flag=flag)
        with pytest.raises(capi.StereoHipError) as e:
            hip_ctx.mvs_sgm_estimate(0, 9, big.data_ptr())
        assert e.value.code == capi.SRH_E_CANCELLED
    finally:
        hip_ctx.set_hooks()
    assert (hip_ctx.download_depth(0) == -3.0).all()
    info = hip_ctx.mvs_sgm_estimate(0, 9, big.data_ptr())
    assert info["paths"] == 8 and not (hip_ctx.download_depth(0)[mask == 1] == -3.0).any()


def test_host_class_use_sgm(hip_ctx, tmp_path):
    """MultiViewStereo::setUseSGM(true) through the host class = peaks + srh_mvs_sgm_estimate_views + the cross-check chain
    through the C-ABI; switched off, the winner-take-all maps as before"""
    import test_gpu_host_api as HA
    import test_mvs_sgm_host as TH
    exe = TH.build(tmp_path)
    case = cases.get_mvs("mvs_geodesic", w=48, h=36, D=20, nviews=3)
    views = []
    for (rgba, mask, cam, dist, plane) in case["views"]:
        im = rgba.copy()
        im[..., 3] = np.where(mask == 1, 255, 51)                       # the class takes the mask from the alpha channel
        views.append((im, mask, cam, dist, plane))
    case = dict(case, views=views)
    imgs, ocams, op = cases.oracle_inputs(case)
    neigh = O.mvs_neighbours(ocams, op)
    cams, p = cases.hip_inputs(case)
    want = {}
    for sgm in (True, False):
        cases.upload_case(hip_ctx, case, cams)
        for v in range(3):
            if sgm:
                hip_ctx.mvs_initial_estimate_peaks(v, neigh[v], p)
            else:
                hip_ctx.mvs_initial_estimate(v, neigh[v], p)
        infos = hip_ctx.mvs_sgm_estimate_views([0, 1, 2]) if sgm else None
        for v in range(3):
            hip_ctx.mvs_cross_check([0, 1, 2], v, p)
        want[sgm] = ([hip_ctx.download_depth(v) for v in range(3)], infos)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    HA._write_input(inp, case, False)
    for sgm in (True, False):
        subprocess.check_call([exe, "compute", inp, outp, "1" if sgm else "0"])
        got, steps = HA._read_output(outp, 3, 48, 36)
        assert steps == list(range(6))
        for v in range(3):
            assert G.same_bits(got[v], want[sgm][0][v]), (sgm, v)
        rec = np.frombuffer(open(outp, "rb").read()[-48:], np.float64)
        for v in range(3):
            if sgm:
                assert (int(rec[2 * v]), rec[2 * v + 1]) == (want[sgm][1][v]["paths"], want[sgm][1][v]["energy"])
            else:
                assert rec[2 * v] == 0 and rec[2 * v + 1] == 0
    assert not all(G.same_bits(a, b) for a, b in zip(want[True][0], want[False][0]))
