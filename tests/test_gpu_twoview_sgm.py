"""TwoViewStereo's semi-global aggregation on the device (srh_twoview_sgm_aggregate, srh_twoview_sgm,
srh_twoview_compute_sgm, srh_twoview_sgm_state; csrc/srh_twoview_sgm.hip) against the CPU restatement tests/sgm_ref.py
(itself checked in tests/test_sgm_ref.py).  NOT IN THE REFERENCE: the definition is the header's.

What must hold:
  * a single direction (path_mask = 1 << k): the sums are the bits of the restatement's L_k; labels and depth identical;
  * several directions: S, labels and depth bit for bit, depth NaN exactly where the mask is not WHITE, the energy within
    1e-10 relative (the device sums it as a tree, the restatement in order: the tolerance of test_gpu_twoview_mrf.py),
    info.paths = the bits set;
  * end to end: srh_twoview_compute_sgm = label costs -> restatement -> the oracle's cross-check, bit for bit."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import cases
import oracle_ffi as O
import sad_ref as S
import sgm_ref as G
import twoview_mrf_cases as TC
from stereoreconstruction_amd import capi
from test_gpu_sad import _assert_same, _options
from test_gpu_twoview_mrf import _case, _upload_blank_view

pytestmark = pytest.mark.gpu

ZMIN, ZMAX = 1.25, 7.5

# every grid and every label count at least once (NL = 1 .. 4, 16-byte and 8-byte pieces, a ragged last lane); every
# direction and every mask below runs on each of them, on a float and on an integer (many ties) volume
COMBOS = [(1, 1, 2), (1, 37, 3), (53, 1, 63), (7, 16, 64), (3, 17, 65), (33, 35, 100), (100, 70, 128), (33, 35, 130), (7, 16, 201),
          (100, 70, 256)]
COMBO_IDS = ["%dx%dx%d" % c for c in COMBOS]

_refs = {}


def _volume(w, h, L, integer):
    return TC.volume(w, h, L, seed=w * 131 + h + L, integer=integer)


def _ref(w, h, L, integer):
    """the restatement of all 8 directions with the default term, computed once and shared (never modified)"""
    key = (w, h, L, integer)
    if key not in _refs:
        costs, mask = _volume(w, h, L, integer)
        _refs[key] = (costs, mask, G.aggregate(costs, view_mask=mask, min_depth=ZMIN, max_depth=ZMAX))
    return _refs[key]


def _ref_for_mask(costs, mask, full, path_mask, lam=0.25, smax=2.0):
    paths = {k: full["paths"][k] for k in range(8) if path_mask >> k & 1}
    return G._finish(costs, paths, lam, smax, path_mask, mask, ZMIN, ZMAX)


class _Device:
    """a volume on the device and a blank view of its size in slot 0"""

    def __init__(self, ctx, costs, mask, offset_doubles=0):
        import torch
        self.ctx, self.costs = ctx, costs
        self.h, self.w, self.L = costs.shape
        self.p = capi.params_twoview(min_depth=ZMIN, max_depth=ZMAX, num_depth_levels=self.L)
        _upload_blank_view(ctx, 0, mask)
        flat = np.concatenate([np.full(offset_doubles, -1.0), costs.ravel()])
        self.buf = torch.from_numpy(flat).to("cuda:0")
        torch.cuda.synchronize()
        self.ptr = self.buf.data_ptr() + 8 * offset_doubles
        self.offset = offset_doubles

    def run(self, **over):
        self.ctx.upload_depth(0, np.full((self.h, self.w), -7.0))
        info = self.ctx.twoview_sgm_aggregate(0, self.p, self.L, self.ptr, capi.twoview_sgm_params(**over))
        assert self.ctx.twoview_sgm_dims() == (self.w, self.h, self.L)
        labels, _, sums = self.ctx.twoview_sgm_state(self.w, self.h, self.L)
        return info, labels, sums, self.ctx.download_depth(0)

    def unchanged(self):
        got = self.buf.cpu().numpy()
        return (got[:self.offset] == -1.0).all() and np.array_equal(got[self.offset:].reshape(self.costs.shape), self.costs)


def _check(got, ref, mask, path_mask, tag):
    info, labels, sums, depth = got
    neq = np.argwhere(sums.view(np.uint64) != ref["S"].view(np.uint64))
    assert len(neq) == 0, "%s: %d sums differ, first %s: %r vs %r" % (tag, len(neq), neq[:3].tolist(), sums[tuple(neq[0])], ref["S"][tuple(neq[0])])
    bad = np.argwhere(labels != ref["labels"])
    assert len(bad) == 0, "%s: %d labels differ, first at (y, x) = %s" % (tag, len(bad), bad[:5].tolist())
    assert np.array_equal(depth.view(np.uint64), ref["depth"].view(np.uint64)), tag
    assert np.isnan(depth[mask != 1]).all() and (~np.isnan(depth[mask == 1])).all(), tag
    assert info["paths"] == G.popcount(path_mask), (tag, info)
    assert abs(info["energy"] - ref["energy"]) <= 1e-10 * max(1.0, abs(ref["energy"])), (tag, info["energy"], ref["energy"])


@pytest.mark.parametrize("w,h,L", COMBOS, ids=COMBO_IDS)
def test_single_directions(hip_ctx, w, h, L):
    for integer in (False, True):
        costs, mask, full = _ref(w, h, L, integer)
        dev = _Device(hip_ctx, costs, mask)
        for k in range(8):
            tag = "%dx%dx%d%s direction %d" % (w, h, L, " int" if integer else "", k)
            ref = _ref_for_mask(costs, mask, full, 1 << k)
            assert S.same_bits(ref["S"], full["paths"][k])
            _check(dev.run(path_mask=1 << k), ref, mask, 1 << k, tag)
        assert dev.unchanged()


@pytest.mark.parametrize("w,h,L", COMBOS, ids=COMBO_IDS)
def test_sums(hip_ctx, w, h, L):
    for integer in (False, True):
        costs, mask, full = _ref(w, h, L, integer)
        dev = _Device(hip_ctx, costs, mask)
        for path_mask in (0x0F, 0xFF, 0xA5):
            tag = "%dx%dx%d%s mask 0x%02X" % (w, h, L, " int" if integer else "", path_mask)
            ref = full if path_mask == 0xFF else _ref_for_mask(costs, mask, full, path_mask)
            _check(dev.run(path_mask=path_mask), ref, mask, path_mask, tag)
        assert dev.unchanged()


def test_regularises_and_ties():
    """what the cases above exercise: the labels differ from the per-pixel argmin, and the integer volume has pixels whose
    two lowest sums are equal (the tie rule decides)"""
    costs, mask, full = _ref(100, 70, 256, True)
    assert (full["labels"] != np.argmin(costs, axis=2)).sum() > 100
    two = np.sort(full["S"], axis=2)[..., :2]
    assert (two[..., 0] == two[..., 1]).sum() > 10


@pytest.mark.parametrize("smooth_max,lam", [(0.5, 1.0), (1.0, 3.0), (2.5, 0.25), (4.0, 2.0), (3.0, 0.0)])
def test_other_smoothness_terms(hip_ctx, smooth_max, lam):
    """every window width of the message (0 .. 3 neighbours each side) at 1, 2, 3 and 4 labels per lane"""
    for (w, h, L) in ((33, 35, 10), (20, 18, 65), (9, 21, 130), (8, 19, 201), (11, 18, 128)):
        costs, mask = TC.volume(w, h, L, seed=L + w, integer=(L == 65))
        ref = G.aggregate(costs, lam, smooth_max, view_mask=mask, min_depth=ZMIN, max_depth=ZMAX)
        got = _Device(hip_ctx, costs, mask).run(smooth_max=smooth_max, **{"lambda": lam})
        _check(got, ref, mask, 0xFF, "smax %g lambda %g %dx%dx%d" % (smooth_max, lam, w, h, L))


@pytest.mark.parametrize("L", [64, 128, 256])
def test_volume_off_the_16_byte_boundary(hip_ctx, L):
    """a caller's volume 8 bytes into its allocation takes the 8-byte path: same bits, the volume (and the double before
    it) unchanged"""
    costs, mask = TC.volume(19, 11, L, seed=L)
    ref = G.aggregate(costs, view_mask=mask, min_depth=ZMIN, max_depth=ZMAX)
    dev = _Device(hip_ctx, costs, mask, offset_doubles=1)
    assert dev.ptr % 16 == 8
    _check(dev.run(), ref, mask, 0xFF, "offset volume L = %d" % L)
    assert dev.unchanged()
    aligned = _Device(hip_ctx, costs, mask)
    assert aligned.ptr % 16 == 0
    _check(aligned.run(), ref, mask, 0xFF, "aligned volume L = %d" % L)


@pytest.mark.parametrize("w,h", [(2049, 3), (3, 2049)])
def test_long_lines_and_many_short_ones(hip_ctx, w, h):
    """lines of 2049 pixels (the ring of loads in flight wraps 512 times) beside 2051 diagonals of at most 3"""
    costs, mask = TC.volume(w, h, 5, seed=w)
    ref = G.aggregate(costs, view_mask=mask, min_depth=ZMIN, max_depth=ZMAX)
    _check(_Device(hip_ctx, costs, mask).run(), ref, mask, 0xFF, "%dx%dx5" % (w, h))


def test_more_lines_than_one_launch_keeps_resident(hip_ctx):
    """640x480x64, all paths: 1119 diagonal lines"""
    costs, mask = TC.volume(640, 480, 64, seed=11)
    ref = G.aggregate(costs, view_mask=mask, min_depth=ZMIN, max_depth=ZMAX)
    _check(_Device(hip_ctx, costs, mask).run(), ref, mask, 0xFF, "640x480x64")


def _chain(ctx, case, ocams, op, p):
    """label costs -> restatement -> the oracle's cross-check"""
    maps, vols = [], []
    for ref, oth in ((0, 1), (1, 0)):
        cost, _ = ctx.twoview_label_costs(ref, oth, p, want_pixels=False)
        vols.append(cost)
        maps.append(G.aggregate(cost, view_mask=case["views"][ref][1], min_depth=op.min_depth, max_depth=op.max_depth))
    dl, dr = O.twoview_cross_check(ocams[0], ocams[1], op, maps[0]["depth"], maps[1]["depth"])
    return dl, dr, maps, vols


@pytest.mark.parametrize("name,kind", [("geodesic_rect", capi.COST_NCC), ("adaptive_masks", capi.COST_SAD), ("adaptive_verged", capi.COST_NCC)])
def test_compute_sgm_end_to_end(hip_ctx, name, kind):
    case, imgs, ocams, op, cams, p = _case(name)
    cases.upload_case(hip_ctx, case, cams)
    before = hip_ctx.twoview_compute(0, 1, p)
    steps = []
    try:
        hip_ctx.set_hooks(progress=lambda step, stage: steps.append((step, stage)))
        with _options(hip_ctx, cost=kind):
            dl, dr, maps, vols = _chain(hip_ctx, case, ocams, op, p)
            del steps[:]
            gl, gr, infos = hip_ctx.twoview_compute_sgm(0, 1, p)
            got_steps = list(steps)
            gl2, gr2, infos2 = hip_ctx.twoview_compute_sgm(0, 1, p)
            labels, D, sums = hip_ctx.twoview_sgm_state(*hip_ctx.twoview_sgm_dims(), want_costs=True)
    finally:
        hip_ctx.set_hooks()
    assert [s for s, _ in got_steps] == [1, 2, 3, 4, 5, 8]
    assert got_steps[1][1] == "Aggregating..." and got_steps[3][1] == "Aggregating..."
    assert got_steps[0][1] == "Computing cost volume for left image..." and got_steps[2][1] == "Computing cost volume for right image..."
    assert got_steps[4][1] == "Detecting inconsistencies..." and got_steps[5][1] == "Finished!"
    _assert_same(gl, dl, name + " left")
    _assert_same(gr, dr, name + " right")
    for k in range(2):
        assert infos[k]["paths"] == 8
        assert abs(infos[k]["energy"] - maps[k]["energy"]) <= 1e-10 * max(1.0, abs(maps[k]["energy"]))
    # the state is the second direction's
    assert np.array_equal(labels, maps[1]["labels"]) and S.same_bits(sums, maps[1]["S"]) and S.same_bits(D, vols[1])
    mask = case["views"][0][1]
    assert np.isnan(gl[mask != 1]).all()
    # running twice gives the same bits
    _assert_same(gl2, gl, name + " left again")
    _assert_same(gr2, gr, name + " right again")
    assert infos2 == infos
    # the live path is untouched
    after = hip_ctx.twoview_compute(0, 1, p)
    for k in range(2):
        _assert_same(after[k], before[k], name + " WTA afterwards %d" % k)
    # one direction alone = the first half
    with _options(hip_ctx, cost=kind):
        info = hip_ctx.twoview_sgm(0, 1, p)
    assert info == infos[0]
    _assert_same(hip_ctx.download_depth(0), maps[0]["depth"], name + " one direction")


def test_compute_sgm_with_hole_filling_steps(hip_ctx):
    case, imgs, ocams, op, cams, p = _case("geodesic_rect")
    cases.upload_case(hip_ctx, case, cams)
    steps = []
    try:
        hip_ctx.set_hooks(progress=lambda step, stage: steps.append(step))
        with _options(hip_ctx, filter_invalid=capi.FILTER_GAPS | capi.FILTER_MEDIAN):
            hip_ctx.twoview_compute_sgm(0, 1, p)
    finally:
        hip_ctx.set_hooks()
    assert steps == [1, 2, 3, 4, 5, 6, 7, 8]


def test_refusals(hip_ctx):
    import torch
    costs, mask = TC.volume(12, 9, 5, seed=2)
    _upload_blank_view(hip_ctx, 0, mask)
    _upload_blank_view(hip_ctx, 1, mask)
    vol = torch.from_numpy(np.ascontiguousarray(np.concatenate([costs] * 60, axis=-1))).to("cuda:0")   # room for any L below
    torch.cuda.synchronize()

    def run(L, **over):
        return hip_ctx.twoview_sgm_aggregate(0, capi.params_twoview(num_depth_levels=max(L, 2)), L, vol.data_ptr(),
                                             capi.twoview_sgm_params(**over))

    for L, over in ((1, {}), (257, {}), (5, dict(smooth_exp=2)), (5, dict(smooth_max=0.0)), (5, dict(smooth_max=5.0))):
        with pytest.raises(capi.StereoHipError) as e:
            run(L, **over)
        assert e.value.code == capi.SRH_E_UNSUPPORTED, (L, over)
    for over in ({"lambda": -1.0}, dict(path_mask=0), dict(path_mask=0x100), dict(path_mask=0x1FF), dict(path_mask=-1)):
        with pytest.raises(capi.StereoHipError) as e:
            run(5, **over)
        assert e.value.code == capi.SRH_E_INVALID, over
    with pytest.raises(capi.StereoHipError) as e:                      # labels and depth levels must agree
        hip_ctx.twoview_sgm_aggregate(0, capi.params_twoview(num_depth_levels=6), 5, vol.data_ptr())
    assert e.value.code == capi.SRH_E_INVALID
    with pytest.raises(capi.StereoHipError):
        hip_ctx.twoview_sgm_aggregate(0, capi.params_twoview(num_depth_levels=5), 5, 0)                 # NULL volume
    with pytest.raises(capi.StereoHipError):
        hip_ctx.twoview_sgm_aggregate(41, capi.params_twoview(num_depth_levels=5), 5, vol.data_ptr())   # no such view
    L = capi.lib()
    p5 = capi.params_twoview(num_depth_levels=5)
    assert L.srh_twoview_sgm_aggregate(hip_ctx._h, 0, C.byref(p5), 5, C.c_void_p(vol.data_ptr()), None, None) == capi.SRH_E_INVALID
    assert L.srh_twoview_sgm(hip_ctx._h, 0, 1, None, None, None) == capi.SRH_E_INVALID
    assert L.srh_twoview_sgm(hip_ctx._h, 0, 1, C.byref(p5), None, None) == capi.SRH_E_INVALID
    assert L.srh_twoview_compute_sgm(hip_ctx._h, 0, 1, C.byref(p5), None, None, None, None) == capi.SRH_E_INVALID
    with pytest.raises(capi.StereoHipError):
        hip_ctx.twoview_sgm(0, 0, p5)                                  # one slot twice
    # state: a finished run, then wrong dimensions
    info = run(5)
    assert info["paths"] == 8 and hip_ctx.twoview_sgm_dims() == (12, 9, 5)
    for dims in ((12, 9, 6), (9, 12, 5), (12, 8, 5)):
        with pytest.raises(capi.StereoHipError):
            hip_ctx.twoview_sgm_state(*dims)
    with pytest.raises(capi.StereoHipError):
        hip_ctx.twoview_sgm_state(12, 9, 5, want_costs=True)           # the volume was the caller's
    assert L.srh_twoview_sgm_state(None, 12, 9, 5, None, None, None) == capi.SRH_E_INVALID
    assert L.srh_twoview_sgm_state(hip_ctx._h, 12, 9, 5, None, None, None) == capi.SRH_OK
    # an upload of a view of that size forgets the state
    _upload_blank_view(hip_ctx, 0, mask)
    with pytest.raises(capi.StereoHipError):
        hip_ctx.twoview_sgm_dims()
    # a device that is too small: refused before anything runs, the message names the bytes
    costs, mask = TC.volume(100, 70, 64, seed=3)
    _upload_blank_view(hip_ctx, 0, mask)
    _upload_blank_view(hip_ctx, 1, mask)
    big = torch.from_numpy(costs).to("cuda:0")
    torch.cuda.synchronize()
    hip_ctx.upload_depth(0, np.full((70, 100), -3.0))
    p64 = capi.params_twoview(num_depth_levels=64)
    try:
        hip_ctx.set_option("mem_limit_mb", 2)                          # the sums alone are 3.6 MB
        with pytest.raises(capi.StereoHipError) as e:
            hip_ctx.twoview_sgm_aggregate(0, p64, 64, big.data_ptr())
        assert e.value.code == capi.SRH_E_DEVICE and "bytes" in str(e.value) and str(100 * 70 * 64 * 8) in str(e.value)
    finally:
        hip_ctx.set_option("mem_limit_mb", 0)
    assert (hip_ctx.download_depth(0) == -3.0).all()
    # a cancel flag set before the call
    flag = C.c_int(1)
    try:
        hip_ctx.set_hooks(cancel_flag=flag)
        for call in (lambda: hip_ctx.twoview_sgm_aggregate(0, p64, 64, big.data_ptr()),
                     lambda: hip_ctx.twoview_sgm(0, 1, capi.params_twoview(num_depth_levels=8)),
                     lambda: hip_ctx.twoview_compute_sgm(0, 1, capi.params_twoview(num_depth_levels=8))):
            with pytest.raises(capi.StereoHipError) as e:
                call()
            assert e.value.code == capi.SRH_E_CANCELLED
    finally:
        hip_ctx.set_hooks()
    assert (hip_ctx.download_depth(0) == -3.0).all()
    info = hip_ctx.twoview_sgm_aggregate(0, p64, 64, big.data_ptr())
    assert info["paths"] == 8 and not (hip_ctx.download_depth(0) == -3.0).any()


def test_host_class_use_sgm(hip_ctx, tmp_path):
    """TwoViewStereo::setUseSGM(true) through the host class = srh_twoview_compute_sgm through the C-ABI"""
    import test_gpu_host_api as HA
    import test_twoview_sgm_host as TH
    exe = TH.build(tmp_path)
    case = cases.get_twoview("geodesic_masks")
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    want_l, want_r, infos = hip_ctx.twoview_compute_sgm(0, 1, p)
    plain = hip_ctx.twoview_compute(0, 1, p)
    h, w = want_l.shape
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    HA._write_input(inp, case, True)
    subprocess.check_call([exe, "compute", inp, outp, "1", str(capi.COST_NCC)])
    (gl, gr), steps = HA._read_output(outp, 2, w, h)
    assert steps == [1, 2, 3, 4, 5, 8]
    _assert_same(gl, want_l, "host left")
    _assert_same(gr, want_r, "host right")
    rec = np.frombuffer(open(outp, "rb").read()[-64:], np.float64)
    for k in range(2):
        assert (int(rec[2 * k]), rec[2 * k + 1]) == (infos[k]["paths"], infos[k]["energy"])
    assert (rec[4:] == 0).all()                                        # no scan made these maps: no WTA by-products
    assert not S.same_bits(gl, plain[0])
    # the switch off: the reference as it is compiled
    subprocess.check_call([exe, "compute", inp, outp, "0", str(capi.COST_NCC)])
    (gl, gr), steps = HA._read_output(outp, 2, w, h)
    assert steps == [1, 3, 5, 8]
    _assert_same(gl, plain[0], "host WTA left")
    _assert_same(gr, plain[1], "host WTA right")
    assert (np.frombuffer(open(outp, "rb").read()[-64:], np.float64) == 0).all()
