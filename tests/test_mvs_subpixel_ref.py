"""srh_mvs_view_subpixel without a device: the facts the stage rests on -- a MultiViewStereo depth map identifies
its own winner -- as assertions on the CPU oracle, every class of the definition of tests/mvs_subpixel_ref.py, what the
refinement buys on a slanted plane seen by three views, and the interface: exports, header, binding and a program using the
host class's new members (tests/test_gpu_mvs_subpixel.py runs the stage on the device)."""
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import mvs_subpixel_ref as MR
import oracle_ffi as O
from stereoreconstruction_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "stereoreconstruction_amd", "host")
SMALL = dict(w=40, h=28, D=12, nviews=3)
PROBE_CASES = [("mvs_geodesic", SMALL), ("mvs_distorted", {}), ("mvs_refractive", {}), ("mvs_scaled", {})]


def build_host_program(out_dir):
    """tests/host_mvs_subpixel_test.cpp against the host library and libstereo_recon_hip, by host/Makefile -> its path"""
    subprocess.check_call(["make", "-C", HOST, "mvs_subpixel_test", "TESTBIN=" + str(out_dir)], stdout=subprocess.DEVNULL)
    return os.path.join(str(out_dir), "host_mvs_subpixel_test")


_SMALL = {}


def small_geodesic():
    """mvs_geodesic 40x28x12, 3 views: (imgs, ocams, op, neigh, WTA map of view 0, its peaks), computed once"""
    if not _SMALL:
        case = cases.get_mvs("mvs_geodesic", **SMALL)
        imgs, ocams, op = cases.oracle_inputs(case)
        neigh = O.mvs_neighbours(ocams, op)
        depth, peaks, _ = O.mvs_initial_estimate(imgs, ocams, 0, neigh[0], op, want_peaks=True)
        _SMALL["v"] = (imgs, ocams, op, neigh, depth, peaks)
    return _SMALL["v"]


# ---------------------------------------------------------------------------------------------- (a) the probe facts
@pytest.mark.parametrize("name,over", PROBE_CASES, ids=[c[0] for c in PROBE_CASES])
def test_a_depth_map_identifies_its_own_winner(name, over):
    """views 0 and 1: every pixel with 0 < depth < inf has a winner, exactly one distinct (neighbour, pixel) matches, the
    winner's recomputed cost is the top peak's cost bit for bit, and the winner has at most 2 visited neighbours"""
    case = cases.get_mvs(name, **over)
    imgs, ocams, op = cases.oracle_inputs(case)
    neigh = O.mvs_neighbours(ocams, op)
    for v in (0, 1):
        depth, peaks, _ = O.mvs_initial_estimate(imgs, ocams, v, neigh[v], op, want_peaks=True)
        out = MR.refine_view(imgs, ocams, op, v, neigh[v], depth, count_all=True)
        has = np.isfinite(depth) & (depth > 0)
        assert has.sum() > 300
        assert (out["cls"][has] != MR.NO_WINNER).all() and (out["cls"][has] != MR.NONE).all()
        assert (out["nmatch"][has] == 1).all(), np.bincount(out["nmatch"][has])
        assert (out["cls"][~has] == MR.NONE).all() and (out["win"][~has] == -1).all()
        assert out["nadj"].max() <= 2
        costed = out["cls"] >= MR.FLAT
        assert costed.any()
        assert np.array_equal(out["c0"][costed].view(np.uint64), peaks[:, :, -1, 0][costed].view(np.uint64))
        # after the plain WTA the winner's cost is the maximum: nothing is FLAT or OUTSIDE
        counts = np.bincount(out["cls"].ravel(), minlength=6)
        print("%s view %d: %d pixels with a peak, %s" % (name, v, has.sum(), dict(zip(MR.CLASS_NAMES, counts.tolist()))))
        assert counts[MR.FLAT] == 0 and counts[MR.OUTSIDE] == 0 and counts[MR.REFINED] > 0 and counts[MR.NO_NEIGHBOUR] > 0


# ---------------------------------------------------------------------------------------------- (b) every class
def test_every_class_occurs_on_the_second_best_peaks():
    """view 0 of mvs_geodesic 40x28x12, every pixel's depth replaced by its second-best peak's where it has one (what the MRF and
    the semi-global stage may pick): 408 pixels, NO_NEIGHBOUR 119, FLAT 12, OUTSIDE 37, REFINED 240, all found"""
    imgs, ocams, op, neigh, depth, peaks = small_geodesic()
    second, replaced = MR.peak_map(peaks, 1)
    assert replaced.sum() > 300
    out = MR.refine_view(imgs, ocams, op, 0, neigh[0], second, count_all=True)
    counts = np.bincount(out["cls"][replaced], minlength=6)
    print("second-best peaks: %d pixels, %s" % (replaced.sum(), dict(zip(MR.CLASS_NAMES, counts.tolist()))))
    assert (out["nmatch"][replaced] == 1).all()
    for k in (MR.NO_NEIGHBOUR, MR.FLAT, MR.OUTSIDE, MR.REFINED):
        assert counts[k] > 0, MR.CLASS_NAMES[k]
    assert counts[MR.NO_WINNER] == 0 and counts[MR.NONE] == 0
    third, replaced3 = MR.peak_map(peaks, 2)
    out3 = MR.refine_view(imgs, ocams, op, 0, neigh[0], third, count_all=True)
    assert replaced3.any() and (out3["nmatch"][replaced3] == 1).all()


def test_no_winner_and_none():
    imgs, ocams, op, neigh, depth, _ = small_geodesic()
    has = np.isfinite(depth) & (depth > 0)
    out = MR.refine_view(imgs, ocams, op, 0, neigh[0], depth * (1.0 + 2.0 ** -40))
    assert (out["cls"][has] == MR.NO_WINNER).all() and (out["cls"][~has] == MR.NONE).all()
    assert np.array_equal(out["depth"].view(np.uint64), (depth * (1.0 + 2.0 ** -40)).view(np.uint64))
    assert (out["win"] == -1).all() and (out["neigh_xy"] == -1).all() and (out["delta"] == 0).all()
    # -1, NaN, +INF inside the mask, and a good depth outside it
    odd = depth.copy()
    ys, xs = np.nonzero(has)
    for k, val in enumerate((-1.0, np.nan, np.inf)):
        odd[ys[k], xs[k]] = val
    mask = imgs[0].mask
    assert (mask != 1).any()
    oy, ox = np.argwhere(mask != 1)[0]
    odd[oy, ox] = depth[has][0]
    out = MR.refine_view(imgs, ocams, op, 0, neigh[0], odd)
    for k in range(3):
        assert out["cls"][ys[k], xs[k]] == MR.NONE
    assert out["cls"][oy, ox] == MR.NONE
    same = (out["depth"].view(np.uint64) == odd.view(np.uint64))
    assert same[out["cls"] != MR.REFINED].all()
    # a second application finds (nearly) no winner: a refined depth is no candidate depth
    first = MR.refine_view(imgs, ocams, op, 0, neigh[0], depth)
    moved = (first["cls"] == MR.REFINED) & (first["delta"] != 0)
    again = MR.refine_view(imgs, ocams, op, 0, neigh[0], first["depth"])
    assert moved.sum() > 100 and (again["cls"][moved] == MR.NO_WINNER).mean() > 0.95


# ---------------------------------------------------------------------------------------------- (c) quality
_PLANE = {}


def plane_reference(weight_kind):
    """the quality scene on the CPU: per view (WTA map, refine_view's dict, depth_errors' dict), computed once"""
    if weight_kind not in _PLANE:
        case = MR.plane_case(weight_kind=weight_kind)
        imgs, ocams, op = cases.oracle_inputs(case)
        neigh = O.mvs_neighbours(ocams, op)
        res = []
        for v in range(3):
            depth, _ = O.mvs_initial_estimate(imgs, ocams, v, neigh[v], op)
            out = MR.refine_view(imgs, ocams, op, v, neigh[v], depth)
            res.append((depth, out, MR.depth_errors(ocams, op, v, neigh[v], depth, out, case["gt_depth"][v])))
        _PLANE[weight_kind] = (case, neigh, res)
    return _PLANE[weight_kind]


@pytest.mark.parametrize("weight_kind", [1, 0], ids=["geodesic", "adaptive"])
def test_refined_depths_are_closer_to_the_truth(weight_kind):
    """A slanted world plane with an analytic texture, three views 64x40 on a semicircle, rendered exactly; D = 24 over
    8.5 .. 11.5, radius 2.  Over the REFINED pixels of each view (1 700 .. 2 250), |z - truth| before -> after:
    GeodesicWeight median 0.113 -> 0.058, 0.136 -> 0.079, 0.106 -> 0.074; RMS over the pixels whose integer error is at most
    half the gap between n- and n+: 0.160 -> 0.094, 0.199 -> 0.131, 0.171 -> 0.123.  AdaptiveWeight median 0.120 -> 0.070,
    0.154 -> 0.085, 0.110 -> 0.081; RMS 0.175 -> 0.120, 0.228 -> 0.162, 0.180 -> 0.138."""
    _, _, res = plane_reference(weight_kind)
    for v, (_, out, e) in enumerate(res):
        print("plane, weights %d, view %d: %s" % (weight_kind, v, e))
        assert 1500 < e["n"] < 2400
        assert e["median_sub"] < e["median_int"]
        assert e["rms_sub"] < e["rms_int"]


# ---------------------------------------------------------------------------------------------- (d) the interface
def test_entry_point_is_exported_bound_and_declared():
    L = capi.lib()
    hdr = open(os.path.join(ROOT, "include", "stereo_recon_hip.h")).read()
    name = "srh_mvs_view_subpixel"
    assert name in capi.EXPORTS and hasattr(L, name)
    assert re.search(r"\bint\s+%s\s*\(" % name, hdr)
    assert "SRH_SUBPX_NO_WINNER = 5" in hdr and capi.SUBPX_NO_WINNER == 5 == MR.NO_WINNER
    assert "typedef struct srh_mvs_subpixel_info" in hdr and '"mvs_subpixel_search"' in hdr
    assert "#define SRH_ABI_VERSION 5" in hdr and L.srh_abi_version() == 5
    assert callable(capi.Context.mvs_view_subpixel)
    assert [f[0] for f in capi.MvsSubpixelInfo._fields_] == ["n_class", "n_moved", "n_fallback"]
    import ctypes
    assert ctypes.sizeof(capi.MvsSubpixelInfo) == 64


def test_host_program_using_the_new_members_builds_and_runs_without_gpu(tmp_path):
    exe = build_host_program(tmp_path)
    assert subprocess.check_output([exe, "defaults"]).split() == [b"5"]
    for path in (os.path.join(HOST, "multiviewstereo.hpp"), os.path.join(ROOT, "stereoreconstruction_amd", "qt", "stereo_qt.hpp")):
        src = open(path).read()
        for member in ("setSubpixel", "subpixel", "subpixelInfo"):
            assert re.search(r"\b%s\(" % member, src), (path, member)
    assert "srh_mvs_view_subpixel" in open(os.path.join(HOST, "sharded.hpp")).read()
