"""Option "subpixel" without a device: the CPU reference of tests/subpixel_ref.py against the oracle, the classes of the
definition on the class scene, what the refinement buys on a slanted plane, and the interface -- exports, header, bindings
and a program using the host class's new members (tests/test_gpu_subpixel.py runs it on the device)."""
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import subpixel_ref as SR
from stereoreconstruction_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "stereoreconstruction_amd", "host")
LIBDIR = os.path.join(ROOT, "stereoreconstruction_amd")
NAMES = ("srh_view_subpixel", "srh_view_subpixel_device", "srh_view_subpixel_info")
CASES = ["geodesic_r2", "adaptive_masks", "geodesic_verged_dist_masks", "adaptive_refractive", "geodesic_scaled"]
DIRECTIONS = ((0, 1), (1, 0))


def build_host_program(out_dir):
    """tests/host_subpixel_test.cpp against the host library and libstereo_recon_hip -> path of the program"""
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    exe = os.path.join(str(out_dir), "host_subpixel_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + HOST,
                           os.path.join(ROOT, "tests", "host_subpixel_test.cpp"),
                           os.path.join(HOST, "libstereo_recon_host.a"),
                           "-L" + LIBDIR, "-lstereo_recon_hip", "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


# ---------------------------------------------------------------------------------------------- (a) the recomposed depth
@pytest.mark.parametrize("name", CASES)
def test_recomposed_candidate_depth_is_the_oracles_wta_depth(name):
    """candidate_depth put together from sro_unproject and sro_closest_points equals sro_twoview_wta's depth bit for bit on
    every pixel with a finite depth, and the curve's neighbours of a winner are few: never above 2 on these cases"""
    case = cases.get_twoview(name)
    imgs, ocams, op = cases.oracle_inputs(case)
    for ref, oth in DIRECTIONS:
        depth, diag, out = SR.reference_pass(imgs, ocams, op, ref, oth)
        ys, xs = np.nonzero(np.isfinite(depth))
        assert len(ys) > 0
        for y, x in zip(ys, xs):
            cx, cy = (int(v) for v in diag["win_xy"][y, x])
            z = SR.candidate_depth(ocams[ref], ocams[oth], op, int(x), int(y), cx, cy)
            assert z == depth[y, x], "%s %d>%d (%d,%d): %r / %r" % (name, ref, oth, x, y, z, depth[y, x])
        # the definition's invariants on the reference's own output
        refined = out["cls"] == SR.REFINED
        assert refined.any() and (out["cls"] == SR.NO_NEIGHBOUR).any()
        assert (out["delta"][~refined] == 0).all() and (np.abs(out["delta"]) <= 0.5).all()
        moved = refined & (out["delta"] != 0)
        same = out["depth"].view(np.uint64) == depth.view(np.uint64)
        assert same[~moved].all(), "a pixel that is not refined keeps its depth's bits"
        assert np.array_equal(np.isfinite(out["depth"]), np.isfinite(depth))
        # a refined depth lies between the winner's and the chosen neighbour's
        for y, x in np.argwhere(moved):
            n = out["neigh_xy"][y, x, 2:4] if out["delta"][y, x] > 0 else out["neigh_xy"][y, x, 0:2]
            zn = SR.candidate_depth(ocams[ref], ocams[oth], op, int(x), int(y), int(n[0]), int(n[1]))
            lo, hi = sorted((depth[y, x], zn))
            assert lo <= out["depth"][y, x] <= hi, (name, ref, x, y)


# ---------------------------------------------------------------------------------------------- (b) the class scene
def test_every_class_occurs_on_the_class_scene():
    """slanted plane, 64x40, D = 16, radius 2, AdaptiveWeight, 40 % of the rows flat.  Pass 1>0: NO_NEIGHBOUR 389, FLAT 603,
    OUTSIDE 9, REFINED 1228 (4 of them with delta == 0); pass 0>1: NO_NEIGHBOUR 956, OUTSIDE 7, REFINED 1310."""
    case = SR.slanted_case(weight_kind=0, radius=2, flat_frac=0.4)
    imgs, ocams, op = cases.oracle_inputs(case)
    seen = np.zeros(5, np.int64)
    zero = 0
    for ref, oth in DIRECTIONS:
        _, _, out = SR.reference_pass(imgs, ocams, op, ref, oth)
        counts = np.bincount(out["cls"].ravel(), minlength=5)
        print("class scene %d>%d: %s" % (ref, oth, dict(zip(SR.CLASS_NAMES, counts.tolist()))))
        seen += counts
        zero += int(((out["cls"] == SR.REFINED) & (out["delta"] == 0)).sum())
    assert (seen > 0).all(), dict(zip(SR.CLASS_NAMES, seen.tolist()))
    assert zero > 0


# ---------------------------------------------------------------------------------------------- (c) quality
@pytest.mark.parametrize("weight_kind,radius", [(1, 5), (0, 2)])
def test_refined_disparities_are_closer_to_the_truth(weight_kind, radius):
    """Slanted plane d = 10.3 + 0.06 x + 0.05 y with an analytic texture, 64x40x16.  Over the REFINED pixels, integer ->
    sub-pixel: GeodesicWeight radius 5: median 0.250 -> 0.066 (0>1), 0.245 -> 0.048 (1>0), inlier RMS 0.300 -> 0.109,
    0.297 -> 0.075; AdaptiveWeight radius 2: median 0.250 -> 0.094, 0.245 -> 0.087, RMS 0.300 -> 0.151, 0.303 -> 0.147."""
    case = SR.slanted_case(weight_kind=weight_kind, radius=radius)
    imgs, ocams, op = cases.oracle_inputs(case)
    for ref, oth in DIRECTIONS:
        depth, _, out = SR.reference_pass(imgs, ocams, op, ref, oth)
        e = SR.disparity_errors(depth, out["depth"], out["cls"], 64, ref)
        print("slanted, weights %d radius %d, %d>%d: %s" % (weight_kind, radius, ref, oth, e))
        assert e["n"] > 1000
        assert e["median_sub"] < e["median_int"] and e["rms_sub"] < e["rms_int"]


# ---------------------------------------------------------------------------------------------- (d) the interface
def test_entry_points_are_exported_bound_and_declared():
    L = capi.lib()
    hdr = open(os.path.join(ROOT, "include", "stereo_recon_hip.h")).read()
    for name in NAMES:
        assert name in capi.EXPORTS, name
        assert hasattr(L, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    assert (capi.SUBPX_NONE, capi.SUBPX_NO_NEIGHBOUR, capi.SUBPX_FLAT, capi.SUBPX_OUTSIDE, capi.SUBPX_REFINED) == (0, 1, 2, 3, 4)
    assert (SR.NONE, SR.NO_NEIGHBOUR, SR.FLAT, SR.OUTSIDE, SR.REFINED) == (0, 1, 2, 3, 4)
    for k, name in enumerate(("NONE", "NO_NEIGHBOUR", "FLAT", "OUTSIDE", "REFINED")):
        assert "SRH_SUBPX_%s = %d" % (name, k) in hdr
    assert callable(capi.Context.subpixel) and callable(capi.Context.subpixel_device) and callable(capi.Context.subpixel_info)


def test_header_names_the_option_and_keeps_the_abi_version():
    hdr = open(os.path.join(ROOT, "include", "stereo_recon_hip.h")).read()
    assert "#define SRH_ABI_VERSION 5" in hdr
    assert capi.lib().srh_abi_version() == 5
    entry = hdr[hdr.index(' *   "subpixel"'):]
    assert "CHANGES RESULTS" in entry[:120]
    # the "wta_outputs" entry keeps its wording
    assert ' *   "wta_outputs"     never changes a depth map.  0 (default): a WTA pass keeps the depth only' in hdr


def test_host_program_using_the_new_members_compiles_without_gpu(tmp_path):
    exe = build_host_program(tmp_path)
    assert os.path.exists(exe)
    src = open(os.path.join(ROOT, "tests", "host_subpixel_test.cpp")).read()
    for member in ("setSubpixel", "subpixel", "leftSubpixelDelta", "rightSubpixelDelta"):
        assert member + "(" in src, member
    qt = open(os.path.join(ROOT, "stereoreconstruction_amd", "qt", "stereo_qt.hpp")).read()
    for member in ("setSubpixel", "subpixel", "leftSubpixelDelta", "rightSubpixelDelta"):
        assert re.search(r"\b%s\(" % member, qt), member
