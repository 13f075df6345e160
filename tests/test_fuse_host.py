"""Depth-map fusion without a GPU: the C-ABI's host-side pieces, and the CPU restatement (tests/fuse_ref.py) on the very
inputs tests/test_gpu_fuse.py compares the device with -- so that those comparisons cannot be vacuous or hinge on a
last bit -- plus the structural properties of the rule."""
import os
import re

import numpy as np
import pytest

import fuse_ref as F
from stereoreconstruction_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuse_params_defaults():
    f = capi.FuseParams(1.0, 2.0, 7, 9)
    capi.lib().srh_fuse_params_defaults(f)
    assert (f.dist_threshold, f.normal_depth_gap, f.min_views, f.flags) == (0.0, 0.0, 2, 0)
    g = capi.fuse_params(min_views=3, dist_threshold=0.5)
    assert (g.dist_threshold, g.normal_depth_gap, g.min_views, g.flags) == (0.5, 0.0, 3, 0)
    with pytest.raises(AttributeError):
        capi.fuse_params(nonsense=1)


def test_header_declares_the_entry_points_and_the_abi_stays():
    text = open(os.path.join(ROOT, "include", "stereo_recon_hip.h")).read()
    for name in ("srh_fuse_params_defaults", "srh_mvs_fuse", "srh_mvs_fused_count", "srh_mvs_fused_download",
                 "srh_mvs_fused_device"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)
    assert "typedef struct srh_fuse_params" in text and "typedef struct srh_fuse_info" in text
    assert re.search(r"#define\s+SRH_ABI_VERSION\s+5\b", text)
    assert capi.lib().srh_abi_version() == 5
    import ctypes
    assert ctypes.sizeof(capi.FuseParams) == 24 and ctypes.sizeof(capi.FuseInfo) == 40


@pytest.mark.parametrize("name", F.FUSE_CASES)
def test_gpu_inputs_are_not_vacuous(name):
    r = F.case_result(name)
    assert r["n_points"] > 0 and r["n_claimed"] > 0 and r["n_unsupported"] > 0
    has = r["flags"] & 1
    assert (has == 0).sum() >= 1 and has.sum() > r["n_points"] // 2
    assert r["n_normals"] == int(has.sum())
    # the device's decisions must not hinge on a last bit: no member test near the threshold, no orientation test near 0
    assert r["member_margin"] >= 1e-9
    assert r["orient_margin"] >= 1e-6
    # every kind of hole is in the inputs
    I = F.case_inputs(name)
    D = np.concatenate([d.ravel() for d in I["depths"]])
    M = np.concatenate([m.ravel() for m in I["masks"]])
    assert np.isnan(D).any() and np.isposinf(D).any() and (D == -1).any() and (M == 0).any()


@pytest.mark.parametrize("name", F.FUSE_CASES)
def test_structure_of_the_rule(name):
    r = F.case_result(name)
    assert r["n_candidates"] == r["n_points"] + r["n_claimed"] + r["n_unsupported"]
    n = len(r["claimed"])
    I = F.case_inputs(name)
    widths = [m.shape[1] for m in I["masks"]]
    # no pixel both emitted and claimed; no source twice; ascending (view, pixel)
    for v, i in r["src"]:
        assert not r["claimed"][v][i // widths[v], i % widths[v]]
    keys = r["src"][:, 0].astype(np.int64) << 32 | r["src"][:, 1]
    assert np.all(np.diff(keys) > 0)
    assert r["nviews"].min() >= 2 and r["nviews"].max() <= n
    # nothing of the first entry is ever claimed, and its emitted points carry its index
    assert not r["claimed"][0].any()


@pytest.mark.parametrize("name", ["mvs_geodesic", "mvs_mixed_sizes"])
def test_list_order_decides_the_owners_not_the_coverage(name):
    n = len(F.case_inputs(name)["ocams"])
    rev = tuple(reversed(range(n)))
    a, b = F.case_result(name), F.case_result(name, order=rev)
    owners_a = {(int(v), int(i)) for v, i in a["src"]}
    owners_b = {(rev[int(v)], int(i)) for v, i in b["src"]}          # back to view indices
    assert owners_a != owners_b
    # with min_views = 1 every pixel with a point is emitted or claimed, whatever the order
    a1, b1 = F.case_result(name, min_views=1), F.case_result(name, order=rev, min_views=1)
    assert a1["n_unsupported"] == 0 and b1["n_unsupported"] == 0

    def covered(r, order):
        out = set()
        for v, i in r["src"]:
            out.add((order[int(v)], int(i)))
        for k, c in enumerate(r["claimed"]):
            w = c.shape[1]
            for y, x in np.argwhere(c):
                out.add((order[k], int(y) * w + int(x)))
        return out
    assert covered(a1, tuple(range(n))) == covered(b1, rev)
    assert len(covered(a1, tuple(range(n)))) == a1["n_candidates"]


# ---------------------------------------------------------------- the inputs of the larger and the optional GPU cases

def _margins_and_branches(r):
    assert r["n_points"] > 0 and r["n_claimed"] > 0 and r["n_unsupported"] > 0
    has = r["flags"] & 1
    assert (has == 0).sum() >= 1 and has.sum() >= 1 and r["n_normals"] == int(has.sum())
    assert r["member_margin"] >= 1e-9
    assert r["orient_margin"] >= 1e-6
    assert r["gap_margin"] >= 1e-9
    assert r["n_candidates"] == r["n_points"] + r["n_claimed"] + r["n_unsupported"]


def test_fuse_block_is_what_the_sizes_were_chosen_for():
    text = open(os.path.join(ROOT, "stereoreconstruction_amd", "csrc", "srh_internal.hpp")).read()
    m = re.search(r"^#define\s+SRH_FUSE_BLOCK\s+(\d+)\s*$", text, re.M)
    assert m and int(m.group(1)) == F.FUSE_BLOCK == 256
    assert re.search(r"enum\s*\{\s*SRH_MAX_VIEWS\s*=\s*64\s*\}", open(os.path.join(ROOT, "include", "stereo_recon_hip.h")).read())
    assert F.MANY_VIEWS == capi.MAX_VIEWS == 64
    # (blocks, blocks per run of a thread of the scan, runs): the boundaries at 256 and 512 blocks, crossed by one
    assert F.scan_layout(56 * 40) == (9, 1, 9)                          # the largest view of the small cases
    assert [F.scan_layout(w * h) for w, h in F.COMPACTION_SIZES] == [(256, 1, 256), (257, 2, 129), (514, 3, 172)]
    assert 363 * 362 % F.FUSE_BLOCK == 78 and 257 % 2 == 1 and 514 % 3 == 1   # a ragged last block; ragged last runs
    assert F.scan_layout(F.TWIN_SIZE[0] * F.TWIN_SIZE[1]) == (257, 2, 129)
    assert [F.scan_layout(o["w"] * o["h"]) for _, o in F.FUSE_SIZE_CASES] == [(257, 2, 129), (513, 3, 171)]
    assert F.scan_layout(1280 * 960) == (4800, 19, 253)                 # (timed in profiles/, compared nowhere)


# (points, claimed, unsupported, empty blocks per view) of the restatement
SIZE_CASE_FACTS = {"mvs_distorted": (18660, 16623, 8898, [53, 64]), "mvs_geodesic": (38046, 34087, 17647, [117, 198])}


@pytest.mark.parametrize("name,over", F.FUSE_SIZE_CASES, ids=[c[0] for c in F.FUSE_SIZE_CASES])
def test_size_cases_cross_the_scans_boundaries(name, over):
    I = F.case_inputs(name, **over)
    r = F.case_result(name, **over)
    _margins_and_branches(r)
    assert has_every_hole(I)
    points, claimed, unsupported, empty = SIZE_CASE_FACTS[name]
    assert (r["n_points"], r["n_claimed"], r["n_unsupported"]) == (points, claimed, unsupported)
    # what the views emit, block by block: empty and partial blocks (the hole lattice leaves no full
    # one), and points in more than one wave of the scan
    for v, m in enumerate(I["masks"]):
        nb, per, runs = F.scan_layout(m.size)
        emitted = np.zeros(m.size, dtype=bool)
        emitted[r["src"][r["src"][:, 0] == v, 1]] = True
        counts = F.block_counts(emitted)
        assert counts.size == nb and int((counts == 0).sum()) == empty[v]
        assert ((counts > 0) & (counts < F.FUSE_BLOCK)).any()
        wave_of_block = np.arange(nb) // per // 64
        assert {0, 1} <= set(wave_of_block[counts > 0].tolist())          # (the sphere leaves the image's last rows empty)
    print("%s %s: member margin %.3g orientation margin %.3g gap margin %.3g"
          % (name, over, r["member_margin"], r["orient_margin"], r["gap_margin"]))


def has_every_hole(I):
    D = np.concatenate([d.ravel() for d in I["depths"]])
    M = np.concatenate([m.ravel() for m in I["masks"]])
    return np.isnan(D).any() and np.isposinf(D).any() and (D == -1).any() and (M == 0).any()


def test_min_views_three_and_four():
    r2, r3, r4 = (F.case_result("mvs_geodesic", min_views=k) for k in (2, 3, 4))
    for r in (r3, r4):
        _margins_and_branches(r)
    assert r3["n_points"] == 865 and np.bincount(r3["nviews"], minlength=5).tolist() == [0, 0, 0, 365, 500]
    assert r4["n_points"] == 556 and (r4["nviews"] == 4).all()
    assert r2["n_points"] > r3["n_points"]


def test_explicit_gaps_thin_the_normals():
    I = F.case_inputs("mvs_geodesic")
    g0 = F.default_gap(I["op"])
    assert abs(g0 - 0.2609) < 5e-5
    r0 = F.case_result("mvs_geodesic")
    assert (r0["n_points"], r0["n_normals"]) == (1078, 964) and r0["gap_margin"] >= 1e-9
    for fraction, normals in zip(F.GAP_FRACTIONS, (462, 69)):
        r = F.case_result("mvs_geodesic", gap=g0 / fraction)
        _margins_and_branches(r)
        assert (r["n_points"], r["n_normals"]) == (1078, normals)
        for k in ("src", "nviews", "rgb", "xyz"):                        # the gap decides normals only
            assert r[k].tobytes() == r0[k].tobytes()
        print("gap g0/%d: gap margin %.3g" % (fraction, r["gap_margin"]))


def test_mixed_size_orders():
    points = {}
    for over, order in F.MIXED_ORDERS:
        I = F.case_inputs("mvs_mixed_sizes", **over)
        blocks = [F.scan_layout(m.size)[0] for m in I["masks"]]
        assert blocks[0] == max(blocks) and order[0] != 0               # the largest view is not the first entry
        r = F.case_result("mvs_mixed_sizes", order=order, **over)
        _margins_and_branches(r)
        assert sorted(set(r["src"][:, 0].tolist())) == [0, 1, 2]         # every entry emits
        points[(tuple(sorted(over.items())), order)] = (blocks, r["n_points"])
        print("mixed sizes %s order %s: blocks %s, %s, margins %.3g %.3g %.3g" % (
            over, order, blocks, {k: r[k] for k in F.COUNTERS}, r["member_margin"], r["orient_margin"], r["gap_margin"]))
    assert [points[((), o)] for o in ((2, 1, 0), (1, 2, 0), (1, 0, 2))] == [([9, 7, 7], 784), ([9, 7, 7], 720), ([9, 7, 7], 719)]
    big = (("h", 80), ("w", 120))
    assert points[(big, (2, 1, 0))][0] == points[(big, (1, 0, 2))][0] == [38, 34, 33]   # three different block counts


# ---------------------------------------------------------------- the compaction inputs and their closed form

def _oracle_points(I):
    return F.point_map(I["ocams"][0], I["op"], I["depth"], I["masks"][0])


@pytest.mark.parametrize("w,h", [F.TWIN_SIZE, F.MANY_SIZE], ids=["twin", "many"])
def test_a_point_projects_into_its_own_pixel(w, h):
    """What the closed form rests on: with the same camera in every slot, the point of pixel (x, y) projects into pixel
    (x, y), and no rounding can move it out: the fraction stays inside [0.25, 0.75]."""
    I = F.compaction_inputs("twin" if (w, h) == F.TWIN_SIZE else "many", w, h)
    pts, valid = _oracle_points(I)
    assert valid.all()
    L = F.O.lib()
    q = np.zeros(3)
    s = I["op"].image_scale
    for y in range(h):
        for x in range(w):
            q[:] = pts[y, x]
            assert L.sro_project(I["ocams"][0], F.O.dptr(q))
            x2, y2 = float(q[0]) * s, float(q[1]) * s
            assert (int(x2), int(y2)) == (x, y) and 0.25 <= x2 - x <= 0.75 and 0.25 <= y2 - y <= 0.75, (x, y, x2, y2)


@pytest.mark.parametrize("w,h", F.COMPACTION_SIZES, ids=["%dx%d" % s for s in F.COMPACTION_SIZES])
def test_compaction_inputs_have_the_blocks_they_promise(w, h):
    I = F.compaction_inputs("twin", w, h)
    assert np.isfinite(I["depth"]).all() and all((m == 1).all() for m in I["masks"])
    assert F.COMPACTION_GAP > I["op"].max_depth - I["op"].min_depth
    pts, _ = _oracle_points(I)
    # the second slot alone: points in every wave of the scan
    other = F.same_camera_cloud(pts, I["valids"][1:], I["rgbas"][1:], I["C"], 1)
    assert other["orient_margin"] >= 1e-6 and 0 < other["n_normals"] < other["n_points"]
    runs_with_points = np.unique(other["src"][:, 1] // F.FUSE_BLOCK // F.scan_layout(w * h)[1])
    assert set((runs_with_points // 64).tolist()) == set(range((F.scan_layout(w * h)[2] + 63) // 64))
    # the first slot alone
    want = F.same_camera_cloud(pts, I["valids"][:1], I["rgbas"][:1], I["C"], 1)
    assert want["orient_margin"] >= 1e-6
    nb, per, runs = F.scan_layout(w * h)
    emitted = np.zeros(w * h, dtype=bool)
    emitted[want["src"][:, 1]] = True
    assert np.array_equal(emitted, I["valids"][0].ravel()) and (want["src"][:, 0] == 0).all()
    counts = F.block_counts(emitted)
    assert counts.size == nb
    n_empty, n_full = int((counts == 0).sum()), int((counts == F.FUSE_BLOCK).sum())
    n_partial = nb - n_empty - n_full
    assert n_empty >= 64 * per + 10 and n_full >= 10 and n_partial >= 10
    assert counts[0] == 0 and counts[1] == F.FUSE_BLOCK and 0 < counts[2] < F.FUSE_BLOCK
    # a whole wave of the scan (64 consecutive runs of `per` blocks) without a point, waves with points on both sides
    run_sums = np.zeros(runs * per, dtype=np.int64)
    run_sums[:nb] = counts
    run_sums = run_sums.reshape(runs, per).sum(1)
    assert (run_sums[64:128] == 0).all() and run_sums[:64].any() and run_sums[128:].any()
    assert set((np.flatnonzero(run_sums) // 64).tolist()) == set(range((runs + 63) // 64)) - {1}
    # the last block is not empty; it is ragged where the size gives one, and so is the last run
    last = w * h - (nb - 1) * F.FUSE_BLOCK
    assert 0 < counts[-1] < last
    if (w, h) == (363, 362):
        assert last == 78
    if per > 1:
        assert nb - (runs - 1) * per < per
    # both kinds of point, and every combination of usable neighbours
    assert 0 < want["n_normals"] < want["n_points"]
    print("slot 0 alone %dx%d: %d blocks, per %d; %d empty, %d full, %d partial; %s; orientation margin %.3g"
          % (w, h, nb, per, n_empty, n_full, n_partial, {k: want[k] for k in F.COUNTERS}, want["orient_margin"]))
    print("slot 1 alone %dx%d: %s; orientation margin %.3g" % (w, h, {k: other[k] for k in F.COUNTERS}, other["orient_margin"]))


def test_twin_inputs():
    w, h = F.TWIN_SIZE
    I = F.compaction_inputs("twin", w, h)
    v0, v1 = (v.ravel() for v in I["valids"])
    assert not np.array_equal(I["rgbas"][0], I["rgbas"][1])
    pts, _ = _oracle_points(I)
    for min_views in (1, 2):
        r = F.same_camera_cloud(pts, I["valids"], I["rgbas"], I["C"], min_views)
        assert r["orient_margin"] >= 1e-6 and 0 < r["n_normals"] < r["n_points"]
        assert r["n_claimed"] == int((v0 & v1).sum()) > 1000
        print("twin min_views %d: %s; orientation margin %.3g" % (min_views, {k: r[k] for k in F.COUNTERS}, r["orient_margin"]))
    # the second entry's points start on top of hundreds of the first's blocks, and lie in more than 100 blocks themselves
    r = F.same_camera_cloud(pts, I["valids"], I["rgbas"], I["C"], 1)
    first_of_1 = int(np.flatnonzero(r["src"][:, 0] == 1)[0])
    assert first_of_1 == int(v0.sum()) > 10000
    assert int((F.block_counts(v1 & ~v0) > 0).sum()) > 100 and int((F.block_counts(v0) > 0).sum()) > 64
    assert {1, 2} == set(r["nviews"][:first_of_1].tolist()) and (r["nviews"][first_of_1:] == 1).all()


def test_closed_form_is_the_restatement():
    """same_camera_cloud against fuse() on inputs of its own kind small enough for the per-pixel restatement: two slots
    with holes (min_views 1 and 2) and the 64 slots of the GPU test."""
    for kind, (w, h), all_min_views in (("twin", (48, 40), (1, 2)), ("many", F.MANY_SIZE, (2,))):
        I = F.compaction_inputs(kind, w, h)
        pts, _ = _oracle_points(I)
        for min_views in all_min_views:
            want = F.fuse(I["ocams"], I["op"], I["rgbas"], I["masks"], I["depths"], F.COMPACTION_THR, gap=F.COMPACTION_GAP,
                          min_views=min_views)
            assert want["member_margin"] == 1.0 and want["gap_margin"] > 0.9 and want["n_points"] > 0
            got = F.same_camera_cloud(pts, I["valids"], I["rgbas"], I["C"], min_views)
            F.assert_equal(got, want, "%s, min_views %d" % (kind, min_views), [w * h] * len(I["valids"]))
            assert got["orient_margin"] <= want["orient_margin"] + 1e-12   # (over every pixel with a point, emitted or not)
    assert want["n_points"] == 256 and (want["nviews"] == 64).all() and want["n_claimed"] == 63 * 256
