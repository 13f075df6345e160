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
