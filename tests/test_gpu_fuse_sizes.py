"""The compaction of srh_mvs_fuse (fuse_scan_kernel, fuse_scatter_kernel, the carry of the points emitted so far from one
list entry to the next) at sizes on the scan's boundaries, against a closed form in numpy (tests/fuse_ref.py,
same_camera_cloud): every slot holds the same pinhole camera and the same smooth depth map, with holes laid out by
blocks of SRH_FUSE_BLOCK pixels -- empty, full and partial blocks, an empty first block, a whole wave of empty runs, a
ragged last block.  tests/test_fuse_host.py checks, without a GPU, that the inputs have those blocks, that a pixel's
point projects into its own pixel, and that the closed form is the restatement's result."""
import numpy as np
import pytest

import cases
import fuse_ref as F
from stereoreconstruction_amd import capi

pytestmark = pytest.mark.gpu


def _upload(ctx, I):
    """The slots' views with the hole-free depth map in slot 0 -> (srh_params, the point of every pixel as
    srh_view_point_cloud makes it); then every slot's own depth map with its holes."""
    case = I["case"]
    cams, p = cases.hip_inputs(case)
    for slot, (rgba, mask, _, _, _) in enumerate(case["views"]):
        ctx.upload_view(slot, rgba, mask, cams[slot])
    ctx.upload_depth(0, I["depth"])
    full = ctx.point_cloud(0, p)
    assert full["n_points"] == I["depth"].size and (full["valid"] == 1).all()
    for slot, d in enumerate(I["depths"]):
        ctx.upload_depth(slot, d)
    return p, full["xyz"]


def _params(min_views):
    return capi.fuse_params(dist_threshold=F.COMPACTION_THR, normal_depth_gap=F.COMPACTION_GAP, min_views=min_views)


@pytest.mark.parametrize("w,h", F.COMPACTION_SIZES, ids=["%dx%d" % s for s in F.COMPACTION_SIZES])
def test_single_view_compaction(hip_ctx, w, h):
    """Each of the two slots alone: the first has a whole wave of empty runs, the second has points in every wave."""
    I = F.compaction_inputs("twin", w, h)
    p, pts = _upload(hip_ctx, I)
    for slot in (0, 1):
        valid = I["valids"][slot]
        pc = hip_ctx.point_cloud(slot, p)
        assert np.array_equal(pc["valid"] == 1, valid)
        assert np.array_equal(pc["xyz"][valid].view(np.uint64), pts[valid].view(np.uint64))
        want = F.same_camera_cloud(pts, [valid], [I["rgbas"][slot]], I["C"], 1)
        got = hip_ctx.mvs_fuse([slot], p, _params(1))
        F.assert_equal(got, want, "slot %d alone, %dx%d" % (slot, w, h), [w * h])
        # the closed form, spelt out: the view's own cloud compacted in pixel order
        idx = np.flatnonzero(valid)
        assert got["n_points"] == idx.size and got["n_claimed"] == 0 and got["n_unsupported"] == 0
        assert np.array_equal(got["src"][:, 0], np.zeros(idx.size, np.int32))
        assert np.array_equal(got["src"][:, 1], idx.astype(np.int32))
        assert np.array_equal(got["xyz"].view(np.uint64), pc["xyz"].reshape(-1, 3)[idx].view(np.uint64))
        assert np.array_equal(got["rgb"], pc["rgb"].reshape(-1, 3)[idx])
        assert np.all(got["nviews"] == 1)
        assert np.all((got["normals"] * (I["C"][None, :] - got["xyz"])).sum(1) > 0)


@pytest.mark.parametrize("min_views", [1, 2])
def test_twin_views_compaction(hip_ctx, min_views):
    """Two slots with the same camera: the second entry's points lie behind the first's, on a base of hundreds of blocks."""
    w, h = F.TWIN_SIZE
    I = F.compaction_inputs("twin", w, h)
    p, pts = _upload(hip_ctx, I)
    want = F.same_camera_cloud(pts, I["valids"], I["rgbas"], I["C"], min_views)
    got = hip_ctx.mvs_fuse([0, 1], p, _params(min_views))
    F.assert_equal(got, want, "twin views, min_views %d" % min_views, [w * h, w * h])
    # the closed form, spelt out
    v0, v1 = (v.ravel() for v in I["valids"])
    both = int((v0 & v1).sum())
    assert got["n_claimed"] == both
    flat = pts.reshape(-1, 3)
    c0, c1 = (im.reshape(-1, 4)[:, :3].astype(np.int64) for im in I["rgbas"])
    if min_views == 1:
        i0, i1 = np.flatnonzero(v0), np.flatnonzero(v1 & ~v0)
        assert np.array_equal(got["src"], np.concatenate([np.stack([0 * i0, i0], 1), np.stack([0 * i1 + 1, i1], 1)]).astype(np.int32))
        assert np.array_equal(got["nviews"], np.concatenate([1 + v1[i0], np.ones(i1.size, np.int64)]).astype(np.uint8))
        assert np.array_equal(got["xyz"].view(np.uint64), np.concatenate([flat[i0], flat[i1]]).view(np.uint64))
        rgb0 = np.where(v1[i0][:, None], (2 * (c0[i0] + c1[i0]) + 2) // 4, c0[i0])
        assert np.array_equal(got["rgb"], np.concatenate([rgb0, c1[i1]]).astype(np.uint8))
        assert got["n_unsupported"] == 0
    else:
        i0 = np.flatnonzero(v0 & v1)
        assert np.array_equal(got["src"], np.stack([0 * i0, i0], 1).astype(np.int32))
        assert np.all(got["nviews"] == 2)
        assert np.array_equal(got["xyz"].view(np.uint64), flat[i0].view(np.uint64))
        assert np.array_equal(got["rgb"], ((2 * (c0[i0] + c1[i0]) + 2) // 4).astype(np.uint8))
        assert got["n_unsupported"] == int(v0.sum() + v1.sum()) - 2 * both


def test_sixty_four_entries():
    """SRH_MAX_VIEWS list entries, every one a member of every point: the view count, the colour sums and the sequential
    mean over 64 members.  In a context of its own: other tests count on the session's context having empty slots."""
    w, h = F.MANY_SIZE
    n = F.MANY_VIEWS
    assert n == capi.MAX_VIEWS
    I = F.compaction_inputs("many", w, h)
    with capi.Context(0) as ctx:
        p, pts = _upload(ctx, I)
        got = ctx.mvs_fuse(list(range(n)), p, _params(2))
        # one more entry than the ABI allows is refused
        with pytest.raises(capi.StereoHipError) as e:
            ctx.mvs_fuse(list(range(n)) + [0], p, _params(2))
        assert e.value.code == capi.SRH_E_INVALID
    want = F.same_camera_cloud(pts, I["valids"], I["rgbas"], I["C"], 2)
    F.assert_equal(got, want, "64 entries", [w * h] * n)
    # the closed form, spelt out
    assert got["n_points"] == w * h and got["n_claimed"] == (n - 1) * w * h and got["n_unsupported"] == 0
    assert np.array_equal(got["src"], np.stack([np.zeros(w * h), np.arange(w * h)], 1).astype(np.int32))
    assert np.all(got["nviews"] == n)
    acc = pts.reshape(-1, 3).copy()
    for _ in range(n - 1):
        acc = acc + pts.reshape(-1, 3)
    assert np.array_equal(got["xyz"].view(np.uint64), (acc / float(n)).view(np.uint64))
    col = sum(im.reshape(-1, 4)[:, :3].astype(np.int64) for im in I["rgbas"])
    assert np.array_equal(got["rgb"], ((2 * col + n) // (2 * n)).astype(np.uint8))
