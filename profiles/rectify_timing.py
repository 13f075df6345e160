"""Times rectification (srh_twoview_rectify, srh_view_depth_unrectify) with srh_profile_*:
  - the two warps and one unrectify of a verged, distorted 1920x1080 pair (the kernels' device events and the calls' wall
    time, which includes the installs of the two rectified views: their derived planes, the mask's copy to the host);
  - the example project's pair (tests/golden/bunny_pair.npz, 256x192, 100 levels): srh_twoview_compute on the views as they
    are (candidate-list kernels) against srh_twoview_compute on the rectified views (the dense plan), with the rectify in
    front and the two unrectifies behind it counted on the rectified side.
usage: python3 profiles/rectify_timing.py [small]      (from the repository root)"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from stereoreconstruction_amd import capi, synthetic

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
REPEATS = 3


def _rot(ax, a):
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[ax]


def verged_pair(w, h):
    """the verged, distorted rig of tests/cases.py on a synthetic pair of w x h"""
    L, R, ml, mr, _ = synthetic.rectified_pair(w, h, 64, 0x5EED0D00)
    (K, _, _), _ = synthetic.rectified_cameras(w, h)
    Rl, Rr = _rot("y", 0.03), _rot("z", 0.05) @ _rot("x", 0.02) @ _rot("y", -0.04)
    cams = [capi.camera_from_krt(K, Rl, np.zeros(3), np.array([-0.131, 0.4, 0.004, 0.003, -0.6])),
            capi.camera_from_krt(K, Rr, -Rr @ np.array([1.0, 0.03, 0.02]), np.array([-0.058, -0.2, 0.0, 0.006, 0.3]))]
    zmin, zmax = synthetic.rectified_depth_range(w, 64)
    return [(L, ml), (R, mr)], cams, capi.params_twoview(min_depth=zmin, max_depth=zmax, num_depth_levels=64)


def bunny_pair():
    g = np.load(os.path.join(ROOT, "tests", "golden", "bunny_pair.npz"))
    views = [(g[t + "_rgba"], g[t + "_mask"]) for t in ("left", "right")]
    cams = [capi.camera_from_krt(g[t + "_K"], g[t + "_R"], g[t + "_t"], g[t + "_dist"]) for t in ("left", "right")]
    return views, cams, capi.params_twoview(min_depth=30.0, max_depth=80.0, num_depth_levels=100, image_scale=float(g["scale"][0]))


def profiled(ctx, fn):
    ctx.synchronize()
    ctx.profile_reset(); ctx.profile_enable(True)
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    prof = ctx.profile()
    ctx.profile_enable(False)
    return out, wall, prof


def warp_times(small):
    w, h = (480, 270) if small else (1920, 1080)
    views, cams, p = verged_pair(w, h)
    print("verged, distorted pair %dx%d" % (w, h))
    with capi.Context(0) as ctx:
        for s in (0, 1):
            ctx.upload_view(s, views[s][0], views[s][1], cams[s])
        ctx.twoview_rectify(0, 1, 2, 3, p)                               # warm: the kernels' code is on the device, the slots exist
        ctx.depth_unrectify(2, 0, p)
        runs = []
        for _ in range(REPEATS):
            info, wall_r, prof = profiled(ctx, lambda: ctx.twoview_rectify(0, 1, 2, 3, p))
            warp = prof["rectify_warp_kernel"]
            ctx.upload_depth(2, np.full((h, w), 10.0))
            _, wall_u, prof = profiled(ctx, lambda: ctx.depth_unrectify(2, 0, p))
            runs.append((warp[0], wall_r, prof["unrectify_kernel"][0], wall_u))
        print("  runs (ms): " + "; ".join("warps %.3f (call %.2f) unrectify %.3f (call %.2f)" % r for r in runs))
        best = [min(r[k] for r in runs) for k in range(4)]
        print("  two warps        : %8.3f ms in %d kernels (srh_twoview_rectify: %.2f ms wall with both installs)" % (best[0], warp[1], best[1]))
        print("  one unrectify    : %8.3f ms (srh_view_depth_unrectify: %.2f ms wall)" % (best[2], best[3]))
        print("  WHITE            : %d and %d of %d; axes turned by %.4f and %.4f rad" % (info["white_a"], info["white_b"], w * h, info["angle_a"], info["angle_b"]))


def bunny_times():
    views, cams, p = bunny_pair()
    h, w = views[0][1].shape
    print("bunny pair %dx%d, %d levels" % (w, h, p.num_depth_levels))
    with capi.Context(0) as ctx:
        for s in (0, 1):
            ctx.upload_view(s, views[s][0], views[s][1], cams[s])

        def plain():
            return ctx.twoview_compute(0, 1, p)

        def rectified():
            ctx.twoview_rectify(0, 1, 2, 3, p)
            ctx.twoview_compute(2, 3, p)
            dense = ctx.stats()["used_dense_path"]
            ctx.depth_unrectify(2, 0, p)
            ctx.depth_unrectify(3, 1, p)
            return dense

        def compute_only():
            return ctx.twoview_compute(2, 3, p)

        plain(); plain()                                                  # warm; the list capacities are learnt
        t_plain = []
        for _ in range(REPEATS):
            _, wall, _ = profiled(ctx, plain)
            t_plain.append(wall)
        assert not ctx.stats()["used_dense_path"]
        rectified(); rectified()
        t_rect, t_comp = [], []
        for _ in range(REPEATS):
            dense, wall, _ = profiled(ctx, rectified)
            assert dense
            t_rect.append(wall)
            _, wall, _ = profiled(ctx, compute_only)
            t_comp.append(wall)
        print("  runs (ms, wall, profiling on): lists %s; rectify + dense + unrectify %s; dense compute alone %s"
              % tuple(" ".join("%.2f" % t for t in ts) for ts in (t_plain, t_rect, t_comp)))
        print("  srh_twoview_compute, views as they are (lists)   : %8.2f ms" % min(t_plain))
        print("  srh_twoview_compute, rectified views (dense plan): %8.2f ms" % min(t_comp))
        print("  rectify + compute + two unrectifies              : %8.2f ms" % min(t_rect))


if __name__ == "__main__":
    small = len(sys.argv) > 1 and sys.argv[1] == "small"
    warp_times(small)
    bunny_times()
