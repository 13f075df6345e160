"""Times depth-map fusion (srh_mvs_fuse) with srh_profile_* next to the cross-check chain on the same depth maps:
the C4 rig (8 views 1280x960 on a semicircle around the textured sphere) and the eight bunny views of the fixture, each
after the initial estimates.  The chain is the yardstick: a fusion launch does per pixel what a cross-check launch does
without its early exit, plus the compaction, so (nviews - 1) x the chain's time is the reference for the fusion's.
usage: python3 profiles/fuse_timing.py [small]      (from the repository root)"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from stereoreconstruction_amd import capi, synthetic

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
REPEATS = 3
FUSE_KERNELS = ("point_cloud_kernel", "fuse_view_kernel", "fuse_scan_kernel", "fuse_scatter_kernel")


def c4_rig(small):
    W, H, D, NV = (320, 240, 64, 8) if small else (1280, 960, 128, 8)
    cams3 = synthetic.semicircle_rig(NV, W, H, radius=10.0, step_deg=22.5, focal=float(W))
    rgba, masks, _ = synthetic.render_sphere_views(cams3, W, H, 0x5EED0004, sphere_radius=2.0, tex_size=1024)
    cams = [capi.camera_from_krt(K, R, t) for (K, R, t) in cams3]
    p = capi.params_mvs(min_depth=8.0, max_depth=12.0, num_depth_levels=D, cross_check_threshold=2 * 4.0 / (D - 1))
    return "C4 %dx%d x%d" % (W, H, NV), rgba, masks, cams, p


def bunny_rig():
    g = np.load(os.path.join(ROOT, "tests", "golden", "bunny_views.npz"))
    NV = 8
    cams = [capi.camera_from_p(g["P"][v], g["dist"][v]) for v in range(NV)]
    p = capi.params_mvs(min_depth=30.0, max_depth=80.0, num_depth_levels=100, image_scale=0.25, cross_check_threshold=1.01)
    return "bunny %dx%d x%d" % (g["rgba"][0].shape[1], g["rgba"][0].shape[0], NV), list(g["rgba"][:NV]), list(g["mask"][:NV]), cams, p


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


def run(tag, rgba, masks, cams, p):
    nv = len(cams)
    slots = list(range(nv))
    print(tag)
    with capi.Context(0) as ctx:
        for v in slots:
            ctx.upload_view(v, rgba[v], masks[v], cams[v])
        neigh = capi.mvs_neighbours(cams, p)
        for v in slots:
            ctx.mvs_initial_estimate(v, neigh[v], p)
        est = [ctx.download_depth(v) for v in slots]

        def chain():
            for v in slots:
                ctx.mvs_cross_check(slots, v, p)
        chain()                                                   # warm: the kernel's code is on the device
        chain_runs = []
        for _ in range(REPEATS):
            for v in slots:
                ctx.upload_depth(v, est[v])                       # the chain works in place: the same maps every time
            _, chain_wall, prof = profiled(ctx, chain)
            chain_runs.append(prof["mvs_cross_check_kernel"][0])
        chain_ms, chain_n = min(chain_runs), prof["mvs_cross_check_kernel"][1]
        per_view = [ctx.point_cloud(v, p)["n_points"] for v in slots]
        ctx.mvs_fuse(slots, p)                                    # warm
        fuse_runs = []
        for _ in range(REPEATS):
            res, fuse_wall, prof = profiled(ctx, lambda: ctx.mvs_fuse(slots, p))
            fuse_runs.append(sum(prof[k][0] for k in FUSE_KERNELS))
        kern = {k: prof[k] for k in FUSE_KERNELS}                 # (the last run's split)
        fuse_ms = min(fuse_runs)
        print("  runs (ms, device events): chain %s; fusion %s" % (" ".join("%.3f" % t for t in chain_runs), " ".join("%.3f" % t for t in fuse_runs)))
        print("  cross-check chain : %8.3f ms in %d kernels (wall %.2f ms)" % (chain_ms, chain_n, chain_wall))
        print("  fusion            : %8.3f ms in kernels (wall %.2f ms with the download of %d points)" % (fuse_ms, fuse_wall, res["n_points"]))
        for k in FUSE_KERNELS:
            print("    %-20s %8.3f ms / %d" % (k, kern[k][0], kern[k][1]))
        print("  fusion / chain    : %.2f   (reference: nviews - 1 = %d)" % (fuse_ms / chain_ms, nv - 1))
        print("  points            : %d concatenated (%s) -> %d fused; claimed %d, unsupported %d, with surface normals %d"
              % (sum(per_view), " ".join(str(n) for n in per_view), res["n_points"], res["n_claimed"], res["n_unsupported"], res["n_normals"]))
        print("  views per point   : %s" % np.bincount(res["nviews"], minlength=nv + 1)[1:].tolist())


if __name__ == "__main__":
    small = len(sys.argv) > 1 and sys.argv[1] == "small"
    run(*c4_rig(small))
    run(*bunny_rig())
