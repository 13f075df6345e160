"""Times the speckle filter (srh_view_filter_speckles) with srh_profile_*, kernel by kernel, on three maps: the 1920x1080
random map of tests/speckle_ref.py, a 1920x1080 single plateau (one component: the worst case of the atomics) and the
bunny pair's two cross-checked maps.  Beside them the hole filling (srh_view_filter_invalid, flags 1 and 3) on the same
1920x1080 random map: code this stage does not touch, the yardstick.
usage: python3 profiles/speckle_timing.py      (from the repository root)"""
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import speckle_ref as R
from stereoreconstruction_amd import capi, synthetic

REPEATS = 5
KERNELS = ("speckle_tile_kernel", "speckle_merge_kernel", "speckle_flatten_kernel", "speckle_count_kernel", "speckle_apply_kernel")
FILTER_KERNELS = ("filter_gap_kernel", "filter_holes_kernel", "filter_median_kernel")


def cam(w, h):
    K = np.array([[w, 0, w / 2], [0, w, h / 2], [0, 0, 1]], np.float64)
    return capi.camera_from_krt(K, np.eye(3), np.zeros(3))


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


def timed(ctx, slot, depth, names, fn):
    """the best of REPEATS runs on the same map -> (sum of the kernels' device events, that run's split, wall, result)"""
    best = None
    for k in range(REPEATS + 1):                                # (the first run warms: the kernels' code reaches the device)
        ctx.upload_depth(slot, depth)
        out, wall, prof = profiled(ctx, fn)
        total = sum(prof[n][0] for n in names if n in prof)
        if k and (best is None or total < best[0]):
            best = (total, {n: prof[n] for n in names if n in prof}, wall, out)
    return best


def report(tag, best):
    total, split, wall, out = best
    print("  %-34s %8.3f ms in kernels (wall %.2f ms)  %s" % (tag, total, wall, out))
    for n, (ms, count) in split.items():
        print("      %-24s %8.3f ms / %d" % (n, ms, count))


def main():
    w, h = 1920, 1080
    p = capi.params_twoview(min_depth=30.0, max_depth=80.0, num_depth_levels=100)
    mask, depth = R.random_map(w, h, 0x5EC0 + w)
    rgba = np.empty((h, w, 4), np.uint8)
    rgba[..., :3] = synthetic.noise_image(7, w, h)
    rgba[..., 3] = 255
    with capi.Context(0) as ctx:
        print("speckle filter, %dx%d, min_size 50, max_diff %.2f (best of %d)" % (w, h, R.RANDOM_MAX_DIFF, REPEATS))
        ctx.upload_view(0, rgba, mask, cam(w, h))
        report("random map", timed(ctx, 0, depth, KERNELS, lambda: ctx.filter_speckles(0, p, 50, R.RANDOM_MAX_DIFF)))
        for flags in (1, 3):
            report("hole filling, flags %d (yardstick)" % flags,
                   timed(ctx, 0, depth, FILTER_KERNELS, lambda: ctx.filter_invalid(0, p, flags)))
        ctx.upload_view(0, rgba, None, cam(w, h))
        plateau = np.full((h, w), 40.0)
        report("single plateau", timed(ctx, 0, plateau, KERNELS, lambda: ctx.filter_speckles(0, p, 50, R.RANDOM_MAX_DIFF)))
        g = np.load(os.path.join(ROOT, "tests", "golden", "bunny_pair.npz"))
        bp = capi.params_twoview(min_depth=30.0, max_depth=80.0, num_depth_levels=100, image_scale=float(g["scale"][0]),
                                 window_radius=5, weight_kind=1)
        for slot, tag in enumerate(("left", "right")):
            ctx.upload_view(slot, g[tag + "_rgba"], g[tag + "_mask"],
                            capi.camera_from_krt(g[tag + "_K"], g[tag + "_R"], g[tag + "_t"], g[tag + "_dist"]))
        maps = ctx.twoview_compute(0, 1, bp)
        print("bunny pair, %dx%d, min_size 20, two depth steps" % (maps[0].shape[1], maps[0].shape[0]))
        for slot, tag in enumerate(("left", "right")):
            report("%s map" % tag, timed(ctx, slot, maps[slot], KERNELS, lambda: ctx.filter_speckles(slot, bp, 20)))


if __name__ == "__main__":
    main()
