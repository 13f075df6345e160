"""Times srh_twoview_compute with option "subpixel" at 0 and 1 in one process, alternating, on the synthetic rectified
pair, after warm-up runs at both settings (buffers, planes, code objects).
    python profiles/subpixel_timing.py [--reps N] [--off-only] [--tree DIR] [W H D kind] ...
default: 1920 1080 256 geodesic, 3 repetitions per setting.  kind: geodesic, adaptive, or either with "-refractive".
Per setting: the median / min / max of the call (host clock around the synchronous call, which ends with a wait for the
device) and the spread max - min, then ONE more call per setting under srh_profile_* (device events around every launch;
the passes one after the other, "tv_overlap" 0, so that every kernel's own duration shows): the two kernels of
srh_subpixel.hip beside twoview_winner_costs_kernel, which the option also brings in, per pass.
--off-only: the option is never set (a build without it: the parent commit).  --tree DIR: import the package from another
checkout (its stereoreconstruction_amd/ with its built library), so that parent and change are timed in one session:
    timeout -k 10 300 python profiles/subpixel_timing.py --off-only --tree ../parent && \
    timeout -k 10 300 python profiles/subpixel_timing.py"""
import os
import statistics
import sys
import time

argv = sys.argv[1:]
reps, off_only = 3, False
tree = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
if "--reps" in argv:
    i = argv.index("--reps")
    reps = int(argv[i + 1])
    del argv[i:i + 2]
if "--tree" in argv:
    i = argv.index("--tree")
    tree = argv[i + 1]
    del argv[i:i + 2]
if "--off-only" in argv:
    argv.remove("--off-only")
    off_only = True
sys.path.insert(0, os.path.abspath(tree))
import numpy as np  # noqa: E402,F401
import torch  # noqa: E402,F401  (attaches torch's ROCm runtime first, as the tests do)
from stereoreconstruction_amd import capi, synthetic  # noqa: E402

sizes = [(int(argv[i]), int(argv[i + 1]), int(argv[i + 2]), argv[i + 3]) for i in range(0, len(argv), 4)] or \
    [(1920, 1080, 256, "geodesic")]
SETTINGS = (0,) if off_only else (0, 1)
KERNELS = ("twoview_winner_costs_kernel", "label_plane_table_kernel", "subpixel_neighbours_kernel", "subpixel_refine_kernel")


def set_subpixel(ctx, on):
    if not off_only:
        ctx.set_option("subpixel", on)


ctx = capi.Context(0)
print("build", capi.lib().srh_build_id().decode(), "of", os.path.abspath(tree))
for (W, H, D, kname) in sizes:
    kind = capi.WEIGHT_GEODESIC if kname.startswith("geodesic") else capi.WEIGHT_ADAPTIVE
    # "<weights>-refractive": the same pair behind a planar refractive interface (bench.py's C5 geometry: curved epipolar
    # lines, the candidate lists instead of the dense plan)
    plane = (np.array([0.0, 0.0, 1.0]), 0.1, 1.333) if kname.endswith("-refractive") else ()
    L, R, ml, mr, _ = synthetic.rectified_pair(W, H, D, 0x5EED0003)
    (Kl, Rl, tl), (Kr, Rr, tr) = synthetic.rectified_cameras(W, H)
    zmin, zmax = synthetic.rectified_depth_range(W, D)
    ctx.upload_view(0, L, ml, capi.camera_from_krt(Kl, Rl, tl, None, *plane))
    ctx.upload_view(1, R, mr, capi.camera_from_krt(Kr, Rr, tr, None, *plane))
    p = capi.params_twoview(min_depth=zmin, max_depth=zmax, num_depth_levels=D, weight_kind=kind)
    for _ in range(2):                                      # warm-up, every setting
        for on in SETTINGS:
            set_subpixel(ctx, on)
            ctx.twoview_compute(0, 1, p)
    ms = {on: [] for on in SETTINGS}
    for _ in range(reps):
        for on in SETTINGS:
            set_subpixel(ctx, on)
            t = time.perf_counter()
            ctx.twoview_compute(0, 1, p)
            ms[on].append((time.perf_counter() - t) * 1e3)
    st = ctx.stats()
    for on in SETTINGS:
        v = ms[on]
        print("%dx%dx%d %s subpixel=%d: call median %.2f ms (min %.2f, max %.2f, spread %.2f, %d calls; dense %d strip %d)" % (
            W, H, D, kname, on, statistics.median(v), min(v), max(v), max(v) - min(v), len(v), st["used_dense_path"], st["used_strip_kernel"]))
    # kernel times: the passes one after the other, device events around every launch
    ctx.set_option("tv_overlap", 0)
    for on in SETTINGS:
        set_subpixel(ctx, on)
        ctx.twoview_compute(0, 1, p)
        ctx.profile_enable(True)
        ctx.profile_reset()
        ctx.twoview_compute(0, 1, p)
        prof = ctx.profile()
        ctx.profile_enable(False)
        total = sum(v[0] for v in prof.values())
        line = "%dx%dx%d %s subpixel=%d, passes in turn: kernels %.2f ms" % (W, H, D, kname, on, total)
        for k in KERNELS:
            if k in prof:
                t_ms, n = prof[k]
                line += "; %s %.3f ms per pass (%d launches)" % (k, t_ms / 2, n)
        print(line)
    ctx.set_option("tv_overlap", 1)
    set_subpixel(ctx, 0)
