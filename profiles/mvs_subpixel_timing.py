"""Times a MultiViewStereo run on bench.py's C4 inputs (8 views 1280x960x128 on a semicircle) with the sub-pixel stage
(srh_mvs_view_subpixel) off and on in one process, alternating, after warm-up runs at both settings.
    python profiles/mvs_subpixel_timing.py [--reps N] [--off-only] [--tree DIR] [--small]
One run is what MultiViewStereo::runTask queues: the eight estimates, with the stage on the stage of every view, the
cross-checks in view order, one wait.  Per setting: the median / min / max of the run (host clock, the run ends with a wait
for the device) and the spread max - min.  Then ONE more run per setting -- off, on, on with "mvs_subpixel_search" = 1 --
under srh_profile_* (device events around every launch, "mvs_async" 0 so that every kernel's own duration shows): the two
kernels of srh_mvs_subpixel.hip and the windows kernel the stage brings in, beside the kernels of the estimate.
--off-only: the stage is never called (a build without it: the parent commit).  --tree DIR: import the package from another
checkout (its stereoreconstruction_amd/ with its built library), so that parent and change are timed in one session:
    timeout -k 10 300 python profiles/mvs_subpixel_timing.py --off-only --tree ../parent && \
    timeout -k 10 300 python profiles/mvs_subpixel_timing.py
--small: 320x240x32 (a functional run)."""
import os
import statistics
import sys
import time

argv = sys.argv[1:]
reps, off_only, small = 3, False, False
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
if "--small" in argv:
    argv.remove("--small")
    small = True
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")            # as bench.py asks, before HIP initialises
sys.path.insert(0, os.path.abspath(tree))
import numpy as np  # noqa: E402,F401
import torch  # noqa: E402,F401  (attaches torch's ROCm runtime first, as the tests do)
from stereoreconstruction_amd import capi, synthetic  # noqa: E402

# bench.py's C4: WORKLOADS["c4"] and run_c4
VIEWS, W, H, D, SEED = 8, 1280, 960, 128, 0x5EED0004
if small:
    W, H, D = 320, 240, 32
SETTINGS = (0,) if off_only else (0, 1)
STAGE_KERNELS = ("mvs_subpixel_search_kernel", "mvs_subpixel_refine_kernel")

cams3 = synthetic.semicircle_rig(VIEWS, W, H, radius=10.0, step_deg=22.5, focal=float(W))
rgba, masks, _ = synthetic.render_sphere_views(cams3, W, H, SEED, sphere_radius=2.0, tex_size=1024)
cams = [capi.camera_from_krt(K, R, t) for (K, R, t) in cams3]
zmin, zmax = 8.0, 12.0
p = capi.params_mvs(min_depth=zmin, max_depth=zmax, num_depth_levels=D, weight_kind=capi.WEIGHT_GEODESIC,
                    cross_check_threshold=2 * (zmax - zmin) / (D - 1))
neigh = capi.mvs_neighbours(cams, p)
ctx = capi.Context(0)
print("build", capi.lib().srh_build_id().decode(), "of", os.path.abspath(tree))
for v in range(VIEWS):
    ctx.upload_view(v, rgba[v], masks[v], cams[v])


def run(on):
    """-> the stage's info per view (None with the stage off)"""
    for v in range(VIEWS):
        ctx.mvs_initial_estimate(v, neigh[v], p)
    infos = [ctx.mvs_view_subpixel(v, neigh[v], p) for v in range(VIEWS)] if on else None
    for v in range(VIEWS):
        ctx.mvs_cross_check(list(range(VIEWS)), v, p)
    ctx.synchronize()
    return infos


for _ in range(2):                                          # warm-up, every setting
    for on in SETTINGS:
        run(on)
ms = {on: [] for on in SETTINGS}
for _ in range(reps):
    for on in SETTINGS:
        t = time.perf_counter()
        infos = run(on)
        ms[on].append((time.perf_counter() - t) * 1e3)
        if on:
            last = infos
for on in SETTINGS:
    v = ms[on]
    print("C4 %dx%dx%d, %d views, stage %s: run median %.2f ms (min %.2f, max %.2f, spread %.2f, %d runs)" % (
        W, H, D, VIEWS, "on" if on else "off", statistics.median(v), min(v), max(v), max(v) - min(v), len(v)))
if not off_only:
    tot = np.sum([i["n_class"] for i in last], axis=0)
    print("the stage over the 8 views: classes (NONE, NO_NEIGHBOUR, FLAT, OUTSIDE, REFINED, NO_WINNER) %s, moved %d, fell back %d" % (
        tot.tolist(), sum(i["n_moved"] for i in last), sum(i["n_fallback"] for i in last)))

# kernel times: one view in flight, device events around every launch
ctx.set_option("mvs_async", 0)
for on, search in ((0, 0),) if off_only else ((0, 0), (1, 0), (1, 1)):
    if not off_only:
        ctx.set_option("mvs_subpixel_search", search)
    run(on)
    ctx.profile_enable(True)
    ctx.profile_reset()
    run(on)
    prof = ctx.profile()
    ctx.profile_enable(False)
    total = sum(v[0] for v in prof.values())
    stage = sum(prof[k][0] for k in STAGE_KERNELS if k in prof)
    line = "C4 stage %s%s, one view in flight: kernels %.2f ms per run" % ("on" if on else "off", ", exhaustive search" if search else "", total)
    if on:
        line += ", of which the stage's two kernels %.2f ms" % stage
    print(line)
    for k, (t_ms, n) in sorted(prof.items(), key=lambda kv: -kv[1][0]):
        print("    %-32s %9.3f ms per view (%d launches)" % (k, t_ms / VIEWS, n))
if not off_only:
    ctx.set_option("mvs_subpixel_search", 0)
ctx.set_option("mvs_async", 1)
