"""Times srh_twoview_compute with option "wta_outputs" at 0, 1 and 3 in one process, alternating, on the synthetic
rectified pair, after warm-up runs at every setting (buffers, planes, code objects).
    python profiles/wta_outputs_timing.py [--reps N] [--once] [W H D kind] ...
default: 1920 1080 256 geodesic and 640 480 64 adaptive, 7 repetitions per setting.
Per setting: the median / min / max of the call (host clock around the synchronous call, which ends with a wait for the
device), then ONE more call per setting under srh_profile_* (device events around every launch; the passes one after the
other, "tv_overlap" 0, so that every kernel's own duration shows): twoview_winner_costs_kernel's time and its bytes per
second -- the band's window buffer read once plus the four planes written -- beside the windows kernel's, which writes
that same buffer.  --once: one call per setting and nothing else (the command a kernel trace is taken of)."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402,F401
import torch  # noqa: E402,F401  (attaches torch's ROCm runtime first, as the tests do)
from stereoreconstruction_amd import capi, synthetic  # noqa: E402

argv = sys.argv[1:]
reps, once = 7, False
if "--reps" in argv:
    i = argv.index("--reps")
    reps = int(argv[i + 1])
    del argv[i:i + 2]
if "--once" in argv:
    argv.remove("--once")
    once = True
sizes = [(int(argv[i]), int(argv[i + 1]), int(argv[i + 2]), argv[i + 3]) for i in range(0, len(argv), 4)] or \
    [(1920, 1080, 256, "geodesic"), (640, 480, 64, "adaptive")]
WINDOW_KERNELS = ("geodesic_dma_kernel", "geodesic_reg_kernel", "adaptive_reg_kernel", "weights_kernel")
SETTINGS = (0, 1, 3)

ctx = capi.Context(0)
print("build", capi.lib().srh_build_id().decode())
for (W, H, D, kname) in sizes:
    kind = capi.WEIGHT_GEODESIC if kname == "geodesic" else capi.WEIGHT_ADAPTIVE
    L, R, ml, mr, _ = synthetic.rectified_pair(W, H, D, 0x5EED0003)
    (Kl, Rl, tl), (Kr, Rr, tr) = synthetic.rectified_cameras(W, H)
    zmin, zmax = synthetic.rectified_depth_range(W, D)
    ctx.upload_view(0, L, ml, capi.camera_from_krt(Kl, Rl, tl, None))
    ctx.upload_view(1, R, mr, capi.camera_from_krt(Kr, Rr, tr, None))
    p = capi.params_twoview(min_depth=zmin, max_depth=zmax, num_depth_levels=D, weight_kind=kind)
    if once:
        for flags in SETTINGS:
            ctx.set_option("wta_outputs", flags)
            ctx.twoview_compute(0, 1, p)
        continue
    for _ in range(2):                                      # warm-up, every setting
        for flags in SETTINGS:
            ctx.set_option("wta_outputs", flags)
            ctx.twoview_compute(0, 1, p)
    ms = {f: [] for f in SETTINGS}
    for _ in range(reps):
        for flags in SETTINGS:
            ctx.set_option("wta_outputs", flags)
            t = time.perf_counter()
            ctx.twoview_compute(0, 1, p)
            ms[flags].append((time.perf_counter() - t) * 1e3)
    st = ctx.stats()
    for flags in SETTINGS:
        v = ms[flags]
        print("%dx%dx%d %s wta_outputs=%d: call median %.2f ms (min %.2f, max %.2f, %d calls; dense %d strip %d)" % (
            W, H, D, kname, flags, statistics.median(v), min(v), max(v), len(v), st["used_dense_path"], st["used_strip_kernel"]))
    # kernel times: the passes one after the other, device events around every launch
    ctx.set_option("tv_overlap", 0)
    for flags in SETTINGS:
        ctx.set_option("wta_outputs", flags)
        ctx.twoview_compute(0, 1, p)
        ctx.profile_enable(True)
        ctx.profile_reset()
        ctx.twoview_compute(0, 1, p)
        prof = ctx.profile()
        ctx.profile_enable(False)
        total = sum(v[0] for v in prof.values())
        line = "%dx%dx%d %s wta_outputs=%d, passes in turn: kernels %.2f ms" % (W, H, D, kname, flags, total)
        R_ = p.window_radius
        wp = (2 * R_ + 2) & ~1
        tiles = (W + 31) // 32 * 32 * H
        wbytes = tiles * (2 * R_ + 1) * (wp if st["used_strip_kernel"] else 2 * R_ + 1) * 8
        for k in WINDOW_KERNELS:
            if k in prof:
                t_ms, n = prof[k]
                line += "; %s %.3f ms per pass (writes %.2f GB: %.0f GB/s)" % (k, t_ms / n, wbytes / 1e9, wbytes / 1e6 / (t_ms / n))
        if "twoview_winner_costs_kernel" in prof:
            t_ms, n = prof["twoview_winner_costs_kernel"]
            moved = wbytes + W * H * 32
            line += "; twoview_winner_costs_kernel %.3f ms per pass (window buffer + planes %.2f GB: %.0f GB/s)" % (
                t_ms / n, moved / 1e9, moved / 1e6 / (t_ms / n))
        print(line)
    ctx.set_option("tv_overlap", 1)
    ctx.set_option("wta_outputs", 0)
