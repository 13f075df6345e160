"""The census matching cost on the dense plan against the candidate lists at 1920x1080x256 (option "census_dense" 1 / 0;
DESIGN.md 4p): for the rectified geodesic pair (C3 inputs) or the refractive pair (C5: not row-aligned, the option must not
move it), `steps` timed srh_twoview_compute calls of each setting on one context -- NCC, SAD on the dense plan, census on the
lists, census on the dense plan -- ALTERNATING call by call after one warm-up call each, so that drift of the clocks falls
on all alike; prints one JSON line with the median wall-clock milliseconds per pair and, per setting, whether the last
pass took the dense plan.  Run under rocprofv3 --kernel-trace --stats (profiles/census_dense_trace.sh) for the per-kernel
numbers.

usage: python3 profiles/census_dense_pair.py STEPS c3|c5"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from stereoreconstruction_amd import capi, synthetic  # noqa: E402

SETTINGS = (("ncc", dict(cost=capi.COST_NCC)), ("sad_dense", dict(cost=capi.COST_SAD, sad_dense=1)),
            ("census_lists", dict(cost=capi.COST_CENSUS, census_dense=0)), ("census_dense", dict(cost=capi.COST_CENSUS, census_dense=1)))


def main(steps, geometry):
    W, H, D = 1920, 1080, 256
    seed, plane = {"c3": (0x5EED0003, (None, 0.0, 1.0)),
                   "c5": (0x5EED0050, (np.array([0.0, 0.0, 1.0]), 0.1, 1.333))}[geometry]
    ctx = capi.Context(0)
    ctx.set_option("tv_overlap", 0)          # the two passes one after the other: each kernel's own duration
    L, R, ml, mr, _ = synthetic.rectified_pair(W, H, D, seed)
    (Kl, Rl, tl), (Kr, Rr, tr) = synthetic.rectified_cameras(W, H)
    zmin, zmax = synthetic.rectified_depth_range(W, D)
    ctx.upload_view(0, L, ml, capi.camera_from_krt(Kl, Rl, tl, None, *plane))
    ctx.upload_view(1, R, mr, capi.camera_from_krt(Kr, Rr, tr, None, *plane))
    p = capi.params_twoview(min_depth=zmin, max_depth=zmax, num_depth_levels=D, weight_kind=capi.WEIGHT_GEODESIC)

    def call(opts):
        for k, v in opts.items():
            ctx.set_option(k, v)
        t0 = time.perf_counter()
        ctx.twoview_compute(0, 1, p)
        return (time.perf_counter() - t0) * 1e3

    t = {name: [] for name, _ in SETTINGS}
    dense = {}
    for name, opts in SETTINGS:              # warm-up: buffers, learnt list capacities, the signature and padded planes
        call(opts)
        dense[name] = int(ctx.stats()["used_dense_path"])
    for _ in range(steps):
        for name, opts in SETTINGS:
            t[name].append(call(opts))
    for k, v in dict(cost=capi.COST_NCC, sad_dense=0, census_dense=0).items():
        ctx.set_option(k, v)
    ctx.close()
    out = {"geometry": geometry, "steps": steps, "used_dense_path": dense}
    for name, _ in SETTINGS:
        out["%s_ms" % name] = round(float(np.median(t[name])), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20, sys.argv[2] if len(sys.argv) > 2 else "c3")
