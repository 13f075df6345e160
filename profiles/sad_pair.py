"""The SAD matching cost against NCC at 1920x1080x256: for the rectified geodesic pair (C3 inputs) and the
refractive pair (C5), `steps` timed srh_twoview_compute calls of each cost after a warm-up call, on one context; prints
one JSON line with the wall-clock milliseconds per pair.  Run under rocprofv3 --kernel-trace --stats (profiles/sad_trace.sh)
for the per-kernel numbers."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from stereoreconstruction_amd import capi, synthetic  # noqa: E402


def main(steps=3):
    W, H, D = 1920, 1080, 256
    ctx = capi.Context(0)
    ctx.set_option("tv_overlap", 0)          # the two passes one after the other: each kernel's own duration
    out = {}
    for geometry, seed, plane in (("c3", 0x5EED0003, (None, 0.0, 1.0)),
                                  ("c5", 0x5EED0050, (np.array([0.0, 0.0, 1.0]), 0.1, 1.333))):
        L, R, ml, mr, _ = synthetic.rectified_pair(W, H, D, seed)
        (Kl, Rl, tl), (Kr, Rr, tr) = synthetic.rectified_cameras(W, H)
        zmin, zmax = synthetic.rectified_depth_range(W, D)
        ctx.upload_view(0, L, ml, capi.camera_from_krt(Kl, Rl, tl, None, *plane))
        ctx.upload_view(1, R, mr, capi.camera_from_krt(Kr, Rr, tr, None, *plane))
        p = capi.params_twoview(min_depth=zmin, max_depth=zmax, num_depth_levels=D, weight_kind=capi.WEIGHT_GEODESIC)
        for cost in (capi.COST_NCC, capi.COST_SAD):
            ctx.set_option("cost", cost)
            ctx.twoview_compute(0, 1, p)
            t = []
            for _ in range(steps):
                t0 = time.perf_counter()
                ctx.twoview_compute(0, 1, p)
                t.append((time.perf_counter() - t0) * 1e3)
            out["%s_%s_ms" % (geometry, "sad" if cost else "ncc")] = round(float(np.median(t)), 2)
        ctx.set_option("cost", capi.COST_NCC)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 3)
