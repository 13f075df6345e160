"""The SAD matching cost of the rectified pair (C3 inputs, 1920x1080x256, geodesic r = 5) on the dense plan against the
row-run lists (option "sad_dense" 1 / 0): one context, a warm-up call of both settings, then the two
settings alternating, `steps` timed srh_twoview_compute calls each.  Prints one JSON line: median, min and max of the
wall-clock milliseconds per pair and setting.  usage: python3 profiles/sad_dense_pair.py [steps] [tv_overlap] [ncc]
(tv_overlap 0: the two passes one after the other, each kernel's own duration under rocprofv3 --kernel-trace --stats,
profiles/sad_dense_trace.sh; ncc 1: a few NCC pairs behind the SAD ones, for the NCC strip kernel in the same trace)."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from stereoreconstruction_amd import capi, synthetic  # noqa: E402


def main(steps=20, overlap=1, ncc=0):
    W, H, D = 1920, 1080, 256
    ctx = capi.Context(0)
    ctx.set_option("tv_overlap", overlap)
    L, R, ml, mr, _ = synthetic.rectified_pair(W, H, D, 0x5EED0003)
    (Kl, Rl, tl), (Kr, Rr, tr) = synthetic.rectified_cameras(W, H)
    zmin, zmax = synthetic.rectified_depth_range(W, D)
    ctx.upload_view(0, L, ml, capi.camera_from_krt(Kl, Rl, tl, None, None, 0.0, 1.0))
    ctx.upload_view(1, R, mr, capi.camera_from_krt(Kr, Rr, tr, None, None, 0.0, 1.0))
    p = capi.params_twoview(min_depth=zmin, max_depth=zmax, num_depth_levels=D, weight_kind=capi.WEIGHT_GEODESIC)
    ctx.set_option("cost", capi.COST_SAD)
    maps = {}
    for dense in (0, 1):                      # warm-up of both settings (buffers, learnt list capacities, cached planes)
        ctx.set_option("sad_dense", dense)
        for _ in range(2):
            maps[dense] = ctx.twoview_compute(0, 1, p)
        st = ctx.stats()
        assert bool(st["used_dense_path"]) == bool(dense) and bool(st["used_strip_kernel"]) == bool(dense), st
    same = all(np.array_equal(maps[0][k].view(np.uint64), maps[1][k].view(np.uint64)) for k in range(2))
    t = {0: [], 1: []}
    for _ in range(steps):
        for dense in (0, 1):
            ctx.set_option("sad_dense", dense)
            t0 = time.perf_counter()
            ctx.twoview_compute(0, 1, p)
            t[dense].append((time.perf_counter() - t0) * 1e3)
    out = dict(steps=steps, tv_overlap=overlap, same_bits=bool(same))
    for dense, tag in ((0, "rows"), (1, "dense")):
        out["sad_%s_ms" % tag] = dict(median=round(float(np.median(t[dense])), 3), min=round(min(t[dense]), 3),
                                      max=round(max(t[dense]), 3))
    ctx.set_option("sad_dense", 0)
    ctx.set_option("cost", capi.COST_NCC)
    if ncc:
        ctx.twoview_compute(0, 1, p)
        tn = []
        for _ in range(max(3, steps // 4)):
            t0 = time.perf_counter()
            ctx.twoview_compute(0, 1, p)
            tn.append((time.perf_counter() - t0) * 1e3)
        out["ncc_ms"] = dict(median=round(float(np.median(tn)), 3), min=round(min(tn), 3), max=round(max(tn), 3))
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:]]
    main(*a)
