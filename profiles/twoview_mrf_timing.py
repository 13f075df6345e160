"""Times TwoViewStereo's MRF stage (srh_twoview_mrf) with srh_profile_*: ms per label-cost pass and ms per TRW-S sweep
(forward + backward + read-off) on the synthetic rectified pair, sweeps forced to a fixed count, after one warm-up run.
    python profiles/twoview_mrf_timing.py [W H D] ...      default: 640 480 64 and 1920 1080 256, both weight kinds
Beside the times: the step count of one pass, W + 15 + lag * (bands - 1) with lag = 12 columns and bands = ceil(H/16)."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (attaches torch's ROCm runtime first, as the tests do)
from stereoreconstruction_amd import capi, synthetic  # noqa: E402

SWEEPS = 4
args = [int(a) for a in sys.argv[1:]]
sizes = [tuple(args[i:i + 3]) for i in range(0, len(args), 3)] or [(640, 480, 64), (1920, 1080, 256)]
ctx = capi.Context(0)
print("build", capi.lib().srh_build_id().decode())
for (W, H, D) in sizes:
    L, R, ml, mr, _ = synthetic.rectified_pair(W, H, D, 0x5EED0003)
    (Kl, Rl, tl), (Kr, Rr, tr) = synthetic.rectified_cameras(W, H)
    zmin, zmax = synthetic.rectified_depth_range(W, D)
    ctx.upload_view(0, L, ml, capi.camera_from_krt(Kl, Rl, tl, None))
    ctx.upload_view(1, R, mr, capi.camera_from_krt(Kr, Rr, tr, None))
    bands = (H + 15) // 16
    steps = W + 15 + 12 * (bands - 1)
    for kind, kname in ((capi.WEIGHT_GEODESIC, "geodesic"), (capi.WEIGHT_ADAPTIVE, "adaptive")):
        p = capi.params_twoview(min_depth=zmin, max_depth=zmax, num_depth_levels=D, weight_kind=kind)
        m = capi.twoview_mrf_params(min_energy_drop=-1.0, max_iters=SWEEPS - 1)
        ctx.twoview_mrf(0, 1, p, capi.twoview_mrf_params(min_energy_drop=-1.0, max_iters=0))      # warm-up: buffers, code objects
        ctx.profile_enable(True)
        ctx.profile_reset()
        t = time.time()
        info = ctx.twoview_mrf(0, 1, p, m)
        wall = (time.time() - t) * 1e3
        prof = ctx.profile()
        ctx.profile_enable(False)
        cost_ms = prof["twoview_label_costs_kernel"][0]
        sweep_ms = prof["twoview_mrf_pass_kernel"][0] / prof["twoview_mrf_pass_kernel"][1]
        energy_ms = prof["twoview_mrf_energy_kernel"][0] / prof["twoview_mrf_energy_kernel"][1]
        print("%dx%dx%d %s r=%d: label costs %.2f ms, sweep %.3f ms (%d sweeps; %d bands, %d steps per pass: %.2f us per step), "
              "energy %.3f ms, call %.1f ms, energy %.6g -> %.6g" % (
                  W, H, D, kname, p.window_radius, cost_ms, sweep_ms, info["iterations"], bands, steps,
                  sweep_ms * 1e3 / (3 * steps), energy_ms, wall, info["energy_initial"], info["energy_final"]))
