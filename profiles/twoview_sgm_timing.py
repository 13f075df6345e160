"""Times TwoViewStereo's semi-global aggregation (srh_twoview_sgm) with srh_profile_*: ms per direction, the read-off and
the whole stage on the synthetic rectified pair, after one warm-up run; beside it ONE TRW-S sweep (forward + backward +
read-off) of srh_twoview_mrf on the same input in the same session, which is what the stage is measured against.
    python profiles/twoview_sgm_timing.py [W H D] ...      default: 640 480 64 and 1920 1080 256
Bytes moved: the first direction reads C and writes S (2 volumes), each later one reads C and S and writes S (3), the
read-off reads S once: 24 volumes for 8 directions.  A sweep moves 15 volumes (forward and backward: D and two message
planes read, two written; read-off: D and two planes read)."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402,F401
import torch  # noqa: E402,F401  (attaches torch's ROCm runtime first, as the tests do)
from stereoreconstruction_amd import capi, synthetic  # noqa: E402

REPEATS = 10
DIRS = ["+1,0", "-1,0", "0,+1", "0,-1", "+1,+1", "-1,-1", "+1,-1", "-1,+1"]
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
    p = capi.params_twoview(min_depth=zmin, max_depth=zmax, num_depth_levels=D)
    vol = W * H * D * 8
    ctx.twoview_sgm(0, 1, p)                                             # warm-up: buffers, code objects
    ctx.profile_enable(True)
    ctx.profile_reset()
    t = time.time()
    for _ in range(REPEATS):
        info = ctx.twoview_sgm(0, 1, p)
    wall = (time.time() - t) * 1e3 / REPEATS
    prof = ctx.profile()
    ctx.profile_enable(False)
    per = [prof["twoview_sgm_path_kernel[%s]" % d][0] / prof["twoview_sgm_path_kernel[%s]" % d][1] for d in DIRS]
    read_ms = prof["twoview_sgm_readoff_kernel"][0] / prof["twoview_sgm_readoff_kernel"][1]
    stage = sum(per) + read_ms
    moved = 24 * vol
    print("%dx%dx%d SGM: %s ms per direction (%s), read-off %.3f ms, 8 paths + read-off %.3f ms, %.2f GB moved, %.2f TB/s; "
          "label costs %.2f ms, call %.1f ms, energy %.6g" % (
              W, H, D, " ".join("%.3f" % v for v in per), " ".join("[%s]" % d for d in DIRS), read_ms, stage, moved / 1e9,
              moved / stage / 1e9, prof["twoview_label_costs_kernel"][0] / REPEATS, wall, info["energy"]))
    # one TRW-S sweep on the same input, same session
    sweeps = 3
    ctx.twoview_mrf(0, 1, p, capi.twoview_mrf_params(min_energy_drop=-1.0, max_iters=0))
    ctx.profile_enable(True)
    ctx.profile_reset()
    minfo = ctx.twoview_mrf(0, 1, p, capi.twoview_mrf_params(min_energy_drop=-1.0, max_iters=sweeps - 1))
    prof = ctx.profile()
    ctx.profile_enable(False)
    sweep_ms = prof["twoview_mrf_pass_kernel"][0] / prof["twoview_mrf_pass_kernel"][1]
    print("%dx%dx%d TRW-S: sweep %.3f ms (%d sweeps), %.2f GB moved, %.2f TB/s, energy %.6g -> %.6g; 8 paths + read-off = %.2f sweeps "
          "(target: at most 2)" % (W, H, D, sweep_ms, minfo["iterations"], 15 * vol / 1e9, 15 * vol / sweep_ms / 1e9,
                                   minfo["energy_initial"], minfo["energy_final"], stage / sweep_ms))
