"""Times MultiViewStereo's semi-global aggregation over the peak labels (srh_mvs_sgm_estimate) with
srh_profile_*: ms per direction, the read-off (labels + depth map), the data costs and the energy, on a synthetic top-9 peaks
buffer (mrf_cases.peaks_case_fast), after one warm-up run, the mean of REPEATS runs; beside it, in the same process and on
the same peaks, ONE TRW-S sweep of the MRF branch (srh_mvs_mrf_estimate with max_iters = 0: forward + backward + read-off
passes, and the two energy passes it cannot do without), which is what the stage is measured against.
Then N views side by side (srh_mvs_sgm_estimate_views against srh_mvs_mrf_estimate_views with max_iters = 0), wall time per
call: the _views forms take the peaks a real initial estimate kept, so these come from the synthetic sphere rig at the same
size (the kernels' time does not depend on the peaks' values: there is no data-dependent branch in them).
    python profiles/mvs_sgm_timing.py [W H [N]]            default: 1280 960 8
Under rocprofv3 --kernel-trace --stats the same script gives the per-kernel view."""
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")      # as profiles/mrf_views.py: one stream per view in the _views forms
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (attaches torch's ROCm runtime first, as the tests do)
import cases  # noqa: E402
import mrf_cases  # noqa: E402
import oracle_ffi as O  # noqa: E402
from stereoreconstruction_amd import capi  # noqa: E402

REPEATS = 10
DIRS = ["+1,0", "-1,0", "0,+1", "0,-1", "+1,+1", "-1,-1", "+1,-1", "-1,+1"]
args = [int(a) for a in sys.argv[1:]]
W, H = (args[0], args[1]) if len(args) >= 2 else (1280, 960)
N = args[2] if len(args) >= 3 else 8
K = 9
ctx = capi.Context(0)
print("build", capi.lib().srh_build_id().decode(), "GPU_MAX_HW_QUEUES", os.environ.get("GPU_MAX_HW_QUEUES"))

# ---- one view, synthetic peaks
peaks, mask = mrf_cases.peaks_case_fast(W, H, K=K, seed=5)
rgba = np.zeros((H, W, 4), dtype=np.uint8)
rgba[..., 3] = 255
Km = np.array([[100.0, 0, W / 2], [0, 100.0, H / 2], [0, 0, 1]])
ctx.upload_view(0, rgba, mask, capi.camera_from_krt(Km, np.eye(3), np.zeros(3), None))
pk = torch.from_numpy(peaks).to("cuda:0")
torch.cuda.synchronize()
ctx.mvs_sgm_estimate(0, K, pk.data_ptr())                                # warm-up: buffers, code objects
ctx.profile_enable(True)
ctx.profile_reset()
t = time.time()
for _ in range(REPEATS):
    info = ctx.mvs_sgm_estimate(0, K, pk.data_ptr())
wall = (time.time() - t) * 1e3 / REPEATS
prof = ctx.profile()
ctx.profile_enable(False)


def mean(name):
    return prof[name][0] / prof[name][1]


per = [mean("mvs_sgm_path_kernel[%s]" % d) for d in DIRS]
read_ms, data_ms, energy_ms = mean("mvs_sgm_readoff_kernel"), mean("mrf_data_kernel"), mean("mrf_energy_kernel")
stage = sum(per) + read_ms
print("%dx%d K=%d SGM: %s ms per direction (%s), read-off %.3f ms, 8 paths + read-off %.3f ms; data costs %.3f ms, energy %.3f ms, "
      "call %.2f ms, energy %.6f" % (W, H, K, " ".join("%.3f" % v for v in per), " ".join("[%s]" % d for d in DIRS), read_ms, stage,
                                     data_ms, energy_ms, wall, info["energy"]))
one = capi.mrf_params(min_energy_drop=-1.0, max_iters=0)
ctx.mvs_mrf_estimate(0, K, pk.data_ptr(), one)
ctx.profile_enable(True)
ctx.profile_reset()
t = time.time()
for _ in range(REPEATS):
    minfo = ctx.mvs_mrf_estimate(0, K, pk.data_ptr(), one)
mwall = (time.time() - t) * 1e3 / REPEATS
prof = ctx.profile()
ctx.profile_enable(False)
sweep_ms, menergy_ms = mean("mrf_pass_kernel"), mean("mrf_energy_kernel")
print("%dx%d K=%d TRW-S: one sweep %.3f ms, an energy pass %.3f ms, sweep + 2 energy passes %.3f ms, call %.2f ms, energy %.6f -> %.6f; "
      "8 paths + read-off = %.2f of that" % (W, H, K, sweep_ms, menergy_ms, sweep_ms + 2 * menergy_ms, mwall, minfo["energy_initial"],
                                             minfo["energy_final"], stage / (sweep_ms + 2 * menergy_ms)))
full = ctx.mvs_mrf_estimate(0, K, pk.data_ptr())
print("%dx%d K=%d TRW-S by the reference's stopping rule: %d sweeps, energy %.6f" % (W, H, K, full["iterations"], full["energy_final"]))

# ---- N views side by side, peaks of a real initial estimate
case = cases.get_mvs("mvs_geodesic", w=W, h=H, D=64, nviews=N)
imgs, ocams, op = cases.oracle_inputs(case)
neigh = O.mvs_neighbours(ocams, op)
cams, p = cases.hip_inputs(case)
cases.upload_case(ctx, case, cams)
for v in range(N):
    ctx.mvs_initial_estimate_peaks(v, neigh[v], p)
ctx.synchronize()
views = list(range(N))
for name, call in (("SGM, 8 directions", lambda: ctx.mvs_sgm_estimate_views(views)),
                   ("SGM, one view of them", lambda: ctx.mvs_sgm_estimate_views([0])),
                   ("TRW-S, one sweep each", lambda: ctx.mvs_mrf_estimate_views(views, one)),
                   ("TRW-S, one view of them", lambda: ctx.mvs_mrf_estimate_views([0], one))):
    call()
    times = []
    for _ in range(REPEATS):
        t = time.time()
        infos = call()
        times.append((time.time() - t) * 1e3)
    print("%d views %dx%d K=%d side by side: %s: %.2f ms per call (min %.2f, max %.2f)" % (
        len(infos), W, H, p.top_k, name, sum(times) / len(times), min(times), max(times)))
