"""Times of the scaling path on one MI355X: smooth_scale_kernel by device events (srh_profile_*) for
1024x768 -> 256x192 and 4000x3000 -> 1000x750, beside the time the bytes it has to move (the source once, the target
once) would take at the HBM rate; and the wall time of the whole upload_view_scaled call for eight such views.

    python profiles/scale_timing.py [--repeat 20]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stereoreconstruction_amd import capi                      # noqa: E402
from stereoreconstruction_amd import synthetic as S            # noqa: E402

HBM_BYTES_PER_S = 8.0e12                                        # MI355X: 8 TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    (K, R, t), _ = S.rectified_cameras(64, 48)
    cam = capi.camera_from_krt(K, R, t, None)
    with capi.Context(0) as ctx:
        for w, h in ((1024, 768), (4000, 3000)):
            src = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
            src[..., 3][rng.random((h, w)) < 0.75] = 255
            dw, dh = capi.scaled_size(w, h, 0.25)
            for _ in range(3):                                  # warm-up: code objects, pool blocks
                ctx.scale_image(src, 1, 0.25)
            ctx.profile_enable(True)
            ctx.profile_reset()
            for _ in range(a.repeat):
                ctx.scale_image(src, 1, 0.25)
            prof = ctx.profile()
            ctx.profile_enable(False)
            ms, n = prof["smooth_scale_kernel"]
            moved = 4.0*(w*h + dw*dh)
            floor_ms = moved/HBM_BYTES_PER_S*1e3
            print("smooth_scale_kernel %dx%d -> %dx%d: %.4f ms per launch (%d launches); %.1f MB moved = %.4f ms at 8 TB/s; "
                  "HBM floor / kernel time = %.3f" % (w, h, dw, dh, ms/n, n, moved/1e6, floor_ms, floor_ms/(ms/n)))
            pm, pn = prof["premultiply_kernel"]
            print("premultiply_kernel  %dx%d: %.4f ms per launch" % (w, h, pm/pn))
            for _ in range(2):
                for v in range(8):
                    ctx.upload_view_scaled(v, src, 1, 0.25, cam, capi.MASK_ALPHA_FAST)
            best, times = None, []
            for _ in range(max(3, a.repeat//4)):
                t0 = time.perf_counter()
                for v in range(8):
                    ctx.upload_view_scaled(v, src, 1, 0.25, cam, capi.MASK_ALPHA_FAST)
                times.append((time.perf_counter() - t0)*1e3)
            times.sort()
            print("upload_view_scaled, 8 views %dx%d at 0.25 (alpha mask): median %.2f ms, min %.2f, max %.2f (%d runs; %.1f MB "
                  "of source from host memory per run)" % (w, h, times[len(times)//2], times[0], times[-1],
                                                                                 len(times), 8*w*h*4/1e6))
            scaled = np.ascontiguousarray(ctx.download_view_image(0)[0])
            mask = ctx.download_view_image(0)[1]
            times = []
            for _ in range(max(3, a.repeat//4)):
                t0 = time.perf_counter()
                for v in range(8):
                    ctx.upload_view(v, scaled, mask, cam)
                times.append((time.perf_counter() - t0)*1e3)
            times.sort()
            print("upload_view of the same 8 views already scaled (%dx%d): median %.2f ms" % (dw, dh, times[len(times)//2]))


if __name__ == "__main__":
    main()
