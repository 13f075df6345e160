"""Host time of Qt's own scalings (QImage::scaledToWidth smooth + fast, what the Qt binding's ingestViewFile does per
view), beside profiles/scale_timing.py.  Needs the Qt that oracle/Makefile names; one CPU thread.

    python profiles/qt_scale_timing.py
"""
import ctypes
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import qt_scale_qt                                              # noqa: E402


def main():
    qt = qt_scale_qt.Qt(tempfile.mkdtemp())
    qt.lib.qs_time_ingest_ms.restype = ctypes.c_double
    rng = np.random.default_rng(1)
    for w, h, rep in ((1024, 768, 40), (4000, 3000, 6)):
        src = qt_scale_qt.random_image(rng, w, h, 1)
        qt.lib.qs_time_ingest_ms(src.ctypes.data_as(ctypes.c_void_p), w, h, w//4, 2)
        ms = [qt.lib.qs_time_ingest_ms(src.ctypes.data_as(ctypes.c_void_p), w, h, w//4, rep) for _ in range(3)]
        print("Qt %s scaledToWidth smooth + fast, %dx%d at 0.25: %.2f ms per view (3 runs: %s); 8 views: %.1f ms"
              % (qt.version, w, h, min(ms), ", ".join("%.2f" % m for m in ms), 8*min(ms)))


if __name__ == "__main__":
    main()
