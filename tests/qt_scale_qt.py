"""The installed Qt behind tests/qt_scale_driver.cpp, for tests/test_qt_scale_restatement.py and
tests/golden/make_qt_scale.py: builds the driver against the Qt that oracle/Makefile names (its `QT ?=` default, or the
QT environment variable) and wraps its three calls.  TEST INFRASTRUCTURE ONLY."""
import ctypes
import os
import re
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def qt_prefix():
    if os.environ.get("QT"):
        return os.environ["QT"]
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        m = re.search(r"^QT\s*\?=\s*(\S+)", f.read(), re.M)
    return m.group(1) if m else None


def available():
    q = qt_prefix()
    return bool(q) and os.path.exists(os.path.join(q, "lib", "libQt5Gui.so.5")) and \
        os.path.exists(os.path.join(q, "include", "qt", "QtGui", "QImage"))


class Qt:
    def __init__(self, outdir):
        q = qt_prefix()
        so = os.path.join(str(outdir), "libqt_scale_driver.so")
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-o", so,
                               os.path.join(HERE, "qt_scale_driver.cpp"),
                               "-I%s/include/qt" % q, "-I%s/include/qt/QtCore" % q, "-I%s/include/qt/QtGui" % q,
                               "%s/lib/libQt5Gui.so.5" % q, "%s/lib/libQt5Core.so.5" % q,
                               "-Wl,-rpath,%s/lib" % q, "-Wl,-rpath-link,%s/lib" % q])
        self.lib = ctypes.CDLL(so)
        self.lib.qs_qt_version.restype = ctypes.c_char_p
        self.version = self.lib.qs_qt_version().decode()

    def scaled_to_width(self, rgba, has_alpha, dw, smooth):
        """The raw bytes of scaledToWidth(dw, mode), (h, w, 4); None for a null image."""
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        h, w = rgba.shape[:2]
        cap = (max(dw, 1)*(h*max(dw, 1)//w + 2)) + 16
        out = np.zeros((cap, 4), np.uint8)
        dims = (ctypes.c_int*3)()
        rc = self.lib.qs_scaled_to_width(rgba.ctypes.data_as(ctypes.c_void_p), w, h, int(bool(has_alpha)), int(dw), int(bool(smooth)),
                                         out.ctypes.data_as(ctypes.c_void_p), ctypes.c_long(cap), dims)
        assert rc == 0 and dims[2] == 0, (rc, list(dims))
        if dims[0] == 0:
            return None
        return out[:dims[0]*dims[1]].reshape(dims[1], dims[0], 4).copy()

    def premultiply(self, rgba):
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        out = np.zeros_like(rgba)
        self.lib.qs_premultiply(rgba.ctypes.data_as(ctypes.c_void_p), rgba.shape[1], rgba.shape[0], out.ctypes.data_as(ctypes.c_void_p))
        return out


def random_image(rng, w, h, alpha):
    """Uniform bytes; with alpha, 255 on about 75 % of the pixels and uniform elsewhere (0 and 255 included)."""
    im = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if alpha:
        im[..., 3][rng.random((h, w)) < 0.75] = 255
    else:
        im[..., 3] = 255
    return im
