"""Makes tests/golden/qt_scale.npz: Qt's own outputs for the small scaling cases of tests/test_gpu_scale.py (the GPU
machine need not have Qt).  Needs the Qt that oracle/Makefile names and, for the crop, the reference's example images.

    python tests/golden/make_qt_scale.py

Per case NAME: NAME_scale, NAME_crc (zlib.crc32 of the source bytes; synthetic sources are regenerated from their seeds
by qt_scale_ref.synthetic_source, only the crop is stored, as bunny_src), and Qt's scaledToWidth((int)(w*scale), mode)
as NAME_smooth_alpha / NAME_smooth_opaque / NAME_fast_alpha / NAME_fast_opaque (opaque: the same bytes as a
Format_RGB32 image)."""
import os
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import qt_scale_qt          # noqa: E402
import qt_scale_ref as R    # noqa: E402

SYNTHETIC = {"rand64": (64, 48, 0.25, 101), "rand101": (101, 77, 0.5, 102), "rand37": (37, 29, 0.7, 103)}   # w, h, scale, seed
BUNNY = ("/root/reference/example/images/bunny/7310085.png", 384, 384, 256, 192, 0.25)          # file, x, y, w, h, scale


def main():
    from PIL import Image
    qt = qt_scale_qt.Qt(tempfile.mkdtemp())
    out = {"qt_version": np.array(qt.version)}
    cases = {k: (R.synthetic_source(w, h, seed), s) for k, (w, h, s, seed) in SYNTHETIC.items()}
    f, x, y, w, h, s = BUNNY
    crop = np.ascontiguousarray(np.asarray(Image.open(f).convert("RGBA"))[y:y + h, x:x + w])
    a = crop[..., 3]
    assert 0.2 < (a == 255).mean() < 0.8, "the crop should cross the silhouette"
    out["bunny_src"] = crop
    cases["bunny"] = (crop, s)
    for name, (src, scale) in cases.items():
        dw = int(src.shape[1]*scale)
        out[name + "_scale"] = np.array([scale])
        out[name + "_crc"] = np.array([zlib.crc32(src.tobytes())], dtype=np.uint32)
        for mode, smooth in (("smooth", True), ("fast", False)):
            for fmt, alpha in (("alpha", 1), ("opaque", 0)):
                out["%s_%s_%s" % (name, mode, fmt)] = qt.scaled_to_width(src, alpha, dw, smooth)
    path = os.path.join(HERE, "qt_scale.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, Qt", qt.version)


if __name__ == "__main__":
    main()
