"""The scaling interface above the C-ABI.  Without a device: the four entry points are exported, declared and bound,
and a program that uses the host classes' file-resolution forms compiles and links.  On the device
(tests/host_scale_test.cpp): MultiViewStereo::initialize with an ImageDecoder over the fixture's bunny crop gives the
images, masks and depth maps of the ImageLoader form fed the restatement's output, and TwoViewStereo's ScaleOnDevice
constructor those of the constructor that takes scaled images -- bit for bit."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import qt_scale_ref as R
from stereoreconstruction_amd import capi
from stereoreconstruction_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "stereoreconstruction_amd", "host")
LIBDIR = os.path.join(ROOT, "stereoreconstruction_amd")
NAMES = ("srh_scaled_size", "srh_image_scale", "srh_view_upload_scaled", "srh_view_image_download")


def build_host_program(out_dir):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    exe = os.path.join(str(out_dir), "host_scale_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + HOST,
                           os.path.join(ROOT, "tests", "host_scale_test.cpp"),
                           os.path.join(HOST, "libstereo_recon_host.a"),
                           "-L" + LIBDIR, "-lstereo_recon_hip", "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


def test_entry_points_are_exported_bound_and_declared():
    L = capi.lib()
    hdr = open(os.path.join(ROOT, "include", "stereo_recon_hip.h")).read()
    for name in NAMES:
        assert name in capi.EXPORTS, name
        assert hasattr(L, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    assert "SRH_SCALE_SMOOTH = 0, SRH_SCALE_FAST = 1" in hdr
    assert "SRH_MASK_NONE = 0, SRH_MASK_ALPHA_FAST = 1, SRH_MASK_IMAGE_SMOOTH = 2" in hdr
    assert (capi.SCALE_SMOOTH, capi.SCALE_FAST) == (R.SMOOTH, R.FAST) == (0, 1)
    assert (capi.MASK_NONE, capi.MASK_ALPHA_FAST, capi.MASK_IMAGE_SMOOTH) == (R.MASK_NONE, R.MASK_ALPHA_FAST, R.MASK_IMAGE_SMOOTH)
    for m in ("upload_view_scaled", "scale_image", "download_view_image"):
        assert callable(getattr(capi.Context, m))


def test_scaled_size_needs_no_device():
    for args in ((64, 48, 0.25), (101, 77, 0.5), (37, 29, 0.7), (1024, 768, 0.25), (1175, 881, 0.3), (333, 251, 0.41), (40, 30, 1.0)):
        for mode in (R.SMOOTH, R.FAST):
            assert capi.scaled_size(*args, mode=mode) == R.scaled_size(*args, mode=mode), (args, mode)
    assert capi.scaled_size(101, 77, 0.5, capi.SCALE_SMOOTH) == (50, 39) and capi.scaled_size(101, 77, 0.5, capi.SCALE_FAST) == (50, 38)
    for args in ((64, 48, 0.0), (64, 48, 0.01), (64, 48, -1.0), (64, 48, 1.5), (64, 1, 0.7), (0, 4, 0.5), (64, 3, 0.125)):
        for mode in (R.SMOOTH, R.FAST):
            try:
                want = R.scaled_size(*args, mode=mode)
            except R.Refused as e:
                want = e.code
            try:
                got = capi.scaled_size(*args, mode=mode)
            except capi.StereoHipError as e:
                got = e.code
            assert got == want, (args, mode)
    with pytest.raises(capi.StereoHipError) as e:
        capi.scaled_size(64, 48, 0.5, 2)
    assert e.value.code == capi.SRH_E_INVALID


def test_host_program_using_the_new_forms_compiles_without_gpu(tmp_path):
    exe = build_host_program(tmp_path)
    assert os.path.exists(exe)
    src = open(os.path.join(ROOT, "tests", "host_scale_test.cpp")).read()
    for member in ("MultiViewStereo::ImageDecoder", "TwoViewStereo::ScaleOnDevice()", "hasAlpha", "leftMaskBytes("):
        assert member in src, member
    assert "bool hasAlpha" in open(os.path.join(HOST, "image.hpp")).read()


@pytest.mark.gpu
def test_host_classes_scale_on_the_device(tmp_path):
    g = np.load(os.path.join(ROOT, "tests", "golden", "qt_scale.npz"))
    left = g["bunny_src"]
    views = [left, np.ascontiguousarray(np.roll(left, -24, axis=1))]
    scale, D = 0.25, 16
    sh, sw = left.shape[:2]
    w, h = R.scaled_size(sw, sh, scale, R.SMOOTH)
    mw, mh = R.scaled_size(sw, sh, scale, R.FAST)
    cams = S.rectified_cameras(w, h)
    zmin, zmax = S.rectified_depth_range(w, D)
    yy, xx = np.mgrid[0:sh, 0:sw]
    inside = ((xx - sw*0.45)**2/(sw*0.4)**2 + (yy - sh*0.5)**2/(sh*0.42)**2) < 1
    msrc = np.where(inside[..., None], np.uint8(255), np.uint8(0)).repeat(4, axis=-1)
    msrc[..., 3] = 255
    msrc = np.ascontiguousarray(msrc)
    path = os.path.join(str(tmp_path), "in.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<9i", 2, sw, sh, 1, w, h, mw, mh, D))
        f.write(struct.pack("<4d", scale, zmin, zmax, 2.0*(zmax - zmin)/(D - 1)))
        for v, im in enumerate(views):
            K, Rm, t = cams[v]
            K = K.copy()
            K[:2] /= scale
            for a in (K, Rm, t):
                f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
            f.write(im.tobytes())
            f.write(R.scale_image(im, 1, scale, R.SMOOTH).tobytes())
            f.write(R.scale_image(im, 1, scale, R.FAST).tobytes())
            f.write(msrc.tobytes())
            f.write(R.scale_image(msrc, 0, scale, R.SMOOTH).tobytes())
    exe = build_host_program(tmp_path)
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK"), r.stdout
    white = int(r.stdout.split()[4])
    assert 0 < white < w*h                                                  # the mask image did mask
