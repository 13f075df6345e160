"""CPU checks of the census dense plan's plumbing: the host class's setCensusDense compiles and links without a device, and
the strip kernel's source is part of the library's build."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "stereoreconstruction_amd", "host")
LIBDIR = os.path.join(ROOT, "stereoreconstruction_amd")


def test_host_set_census_dense_compiles_without_gpu(tmp_path):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "host_census_dense_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + HOST,
                           os.path.join(ROOT, "tests", "host_census_dense_test.cpp"),
                           os.path.join(HOST, "libstereo_recon_host.a"),
                           "-L" + LIBDIR, "-lstereo_recon_hip", "-Wl,-rpath," + LIBDIR, "-o", exe])
    assert os.path.exists(exe)


def test_strip_census_kernel_is_built_into_the_library():
    with open(os.path.join(LIBDIR, "csrc", "Makefile")) as f:
        srcs = [ln for ln in f if ln.startswith("SRCS")][0]
    assert "srh_census_strip.hip" in srcs.split()
    with open(os.path.join(LIBDIR, "libstereo_recon_hip.so"), "rb") as f:
        assert b"twoview_strip_census_kernel" in f.read()
