"""The host class's semi-global aggregation switch (TwoViewStereo::setUseSGM, useSGM, sgmParams, sgmInfo):
tests/host_twoview_sgm_test.cpp compiled against the host library, and its device-free mode run -- the switch is off by
default, sgmParams() holds the defaults, setUseSGM(true) and setUseMRF(true) switch each other off, numSteps() stays 8.
tests/test_gpu_twoview_sgm.py runs the same program on the device against the C-ABI."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "stereoreconstruction_amd", "host")
LIBDIR = os.path.join(ROOT, "stereoreconstruction_amd")


def build(tmp_path):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "host_twoview_sgm_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + HOST,
                           os.path.join(ROOT, "tests", "host_twoview_sgm_test.cpp"),
                           os.path.join(HOST, "libstereo_recon_host.a"),
                           "-L" + LIBDIR, "-lstereo_recon_hip", "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


def test_host_class_sgm_switch_and_defaults(tmp_path):
    exe = build(tmp_path)
    out = subprocess.check_output([exe, "defaults"]).decode().split()
    assert out == ["1", "2", "0.25", "255"]


def test_header_names_the_stage_and_says_it_is_not_the_references():
    hdr = open(os.path.join(ROOT, "include", "stereo_recon_hip.h")).read()
    assert "#define SRH_ABI_VERSION 5" in hdr
    at = hdr.index("semi-global aggregation")
    section = hdr[at:hdr.index("srh_twoview_sgm_state(")]
    assert "NOT IN THE REFERENCE" in section
    for name in ("srh_twoview_sgm_params", "srh_twoview_sgm_params_defaults", "srh_sgm_info", "srh_twoview_sgm_aggregate",
                 "srh_twoview_sgm(", "srh_twoview_compute_sgm", "srh_twoview_sgm_dims", "srh_twoview_sgm_state", "path_mask"):
        assert name in hdr, name


def test_python_binding_exports_the_stage():
    from stereoreconstruction_amd import capi
    for name in ("srh_twoview_sgm_params_defaults", "srh_twoview_sgm_aggregate", "srh_twoview_sgm", "srh_twoview_compute_sgm",
                 "srh_twoview_sgm_dims", "srh_twoview_sgm_state"):
        assert name in capi.EXPORTS
    m = capi.twoview_sgm_params()
    assert (m.smooth_exp, m.smooth_max, m.lambda_, m.path_mask) == (1, 2.0, 0.25, 0xFF)
