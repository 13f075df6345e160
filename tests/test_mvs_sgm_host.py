"""MultiViewStereo's semi-global aggregation above the kernels, without a device: the header's section, the Python binding's
names and defaults, and the host class's switch (MultiViewStereo::setUseSGM, useSGM, sgmParams, sgmInfo) --
tests/host_mvs_sgm_test.cpp compiled against the host library and its device-free mode run: both switches are off by
default, sgmParams() holds the defaults, setUseSGM(true) and setUseMRF(true) switch each other off, numSteps() stays 2*views.
tests/test_gpu_mvs_sgm.py runs the same program on the device against the C-ABI."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "stereoreconstruction_amd", "host")
LIBDIR = os.path.join(ROOT, "stereoreconstruction_amd")

NAMES = ("srh_mvs_sgm_params_defaults", "srh_mvs_sgm_estimate", "srh_mvs_initial_estimate_sgm", "srh_mvs_sgm_estimate_views",
         "srh_mvs_sgm_dims", "srh_mvs_sgm_state")


def build(tmp_path):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "host_mvs_sgm_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + HOST,
                           os.path.join(ROOT, "tests", "host_mvs_sgm_test.cpp"),
                           os.path.join(HOST, "libstereo_recon_host.a"),
                           "-L" + LIBDIR, "-lstereo_recon_hip", "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


def test_host_class_sgm_switch_and_defaults(tmp_path):
    exe = build(tmp_path)
    out = subprocess.check_output([exe, "defaults"]).decode().split()
    assert out == ["1", "1", "0.5", "0.002", "255"]


def test_header_names_the_stage_and_says_it_is_not_the_references():
    hdr = open(os.path.join(ROOT, "include", "stereo_recon_hip.h")).read()
    assert "#define SRH_ABI_VERSION 5" in hdr
    at = hdr.index("MultiViewStereo, semi-global aggregation")
    section = hdr[at:hdr.index("srh_mvs_sgm_state(")]
    assert "NOT IN THE REFERENCE" in section
    for name in NAMES + ("srh_mvs_sgm_params", "srh_sgm_info", "path_mask", "phi_u", "psi_u"):
        assert name in section + "srh_mvs_sgm_state(", name
    # the definition is there in full
    for words in ("labels", "D(p, l)", "V(q, k; p, d)", "directions", "L_r(p, d) = D(p, d) + (M[d] - g)", "S(p, d)", "label(p)", "depth(p)",
                  "energy", "PRECONDITIONS"):
        assert words in section, words


def test_python_binding_exports_the_stage():
    from stereoreconstruction_amd import capi
    for name in NAMES:
        assert name in capi.EXPORTS
    m = capi.mvs_sgm_params()
    assert (m.beta, m.lambda_, m.phi_u, m.psi_u, m.path_mask) == (1.0, 1.0, 0.5, 0.002, 0xFF)
    m = capi.mvs_sgm_params(path_mask=0x0F, **{"lambda": 2.0})
    assert (m.lambda_, m.path_mask) == (2.0, 0x0F)
    for method in ("mvs_sgm_estimate", "mvs_initial_estimate_sgm", "mvs_sgm_estimate_views", "mvs_sgm_dims", "mvs_sgm_state"):
        assert callable(getattr(capi.Context, method))
