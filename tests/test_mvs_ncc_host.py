"""The library's device header srh_mvs_ncc.hpp (MultiViewStereo's select-form cost, the constants and sweeps of its fast
form, the peak rule) compiled for the host and held to the oracle bit for bit: tests/mvs_ncc_host.cpp, a program of its
own, built with g++ and linked to oracle/liboracle.so.  Built a second time with -fsanitize=address,undefined and run
directly (its own program: nothing is preloaded)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_ffi as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stereoreconstruction_amd import synthetic  # noqa: E402

SRCS = [os.path.join(ROOT, "tests", "mvs_ncc_host.cpp")]
FLAGS = ["-std=c++17", "-O1", "-ffp-contract=off"]
BUILDS = {"plain": [], "sanitized": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-g"]}
SHAPES = [(24, 16), (9, 4)]       # at 9x4 with radius 2 every window crosses the top or the bottom border


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    O.build_oracle()
    d = tmp_path_factory.mktemp("mvs_ncc_host")
    out = {}
    for name, extra in BUILDS.items():
        exe = str(d / ("mvs_ncc_host_" + name))
        subprocess.check_call(["g++"] + FLAGS + extra + ["-I" + O.ORACLE_DIR, "-I" + os.path.join(ROOT, "stereoreconstruction_amd", "csrc")]
                              + SRCS + ["-L" + O.ORACLE_DIR, "-l:liboracle.so", "-Wl,-rpath," + O.ORACLE_DIR, "-o", exe])
        out[name] = exe
    return out


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    """one file per shape: a pair of synthetic.py's generator with a 3x3 masked hole in each view and a black 7x7 patch
    at the same place in both (clipped to the image): windows inside it have sum2 = sum3 = 0"""
    d = tmp_path_factory.mktemp("mvs_ncc_pairs")
    out = []
    for w, h in SHAPES:
        left, right, ml, mr, _ = synthetic.rectified_pair(w, h, 8, seed=0x5eed + w)
        ml[1:4, 1:4] = 0
        mr[0:3, 5:8] = 0
        for img in (left, right):
            img[2:9, 1:8, :3] = 0
        path = str(d / ("pair_%dx%d.bin" % (w, h)))
        with open(path, "wb") as f:
            f.write(np.array([w, h], np.int32).tobytes())
            for a in (left, right, ml, mr):
                f.write(np.ascontiguousarray(a, np.uint8).tobytes())
        out.append(path)
    return out


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_mvs_ncc_header_matches_the_oracle_bit_for_bit(programs, pairs, build):
    # (both shapes in one run: the program's tallies of what its cases met are taken over all of them)
    r = subprocess.run([programs[build]] + pairs, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
