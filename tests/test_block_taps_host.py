"""block_onepass_taps of the library's device header srh_block.hpp (the certified one-pass sums with the tap products
fma(w, l, -meanL)*w supplied by the row source, as the strip kernel's 8-wave form keeps them in LDS per tile) compiled for
the host: tests/block_taps_host.cpp, a program of its own, built with g++ and linked to oracle/liboracle.so and to the gray
plane of tests/f32_restatement.cpp.  P, Q, U and the finished value of every block of 8 adjacent fully usable candidates of
every fully usable pixel are held bit for bit to block_onepass and onepass_finish (which tests/test_block_host.py holds to
the select form and the certificate), on the pairs of that test.  Built a second time with -fsanitize=address,undefined and
run directly (its own program: nothing is preloaded)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_ffi as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stereoreconstruction_amd import synthetic  # noqa: E402

SRCS = [os.path.join(ROOT, "tests", "block_taps_host.cpp"), os.path.join(ROOT, "tests", "f32_restatement.cpp")]
FLAGS = ["-std=c++17", "-O1", "-ffp-contract=off"]
BUILDS = {"plain": [], "sanitized": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-g"]}
CASES = [(48, 24, 12, 5), (24, 16, 8, 2)]      # width, height, levels, window radius: the two radii the kernels instantiate


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    O.build_oracle()
    d = tmp_path_factory.mktemp("block_taps_host")
    out = {}
    for name, extra in BUILDS.items():
        exe = str(d / ("block_taps_host_" + name))
        subprocess.check_call(["g++"] + FLAGS + extra + ["-I" + O.ORACLE_DIR, "-I" + os.path.join(ROOT, "stereoreconstruction_amd", "csrc"),
                                                         "-I" + os.path.join(ROOT, "include")]
                              + SRCS + ["-L" + O.ORACLE_DIR, "-l:liboracle.so", "-Wl,-rpath," + O.ORACLE_DIR, "-o", exe])
        out[name] = exe
    return out


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    """one file per case: a pair of synthetic.py's generator with a 3x3 masked hole in each view"""
    d = tmp_path_factory.mktemp("block_taps_pairs")
    out = {}
    for w, h, levels, _ in CASES:
        left, right, ml, mr, _ = synthetic.rectified_pair(w, h, levels, seed=0x5eed + w)
        ml[3:6, 7:10] = 0
        mr[2:5, 14:17] = 0
        path = str(d / ("pair_%dx%d.bin" % (w, h)))
        with open(path, "wb") as f:
            f.write(np.array([w, h], np.int32).tobytes())
            for a in (left, right, ml, mr):
                f.write(np.ascontiguousarray(a, np.uint8).tobytes())
        out[(w, h)] = path
    return out


@pytest.mark.parametrize("build", sorted(BUILDS))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_r%d" % (c[0], c[1], c[3]))
def test_supplied_tap_products_give_the_one_pass_bits(programs, pairs, case, build):
    w, h, _, radius = case
    r = subprocess.run([programs[build], pairs[(w, h)], str(radius)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
    assert " 0 uncertified" in r.stdout
