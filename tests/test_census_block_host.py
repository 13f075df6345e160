"""The library's device header srh_census_block.hpp (the census cost's blocks on the dense plan: the reference side's
settle, the fast-form and select-form sums, the finish) compiled for the host: tests/census_block_host.cpp, a program of
its own, built with g++ and linked to tests/census_restatement.cpp and oracle/liboracle.so.  Every pixel and candidate of
two small rectified pairs with ragged masks on both sides is held bit for bit to the restatement's cost_census, bad_ret
positions included, under the default weight cut-off, a raised one and a negative one.  Built a second time with
-fsanitize=address,undefined and run directly (its own program: nothing is preloaded)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_ffi as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stereoreconstruction_amd import synthetic  # noqa: E402

SRCS = [os.path.join(ROOT, "tests", "census_block_host.cpp"), os.path.join(ROOT, "tests", "census_restatement.cpp")]
FLAGS = ["-std=c++17", "-O1", "-ffp-contract=off"]
BUILDS = {"plain": [], "sanitized": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-g"]}
CASES = [(48, 24, 12, 5), (24, 16, 8, 2)]      # width, height, levels, window radius: the two radii the kernel instantiates


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    O.build_oracle()
    d = tmp_path_factory.mktemp("census_block_host")
    out = {}
    for name, extra in BUILDS.items():
        exe = str(d / ("census_block_host_" + name))
        subprocess.check_call(["g++"] + FLAGS + extra + ["-I" + O.ORACLE_DIR, "-I" + os.path.join(ROOT, "stereoreconstruction_amd", "csrc")]
                              + SRCS + ["-L" + O.ORACLE_DIR, "-l:liboracle.so", "-Wl,-rpath," + O.ORACLE_DIR, "-o", exe])
        out[name] = exe
    return out


def _ragged(rng, w, h, share):
    """a mask with about `share` of each row cleared in runs of 1 to 5 pixels"""
    m = np.ones((h, w), np.uint8)
    for y in range(h):
        x = 0
        while x < w:
            run = int(rng.integers(1, 6))
            if rng.random() < share:
                m[y, x:x + run] = 0
            x += run
    return m


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    """one file per case: a pair of synthetic.py's generator, ragged masks on both sides (the right one keeps its middle
    rows whole on the right half, so that fully usable windows exist)"""
    d = tmp_path_factory.mktemp("census_block_pairs")
    out = {}
    for w, h, levels, radius in CASES:
        left, right, _, _, _ = synthetic.rectified_pair(w, h, levels, seed=0xCE45 + w)
        rng = np.random.default_rng(0xB10C + w)
        ml, mr = _ragged(rng, w, h, 0.15), _ragged(rng, w, h, 0.2)
        mr[1:h - 1, w // 2:] = 1
        assert 0 < (ml == 0).sum() and 0 < (mr == 0).sum()
        path = str(d / ("pair_%dx%d.bin" % (w, h)))
        with open(path, "wb") as f:
            f.write(np.array([w, h], np.int32).tobytes())
            for a in (left, right, ml, mr):
                f.write(np.ascontiguousarray(a, np.uint8).tobytes())
        out[(w, h)] = path
    return out


@pytest.mark.parametrize("build", sorted(BUILDS))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_r%d" % (c[0], c[1], c[3]))
def test_census_block_header_matches_the_restatement(programs, pairs, case, build):
    w, h, _, radius = case
    r = subprocess.run([programs[build], pairs[(w, h)], str(radius)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
