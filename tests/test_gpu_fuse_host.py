"""MultiViewStereo::fusedPointCloud of the Qt-free host class (tests/host_fuse_test.cpp) against the C-ABI's result for the
same run, and the PLY file with normals it writes; the old outputPLYFile overload keeps its bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cases
import test_gpu_host_api as HA
from stereoreconstruction_amd import capi

ROOT = HA.ROOT
HEADER_OLD = ["ply", "format ascii 1.0", None, "property float x", "property float y", "property float z",
              "property uchar diffuse_red", "property uchar diffuse_green", "property uchar diffuse_blue", "end_header"]
HEADER_NEW = HEADER_OLD[:6] + ["property float nx", "property float ny", "property float nz"] + HEADER_OLD[6:]


def build_host_program(out_dir):
    """tests/host_fuse_test.cpp against the host library and libstereo_recon_hip -> path of the program"""
    subprocess.check_call(["make", "-C", HA.HOST], stdout=subprocess.DEVNULL)
    exe = os.path.join(str(out_dir), "host_fuse_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + HA.HOST,
                           os.path.join(ROOT, "tests", "host_fuse_test.cpp"),
                           os.path.join(HA.HOST, "libstereo_recon_host.a"),
                           "-L" + HA.LIBDIR, "-lstereo_recon_hip", "-Wl,-rpath," + HA.LIBDIR, "-o", exe])
    return exe


def test_host_program_compiles_without_gpu(tmp_path):
    assert os.path.exists(build_host_program(tmp_path))
    src = open(os.path.join(ROOT, "tests", "host_fuse_test.cpp")).read()
    for member in ("fusedPointCloud(", "fuseParams(", "std::vector<FusedPoint>", "outputPLYFile("):
        assert member in src, member


def _read_fused(path, nv, w, h):
    raw = open(path, "rb").read()
    n = w * h * 8
    maps = [np.frombuffer(raw[i * n:(i + 1) * n], np.float64).reshape(h, w) for i in range(nv)]
    off = nv * n
    (k,) = struct.unpack_from("<i", raw, off)
    rec = np.dtype([("p", "<f8", 3), ("n", "<f8", 3), ("rgb", "u1", 3), ("nviews", "u1"), ("flags", "u1"), ("src", "<i4", 2)])
    assert rec.itemsize == 61
    return maps, np.frombuffer(raw[off + 4:off + 4 + k * rec.itemsize], rec)


def _g(values):
    return " ".join("%g" % v for v in values)                      # %g == ostream default formatting


@pytest.mark.gpu
def test_fused_cloud_of_the_host_class(tmp_path, hip_ctx):
    exe = build_host_program(tmp_path)
    case = cases.get_mvs("mvs_distorted")
    views = []
    for (rgba, mask, cam, dist, plane) in case["views"]:
        im = rgba.copy()
        im[..., 3] = np.where(mask == 1, 255, 51)                  # the class takes the mask from the alpha channel
        views.append((im, mask, cam, dist, plane))
    case = dict(case, views=views)
    h, w = views[0][0].shape[:2]
    nv = len(views)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    HA._write_input(inp, case, False)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    depths, rec = _read_fused(outp, nv, w, h)
    # the C-ABI on the same views and the class's depth maps
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    for v in range(nv):
        hip_ctx.upload_depth(v, depths[v])
    want = hip_ctx.mvs_fuse(list(range(nv)), p)
    assert want["n_points"] == len(rec) > 0
    assert np.array_equal(rec["p"].view(np.uint64), want["xyz"].view(np.uint64))
    assert np.array_equal(rec["n"].view(np.uint64), want["normals"].view(np.uint64))
    for a, b in (("rgb", "rgb"), ("nviews", "nviews"), ("flags", "flags"), ("src", "src")):
        assert np.array_equal(rec[a], want[b]), a
    # the PLY with normals: header, 9 fields per line, %g of the data
    lines = open(outp + ".fused.ply").read().split("\n")
    assert lines[-1] == ""
    head = [s if s is not None else "element vertex %d" % len(rec) for s in HEADER_NEW]
    assert lines[:len(head)] == head
    body = lines[len(head):-1]
    assert len(body) == len(rec)
    for line, q in zip(body, rec):
        assert len(line.split(" ")) == 9
        assert line == _g(q["p"]) + " " + _g(q["n"]) + " " + " ".join(str(int(c)) for c in q["rgb"])
    # the old overload for the same run: byte for byte the file the point cloud of view 0 has always given
    pc = hip_ctx.point_cloud(0, p)
    valid = pc["valid"].ravel() == 1
    xyz, rgb = pc["xyz"].reshape(-1, 3)[valid], pc["rgb"].reshape(-1, 3)[valid]
    head = [s if s is not None else "element vertex %d" % len(xyz) for s in HEADER_OLD]
    text = "\n".join(head + [_g(q) + " " + " ".join(str(int(c)) for c in col) for q, col in zip(xyz, rgb)]) + "\n"
    assert open(outp + ".view0.ply", "rb").read() == text.encode()
    # min_views is the class's to set: 1 keeps every point of every view, each once
    r = subprocess.run([exe, inp, outp, "1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    _, rec1 = _read_fused(outp, nv, w, h)
    want1 = hip_ctx.mvs_fuse(list(range(nv)), p, capi.fuse_params(min_views=1))
    assert len(rec1) == want1["n_points"] > len(rec) and want1["n_unsupported"] == 0
    assert np.array_equal(rec1["p"].view(np.uint64), want1["xyz"].view(np.uint64))
