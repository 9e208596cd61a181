"""The sequential restatement of the selection for projection (tests/select_checker.py) pinned to the reference's own pieces, bit for bit.

rgbMapTracker::selectPointsForProjection itself cannot be compiled against the stand-ins of oracle/ (the include mirror shadows
rgbMapTracker, the stand-in OpenCV has no Point2f).  tests/select_ref_reader.cpp drives what can: the reference's own Hash_map_2d<int,
int> / <int, float> holding the mask, cloudFrame::project3dPointInThisImage and Eigen's norm(), with the mask update written out between
them; compiled here, into the test's temporary directory, against a temporary include mirror of symlinks as oracle/Makefile's `refpath`
target builds one and linked to oracle/_ref/libref_path.so.  Neither the reader's binary nor anything of the reference is committed; the
tests skip where the reference tree or the library is absent.  Compared per candidate: the outcome, the cell key, the depth; per call:
the holders."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import render_checker as rk
import select_checker as sk
from oracle import pyref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
REF_TSL = os.path.join(REF, "thirdLibrary", "tessil-src", "include")
REF_HDRS = ("cloudMap", "utility", "eskfEstimator", "state", "parameters", "lioOptimization", "cloudProcessing")      # oracle/Makefile: REF_HDRS

pytestmark = pytest.mark.skipif(
    not pr.available() or not os.path.exists(os.path.join(REF, "include", "lioOptimization.h")) or shutil.which("g++") is None,
    reason="needs oracle/_ref/libref_path.so, the reference tree and g++")


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("select_ref_reader")
    inc = tmp / "include"
    inc.mkdir()
    for h in REF_HDRS:
        os.symlink(os.path.join(REF, "include", h + ".h"), inc / (h + ".h"))
    os.symlink(os.path.join(ROOT, "oracle", "ref_shim", "local", "imageProcessing.h"), inc / "imageProcessing.h")
    out = tmp / "libselect_ref_reader.so"
    refdir = os.path.join(ROOT, "oracle", "_ref")
    cmd = ["g++", "-std=c++14", "-O1", "-fPIC", "-w", "-ffp-contract=off", "-shared", "-I" + os.path.join(ROOT, "oracle"), "-I" + str(inc),
           "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + REF_TSL, "-o", str(out), os.path.join(ROOT, "tests", "select_ref_reader.cpp"),
           "-L" + refdir, "-l:libref_path.so", "-Wl,-rpath," + refdir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    pr.load()
    lib = C.CDLL(str(out))
    p = C.c_void_p
    lib.srr_select.argtypes = [p, C.c_int, C.c_int, C.c_int, p, C.c_double, C.c_int, C.c_double, C.c_double, p, p, p, p]
    lib.srr_select.restype = C.c_int
    return lib


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _compare(reader, smap, cam, rows, cols, voxels, md, skip, use_all, dmin=sk.MINIMUM_DEPTH, dmax=sk.MAXIMUM_DEPTH):
    cand, _ = smap.candidates(voxels, use_all)
    n = len(cand)
    xyz = np.array([c[0] for c in cand], np.float32).reshape(n, 3)
    cam12 = np.array(list(cam.q) + list(cam.t) + [cam.fx, cam.fy, cam.cx, cam.cy, cam.fov_margin])
    outcome = np.zeros(n, np.uint8); key = np.zeros((n, 2), np.int32); depth = np.zeros(n); holder = np.zeros(n, np.uint8)
    cells = reader.srr_select(_vp(cam12), rows, cols, n, _vp(xyz), md, skip, dmin, dmax, _vp(outcome), _vp(key), _vp(depth), _vp(holder))
    rec, tot, w_cells = sk.select_sequential(smap, cam, rows, cols, voxels, md, skip, use_all, dmin, dmax)
    assert cells == len(w_cells) == tot["selected"] == len(rec)
    assert np.array_equal(np.flatnonzero(holder), rec["index"])            # the holders
    assert ((outcome != 255).sum(), (outcome == 1).sum(), (outcome == 2).sum(), (outcome == 3).sum()) == \
        (tot["visited"], tot["far"], tot["near"], tot["behind"] + tot["outside"])
    seen = 0
    for cell, members in w_cells.items():
        for i, d in members:
            assert outcome[i] == 0 and (int(key[i, 0]), int(key[i, 1])) == cell, (i, cell, key[i])      # the keys
            assert np.float64(d).tobytes() == depth[i].tobytes(), i                                     # the depths
            seen += 1
    assert seen == (outcome == 0).sum()
    return tot, w_cells


def test_the_list_mode_scenes_equal_the_reference(reader):
    smap, visited = sk.scene_map()
    negative = 0
    for k, s, m in sk.SEQUENCE:
        if k != (s + 2 * m) % len(rk.RENDERS):                             # one pose per parameter set and margin
            continue
        cam, rows, cols, lists = sk.scene_camera(k, sk.MARGINS[m])
        md, skip = sk.PARAMETER_SETS[s]
        tot, cells = _compare(reader, smap, cam, rows, cols, np.concatenate([visited[j] for j in lists]), md, skip, False)
        negative += sum(1 for c in cells if c[0] < 0 or c[1] < 0)
        assert tot["selected"] > 50
    assert negative > 0                                                    # keys left of / above the image under the negative margin


def test_all_points_the_shells_and_depth_limits_equal_the_reference(reader):
    for batches in (3, 4):
        cam, rows, cols, _ = sk.scene_camera(*sk.ALL_POINTS_CAMERAS[1])
        _compare(reader, sk.scene_map(batches)[0], cam, rows, cols, None, 10.0, 1, True)
    shell_map, _ = sk.shell_scene()
    tot, cells = _compare(reader, shell_map, sk.shell_camera(), sk.SHELL_ROWS, sk.SHELL_COLS, None, 10.0, 1, True)
    assert min(sk.rule_census(cells)[1:]) >= 20
    smap, visited = sk.scene_map()
    cam, rows, cols, lists = sk.scene_camera(0, 0.005)
    tot, _ = _compare(reader, smap, cam, rows, cols, visited[0], 10.0, 1, False, 14.0, 17.5)
    assert tot["far"] > 0 and tot["near"] > 0
