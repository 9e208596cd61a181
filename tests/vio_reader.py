"""Builds and drives tests/vio_ref_reader.cpp: the reference's own pieces (cloudFrame::getRgb with gradients, refreshPoseForProjection,
numType::skewSymmetric / quatToSo3 / so3ToQuat, rgbPoint::getPosition / getRgb / getCovRgb) with the loop statements of vioEsikf and
vioPhotometric between them and the literal solve with the explicit K, all on the stand-in Eigen of oracle/ref_shim.  Compiled into a
temporary directory against the include arrangement of oracle/Makefile's `refpath` target and linked to oracle/_ref/libref_path.so, as
tests/select_ref_reader.cpp is; the reference's src/lioOptimization.cpp is compiled once more into the reader's library with
tests/stub_opencv in front (getRgb needs a cv::Mat with pixels, the stand-in of oracle/ref_shim has none).  Neither the reader's binary
nor anything of the reference is committed.  Used by tests/test_vio_checker_reference.py and tests/golden/make_golden_color_vio.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import vio_checker as vc
from oracle import pyref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
REF_TSL = os.path.join(REF, "thirdLibrary", "tessil-src", "include")
REF_HDRS = ("cloudMap", "utility", "eskfEstimator", "state", "parameters", "lioOptimization", "cloudProcessing")      # oracle/Makefile: REF_HDRS


def available():
    return pr.available() and os.path.exists(os.path.join(REF, "src", "lioOptimization.cpp")) and shutil.which("g++") is not None


def build(tmp):
    """compiles the reader into the directory `tmp`; returns the loaded library"""
    inc = os.path.join(str(tmp), "include")
    os.makedirs(inc)
    for h in REF_HDRS:
        os.symlink(os.path.join(REF, "include", h + ".h"), os.path.join(inc, h + ".h"))
    os.symlink(os.path.join(ROOT, "oracle", "ref_shim", "local", "imageProcessing.h"), os.path.join(inc, "imageProcessing.h"))
    out = os.path.join(str(tmp), "libvio_ref_reader.so")
    refdir = os.path.join(ROOT, "oracle", "_ref")
    cmd = ["g++", "-std=c++14", "-O1", "-fPIC", "-w", "-ffp-contract=off", "-shared", "-Wl,-Bsymbolic", "-I" + os.path.join(ROOT, "tests", "stub_opencv"),
           "-I" + os.path.join(ROOT, "oracle"), "-I" + inc, "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + REF_TSL, "-o", out,
           os.path.join(ROOT, "tests", "vio_ref_reader.cpp"), os.path.join(REF, "src", "lioOptimization.cpp"),
           "-L" + refdir, "-l:libref_path.so", "-Wl,-rpath," + refdir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    pr.load()
    lib = C.CDLL(out)
    p = C.c_void_p
    lib.vrr_rows.argtypes = [p, p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, p, p, p, p, p, p, p, p]
    lib.vrr_rows.restype = None
    lib.vrr_update.argtypes = [p, p, p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, p, p, p, p, p, p, p, C.c_int,
                               C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.vrr_update.restype = C.c_int
    return lib


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _list_arrays(scene, points):
    """the tracked list as the reader takes it: per entry whether the map holds the pool position, and the point's stored fields"""
    pool = points["pool"].astype(np.int64)
    known = ((pool >= 0) & (pool < scene.num_points)).astype(np.int32)
    at = np.where(known == 1, pool, 0)
    keep = known[:, None] == 1
    xyz = np.ascontiguousarray(np.where(keep, scene.position[at], 0).astype(np.float32))
    rgb = np.ascontiguousarray(np.where(keep, scene.rgb[at], 0).astype(np.int16))
    cov = np.ascontiguousarray(np.where(keep, scene.cov[at], 0).astype(np.float32))
    n_rgb = np.ascontiguousarray(np.where(known == 1, scene.n_rgb[at], 0).astype(np.int16))
    match_vel = np.ascontiguousarray(np.stack([points["match_u"], points["match_v"], points["vel_u"], points["vel_v"]], 1).astype(np.float64))
    return known, xyz, rgb, cov, n_rgb, match_vel


def scene_state(scene):
    """the 31 doubles of a camera state whose camera is the scene's (the IMU pose is not read by one iteration's loop)"""
    c = scene.camera
    return np.concatenate([[scene.time_td], scene.R, np.zeros(3), [c.fx, c.fy, c.cx, c.cy], c.q, c.t, [1.0, 0.0, 0.0, 0.0], np.zeros(3)]).astype(np.float64)


def rows(lib, scene, mode, estimate_extrinsic=True, estimate_intrinsic=True, points=None):
    """one iteration's loop through the reader: (rows (n, 24), outcome (n,))"""
    pts = scene.points if points is None else points
    n = len(pts)
    arrays = _list_arrays(scene, pts)
    out, outcome = np.zeros((n, 24)), np.full(n, 255, np.uint8)
    img = np.ascontiguousarray(scene.img)
    st = scene_state(scene)
    lib.vrr_rows(_vp(st), _vp(img), img.shape[0], img.shape[1], int(mode), int(bool(estimate_extrinsic)), int(bool(estimate_intrinsic)), n,
                 *[_vp(a) for a in arrays], _vp(out), _vp(outcome))
    return out, outcome


def update(lib, scene, state31, cov, mode, tracked, number_of_new_visited_voxel, num_iterations=2, estimate_intrinsic=True, estimate_extrinsic=True,
           capacity=16):
    """vioEsikf (mode 0) or vioPhotometric (mode 1) through the reader, the explicit K on the stand-in Eigen:
    (accepted, states behind every updateCameraParameters, covariance, used of the last iteration, state31 afterwards)"""
    st = np.array(state31, dtype=np.float64)
    cv = np.ascontiguousarray(np.array(cov, dtype=np.float64))
    arrays = _list_arrays(scene, tracked)
    img = np.ascontiguousarray(scene.img)
    states = np.zeros((capacity, vc.STATE_DOUBLES))
    it, used = C.c_int(), C.c_int()
    ok = lib.vrr_update(_vp(st), _vp(cv), _vp(img), img.shape[0], img.shape[1], int(mode), int(bool(estimate_extrinsic)), int(bool(estimate_intrinsic)),
                        int(num_iterations), int(number_of_new_visited_voxel), len(tracked), *[_vp(a) for a in arrays], _vp(states), capacity,
                        C.byref(it), C.byref(used))
    return bool(ok), states[:it.value].copy(), cv, used.value, st


def sequence(lib, which, tracked=None):
    """vioEsikf, then vioPhotometric on what it left, as the frame loop runs them (imageProcessing.cpp:149-153)"""
    base = vc.scene(which)
    pts = base.points if tracked is None else tracked
    a = update(lib, base, vc.initial_state(which).vector(), vc.initial_cov(), vc.REPROJECTION, pts, vc.NEW_VISITED_VOXELS)
    b = update(lib, base, a[4], a[2], vc.PHOTOMETRIC, pts, vc.NEW_VISITED_VOXELS)
    return a[:4], b[:4]
