"""The sequential restatement of the render loop (tests/render_checker.py) pinned to the reference's own translation units, bit for bit.

oracle/_ref/libref_path.so holds src/cloudMap.cpp and src/lioOptimization.cpp compiled where they lie; the harness exports neither
rgbPoint::updateRgb nor cloudFrame's projection.  tests/render_ref_reader.cpp drives them: compiled here, into the test's temporary
directory, against a temporary include mirror of symlinks as oracle/Makefile's `refpath` target builds one and linked to
libref_path.so.  Neither the reader's binary nor anything of the reference is committed; the tests skip where the reference tree or the
library is absent.

The pixel fetch cannot be pinned this way: the stand-in cv::Mat of oracle/ref_shim has no pixels (and its Vec3b truncates; inert, since
nothing reaches it).  Its OpenCV semantics are pinned by the known answers of tests/test_render_checker.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import render_checker as rk
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
    tmp = tmp_path_factory.mktemp("render_ref_reader")
    inc = tmp / "include"
    inc.mkdir()
    for h in REF_HDRS:
        os.symlink(os.path.join(REF, "include", h + ".h"), inc / (h + ".h"))
    os.symlink(os.path.join(ROOT, "oracle", "ref_shim", "local", "imageProcessing.h"), inc / "imageProcessing.h")
    out = tmp / "librender_ref_reader.so"
    refdir = os.path.join(ROOT, "oracle", "_ref")
    cmd = ["g++", "-std=c++14", "-O1", "-fPIC", "-w", "-ffp-contract=off", "-shared", "-I" + os.path.join(ROOT, "oracle"), "-I" + str(inc),
           "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + REF_TSL, "-o", str(out), os.path.join(ROOT, "tests", "render_ref_reader.cpp"),
           "-L" + refdir, "-l:libref_path.so", "-Wl,-rpath," + refdir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    pr.load()
    lib = C.CDLL(str(out))
    p = C.c_void_p
    lib.rrr_update_rgb.argtypes = [C.c_int, p, p, p, p]
    lib.rrr_project.argtypes = [p, C.c_int, C.c_int, C.c_int, p, p, p, p]
    return lib


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _observations(seed, n):
    """colours 0 ... 255, distances that straddle the 1.2 gate of the running minimum, time steps that include 0 and negative ones"""
    rng = np.random.default_rng(seed)
    obs = np.zeros((n, 5))
    obs[:, :3] = rng.integers(0, 256, (n, 3))
    t, dmin = 100.0, None
    for k in range(n):
        kind = rng.random()
        if dmin is None:
            d = rng.uniform(20.0, 30.0)
        elif kind < 0.1:
            d = rng.uniform(0.5, 30.0)
        elif kind < 0.4:
            d = dmin * 1.2 * (1.0 + rng.choice([-1e-15, 0.0, 1e-15, 3e-16, -1e-3, 1e-3]))      # on and around the gate
        elif kind < 0.6:
            d = dmin * rng.uniform(1.2, 3.0)                                                    # refused
        else:
            d = dmin * rng.uniform(0.97, 1.19)                                                  # now and then a new minimum
        step = rng.choice([0.0, 0.1, 0.1, 0.05, 1.0, -0.05, -0.3, 1e-9, 7.3])
        t = t + step
        obs[k, 3], obs[k, 4] = d, t
        if dmin is None or (d <= dmin * 1.2 and d < dmin):
            dmin = d
    return obs


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_update_rgb_equals_the_reference_step_by_step(reader, seed):
    n = 12000
    obs = _observations(seed, n)
    out_int = np.zeros((n, 5), np.int32); out_cov = np.zeros((n, 3), np.float32); out_dbl = np.zeros((n, 2))
    reader.rrr_update_rgb(n, _vp(obs), _vp(out_int), _vp(out_cov), _vp(out_dbl))
    s = rk.RgbState()
    counts = {-1: 0, 0: 0, 1: 0}
    for k in range(n):
        r = s.update_rgb([float(obs[k, 0]), float(obs[k, 1]), float(obs[k, 2])], float(obs[k, 3]), float(obs[k, 4]))
        counts[r] += 1
        assert max(r, 0) == out_int[k, 0], k                                # the gate's return value is the reference's 0
        assert s.rgb == [int(v) for v in out_int[k, 1:4]] and s.n_rgb == out_int[k, 4], (k, s.rgb, out_int[k])
        assert np.array(s.cov, np.float32).tobytes() == out_cov[k].tobytes(), (k, s.cov, out_cov[k])
        assert np.array([s.observe_distance, s.last_observe_time]).tobytes() == out_dbl[k].tobytes(), k
    assert counts[0] == 1 and counts[-1] > 1000 and counts[1] > 5000
    steps = np.diff(obs[:, 4])
    assert (steps == 0).sum() > 100 and (steps < 0).sum() > 100


def _poses():
    """the scene's poses, and two that stand in the middle of the scene so that points fall behind the camera and past every bound"""
    for which in (0, 1):
        for pose in rk.POSES[:5]:
            yield rk.scene_camera(pose, which), which
    yield rk.scene_camera((2.5, -0.2, 0.3, (1.0, -1.0, 0.2)), 1), 1
    yield rk.Camera((0.3, -0.2, 0.9, 0.1), (0.5, 0.25, -0.4), 210.0, 190.0, 300.5, 200.25, 0.02), 0      # far from a unit quaternion: inverse() divides


def test_projection_equals_the_reference_for_every_stored_point(reader):
    chk, _ = rk.scene_map()
    xyz = chk.map_arrays()[3]
    first = {k: 0 for k in range(6)}
    for cam, which in _poses():
        rows, cols = rk.IMAGE_SIZES[which]
        cam12 = np.array(list(cam.q) + list(cam.t) + [cam.fx, cam.fy, cam.cx, cam.cy, cam.fov_margin])
        uv = np.zeros((len(xyz), 2)); accept = np.zeros(len(xyz), np.uint8); pose = np.zeros(7)
        reader.rrr_project(_vp(cam12), rows, cols, len(xyz), _vp(xyz), _vp(uv), _vp(accept), _vp(pose))
        # refreshPoseForProjection: t_camera_world bit for bit (the rotation is compared through every projected point)
        assert np.array(cam.t_cw).tobytes() == pose[4:].tobytes()
        for k in range(len(xyz)):
            p = (float(xyz[k, 0]), float(xyz[k, 1]), float(xyz[k, 2]))
            outcome, u, v = cam.project(p, rows, cols)
            first[outcome] += 1
            assert (outcome == 0) == bool(accept[k]), (k, outcome)
            if outcome != 1:                                                # behind the camera the reference leaves u, v untouched
                assert np.array([u, v]).tobytes() == uv[k].tobytes(), (k, u, v, uv[k])
    assert min(first.values()) >= 100, first                                # accepted, behind, and every bound of the field of view
