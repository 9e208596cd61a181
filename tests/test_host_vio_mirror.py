"""The host mirror of the camera ESIKF (csrc/host/imageProcessing.cpp: vioEsikf, vioPhotometric, both updateCameraParameters, through the
srl_lio_vio_* handles) on a box without a GPU: the measurement pass of every iteration is fed from tests/vio_checker.py's in-order sums
through the provider hook -- no device is involved -- and the states behind every iteration and the final covariances are compared with
those tests/vio_ref_reader.cpp recorded in tests/golden/golden_color_vio.npz: the reference's own pieces around the loop statements and
the literal solve with the explicit gain K (imageProcessing.cpp:361, :528) on the stand-in Eigen
(tests/test_vio_checker_reference.py holds the file to the reader).

The mirror solves from the sums (A = HtH + (J0 P J0^T w)^-1, K r = A^-1 Htr, K H = A^-1 HtH): the same algebra by another route, so the
comparison has a tolerance, and it is a measured one.  MEASURED is the largest difference (vio_checker.difference: per block of the state
vector relative to the block's largest magnitude, and of the covariance relative to its largest entry) over both scenes and both updates
against the reader on this tree, 5.1e-15 (scene 0, vioEsikf; the others 4.9e-15, 1.3e-15, 1.2e-15); the test allows 16 x that, because the
rounding of a different but equivalent solve route varies with the conditioning across scenes."""
import ctypes as C
import os

import numpy as np
import pytest

import render_checker as rk
import vio_checker as vc
import sr_livo_amd as srl
from sr_livo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED = 5.1e-15
TOLERANCE = 16 * MEASURED
SRL_ERR_BAD_ARG, SRL_ERR_NO_DEVICE = -3, -1


def _scene_from(base, args, points):
    cam = rk.Camera(tuple(args.cam.q_world_camera), tuple(args.cam.t_world_camera), args.cam.fx, args.cam.fy, args.cam.cx, args.cam.cy)
    return vc.Scene(base.position, base.n_rgb, base.cov, base.rgb, base.img, cam, args.time_td, list(args.R_imu_camera), points)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_color_vio.npz"), allow_pickle=False)


def golden_sequence(g, which):
    """((accepted, states, covariance, used) of vioEsikf, ... of vioPhotometric) as the reader recorded them"""
    return tuple((bool(g["s%d_%s_used" % (which, n)][0]), g["s%d_%s_states" % (which, n)], g["s%d_%s_cov" % (which, n)], int(g["s%d_%s_used" % (which, n)][1]))
                 for n in ("esikf", "photometric"))


def provider_for(base, calls):
    def provider(args, points, sums):
        res = vc.vio_rows(_scene_from(base, args, points), args.mode, bool(args.estimate_extrinsic), bool(args.estimate_intrinsic))
        vc.fill_sums(sums, res)
        calls.append((args.mode, res.counts))
        return capi.SRL_OK
    return provider


def run_sequence(lio, which, tracked=None):
    """vioEsikf then vioPhotometric through the handles from the scene's initial state: ((accepted, states, cov, used), ...)"""
    pts = vc.scene(which).points if tracked is None else tracked
    lio.vio_set_options(2, True, True)
    lio.vio_set_initial_cov()
    lio.vio_set_camera_state(vc.initial_state(which).vector())
    ok_a, st_a, used_a = lio.vio_esikf(pts, vc.NEW_VISITED_VOXELS)
    cov_a = lio.vio_get_cov()
    ok_b, st_b, used_b = lio.vio_photometric(pts, vc.NEW_VISITED_VOXELS)
    return (ok_a, st_a, cov_a, used_a), (ok_b, st_b, lio.vio_get_cov(), used_b)


@pytest.fixture()
def lio():
    handle = srl.Lio(-1)                  # a host-only object: no device behind it
    yield handle
    handle.close()


def test_initial_covariance_and_state_round_trip(lio):
    assert np.array_equal(lio.vio_get_cov(), vc.initial_cov())
    lio.vio_set_cov(np.arange(121.0).reshape(11, 11))
    assert np.array_equal(lio.vio_get_cov(), np.arange(121.0).reshape(11, 11))
    lio.vio_set_initial_cov()
    assert np.array_equal(lio.vio_get_cov(), vc.initial_cov())
    s = vc.initial_state(0).vector()
    assert len(s) == capi.CAMERA_STATE_DOUBLES == vc.STATE_DOUBLES
    lio.vio_set_camera_state(s)
    assert np.array_equal(lio.vio_get_camera_state(), s)


@pytest.mark.parametrize("which", range(len(vc.SCENE_RENDERS)))
def test_the_solve_from_sums_equals_the_readers_explicit_gain(lio, golden, which):
    calls = []
    lio.vio_set_rows_provider(provider_for(vc.scene(which), calls))
    got = run_sequence(lio, which)
    want = golden_sequence(golden, which)
    worst = 0.0
    for name, g, w in zip(("vioEsikf", "vioPhotometric"), got, want):
        assert g[0] == w[0] is True and len(g[1]) == len(w[1]) >= 1 and g[3] == w[3] >= 10, (name, g[0], len(g[1]), len(w[1]), g[3], w[3])
        d = vc.difference(g[1], g[2], w[1], w[2])
        print("scene %d %s: %d iterations, %d points used, largest difference %.3e" % (which, name, len(g[1]), g[3], d))
        worst = max(worst, d)
    assert [m for m, _ in calls] == [vc.REPROJECTION] * len(got[0][1]) + [vc.PHOTOMETRIC] * len(got[1][1])      # one pass per iteration
    assert worst <= TOLERANCE, worst
    assert np.array_equal(lio.vio_get_camera_state(), got[1][1][-1])
    # the photometric update leaves everything outside the 6 x 6 block of the extrinsics as vioEsikf left it
    outside = np.ones((11, 11), bool); outside[1:7, 1:7] = False
    assert np.array_equal(got[1][2][outside], got[0][2][outside]) and not np.array_equal(got[1][2], got[0][2])


def test_fewer_than_ten_tracked_points_return_at_once(lio):
    calls = []
    lio.vio_set_rows_provider(provider_for(vc.scene(0), calls))
    for (ok, states, cov, used) in run_sequence(lio, 0, vc.scene(0).points[:9]):
        assert not ok and len(states) == 0 and used == 0 and np.array_equal(cov, vc.initial_cov())
    assert calls == [] and np.array_equal(lio.vio_get_camera_state(), vc.initial_state(0).vector())


def test_the_gate_breaks_the_loop_and_the_covariance_update_runs_on_zeros(lio):
    """twelve tracked points of which nine are used: the loop breaks at the gate in its first iteration; K, H_mat and `solution` are the
    zeros the iteration began with, so J_k is the identity and the covariance comes back unchanged -- and the function returns true"""
    sc = vc.scene(0)
    used = sc.points[vc.scene_results(0)[0].outcome == vc.USED][:9]
    unknown = np.zeros(3, vc.POINT_DTYPE); unknown["pool"] = -1
    tracked = np.concatenate([used, unknown])
    calls = []
    lio.vio_set_rows_provider(provider_for(sc, calls))
    a, b = run_sequence(lio, 0, tracked)
    assert a[0] and len(a[1]) == 0 and a[3] == 9 and np.array_equal(a[2], vc.initial_cov())
    assert b[0] and len(b[1]) == 0 and b[3] < 10 and np.array_equal(b[2], vc.initial_cov())
    assert [m for m, _ in calls] == [vc.REPROJECTION, vc.PHOTOMETRIC] and np.array_equal(lio.vio_get_camera_state(), vc.initial_state(0).vector())


def test_without_estimation_the_configured_values_are_put_back(lio):
    """:224-236: with both switches off vioEsikf first writes camera_intrinsic and the configured extrinsics into the state"""
    sc = vc.scene(1)
    lio.vio_set_rows_provider(provider_for(sc, []))
    K = np.array([[200.0, 0, 250.0], [0, 201.0, 190.0], [0, 0, 1]])
    R, t = vc.r_imu_camera(), np.array([0.01, 0.02, 0.03])
    lio.vio_set_options(1, False, False, K, R, t)
    lio.vio_set_initial_cov()
    lio.vio_set_camera_state(vc.initial_state(1).vector())
    ok, states, _ = lio.vio_esikf(sc.points, vc.NEW_VISITED_VOXELS)
    assert ok and len(states) == 1
    s = vc.CameraState(states[0])
    # only the time offset has a column left: the rest of the solution is what the prior pulls back, zero from a zero d_x
    assert (s.fx, s.fy, s.cx, s.cy) == (200.0, 201.0, 250.0, 190.0) and np.allclose(s.R, R, atol=1e-12) and np.allclose(s.t, t, atol=1e-12)
    assert s.time_td != vc.TIME_TD


def test_refusals():
    lib = srl.load_library()
    h = C.c_void_p()
    assert lib.srl_lio_create(-1, C.byref(h)) == capi.SRL_OK
    try:
        pts = np.ascontiguousarray(vc.scene(0).points[:12])
        ok, it, used = C.c_int(5), C.c_int(5), C.c_int(5)
        for fn in (lib.srl_lio_vio_esikf, lib.srl_lio_vio_photometric):
            assert fn(h, capi._ptr(pts), 12, 800, C.byref(ok), C.byref(it), C.byref(used), None, 0) == SRL_ERR_NO_DEVICE      # never a host loop
            assert (ok.value, it.value, used.value) == (0, 0, 0)
            assert fn(None, capi._ptr(pts), 12, 800, C.byref(ok), None, None, None, 0) == SRL_ERR_BAD_ARG
            assert fn(h, capi._ptr(pts), 12, 800, None, None, None, None, 0) == SRL_ERR_BAD_ARG
            assert fn(h, None, 12, 800, C.byref(ok), None, None, None, 0) == SRL_ERR_BAD_ARG
            assert fn(h, capi._ptr(pts), -1, 800, C.byref(ok), None, None, None, 0) == SRL_ERR_BAD_ARG
            assert fn(h, capi._ptr(pts), 12, 800, C.byref(ok), None, None, None, 2) == SRL_ERR_BAD_ARG
        assert lib.srl_lio_vio_set_cov(h, None) == SRL_ERR_BAD_ARG and lib.srl_lio_vio_get_cov(None, None) == SRL_ERR_BAD_ARG
        assert lib.srl_lio_vio_set_camera_state(h, None) == SRL_ERR_BAD_ARG and lib.srl_lio_vio_set_options(h, -1, 1, 1, None, None, None) == SRL_ERR_BAD_ARG
    finally:
        lib.srl_lio_destroy(h)
