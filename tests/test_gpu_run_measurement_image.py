"""A measurement with its camera frame through the mirror (srl_lio_run_measurement_image: lioOptimization::process with to_rendering,
lioOptimization.cpp:1037-1086) against the same measurement taken apart in this file: srl_lio_run_measurement, the camera-state
statements of :1053-1075 restated in Python FP64 in the mirror's operation order, and srl_lio_image_process.

The synthetic sequence is the replay tests' (synth.make_sequence, 12 000 points per sweep); every measurement carries an image and the
run ends behind the fourth processed frame.  Frames 1 - 2 take the configured intrinsics and extrinsics (all_cloud_frame.size() < 3),
frames 3 - 4 inherit what the camera updates of the frame before left, and the two differ.  Both sides agree BYTEWISE after every
frame on the replay's record, the filter, the camera state and covariance, both pose maps, the totals, the refreshed candidates and the
registered colours.  With no image the call is srl_lio_run_measurement, byte for byte.  One handle at a time: the replay's
initialisation flag and G_norm belong to the process, and every handle here starts from the values a process starts with."""
import functools
import math

import numpy as np
import pytest

import flow_checker as fc
import sr_livo_amd as srl
from sr_livo_amd import capi, synth

pytestmark = pytest.mark.gpu
ROWS, COLS = 120, 160
K = (88.0, 89.5, 81.25, 58.5)                            # fx fy cx cy
R_IC = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])      # the camera looks along the body's x axis
T_IC = np.array([0.05, -0.02, 0.03])
OO = dict(init_voxel_size=0.2, init_sample_voxel_size=1.0, init_num_frames=6, num_for_initialization=10, voxel_size=0.2, sample_voxel_size=1.5,
          max_num_points_in_voxel=20, min_distance_points=0.1, motion_compensation=capi.MC_CONSTANT_VELOCITY, initialization=0, point_time_enable=1,
          acc_cov=0.1, gyr_cov=0.1, b_acc_cov=1e-4, b_gyr_cov=1e-4)
FRAMES = 4


@functools.lru_cache(maxsize=None)
def _sequence():
    _, L = synth.map_candidates(555, 60_000)
    return synth.make_sequence(31, 2, 12_000, L)[0]


@functools.lru_cache(maxsize=None)
def _image(k):
    g = fc.crop(fc.texture(92, ROWS, COLS), ROWS, COLS, -(k % 8), -((2 * k) % 16)).astype(np.int64)
    img = np.clip(np.stack([g, (g * 3) // 4 + 30, 255 - (g * 2) // 3], axis=-1), 0, 255).astype(np.uint8)
    img.setflags(write=False)
    return img


# ---- the mirror's quaternion and 3 x 3 statements (csrc/host/srl_la.h), operation for operation, on Python floats
def _rotation_matrix(q):
    w, x, y, z = (float(v) for v in q)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def _quaternion(m):
    t = m[0][0] + m[1][1] + m[2][2]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return [w, (m[2][1] - m[1][2]) * t, (m[0][2] - m[2][0]) * t, (m[1][0] - m[0][1]) * t]
    i = 1 if m[1][1] > m[0][0] else 0                   # Shepperd's branches for a non-positive trace: the largest diagonal element
    if m[2][2] > m[i][i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = math.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
    v = [0.0, 0.0, 0.0]
    v[i] = 0.5 * t
    t = 0.5 / t
    w = (m[k][j] - m[j][k]) * t
    v[j] = (m[j][i] + m[i][j]) * t
    v[k] = (m[k][i] + m[i][k]) * t
    return [w] + v


def _matmul(x, y):
    return [[(x[i][0] * y[0][j] + x[i][1] * y[1][j]) + x[i][2] * y[2][j] for j in range(3)] for i in range(3)]


def _matvec(x, v):
    return [(x[i][0] * v[0] + x[i][1] * v[1]) + x[i][2] * v[2] for i in range(3)]


def _lio(with_camera):
    lio = srl.Lio(0)
    lio.set_initial_flag(False)
    lio.set_g_norm(9.81)                                 # process-global like the flag: every replay of this file starts where a process starts
    lio.set_odometry_options(icp=srl.default_opts(max_num_residuals=600), **OO)
    if with_camera:
        lio.set_color_map_options(capi.default_color_opts())
        lio.vio_set_options(2, True, True, np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]]), R_IC, T_IC)
        lio.image_set_options(image_width=COLS, image_height=ROWS, track_windows_size=8.0)
    return lio


def _snapshot(lio, r, image):
    oft = lio.image_oft()
    return dict(state=np.asarray(r["state"], np.float64).tobytes(), counts=(r["success"], r["num_residuals"], r["iters"], r["frame_points"], r["keypoints"],
                                                                            r["points_added"], r["index_frame"]),
                eskf=lio.eskf_get_state().tobytes() + lio.eskf_get_cov().tobytes(), camera=lio.vio_get_camera_state().tobytes(),
                cov=lio.vio_get_cov().tobytes(), poses=(oft.pose_map(0).tobytes(), oft.pose_map(1).tobytes()), sizes=oft.sizes(),
                image=bytes(image), candidates=lio.image_candidates().tobytes(), rgb=tuple(a.tobytes() for a in lio.ctx.color_registered_rgb()),
                map=tuple(a.tobytes() for a in lio.ctx.map_download()), last=lio.image_time_last_process())


def _args(ms):
    return (ms["time_frame"], ms["imu_t"], ms["imu_acc"], ms["imu_gyr"], ms["pts_raw"], ms["pts_timestamp"], ms["time_sweep_begin"], ms["time_sweep_offset"])


@functools.lru_cache(maxsize=None)
def _one_call():
    """srl_lio_run_measurement_image over the sequence: a snapshot behind each of the first four processed frames"""
    lio, out = _lio(True), []
    try:
        for k, ms in enumerate(_sequence()):
            r = lio.run_measurement_image(*_args(ms), _image(k))
            assert r["rc"] == 0
            if not r["processed"]:
                assert bytes(r["image"]) == bytes(len(bytes(r["image"])))      # no camera frame while the filter initialises
                continue
            out.append((k, _snapshot(lio, r, r["image"]), r["image"], lio.vio_get_camera_state()))
            if len(out) == FRAMES:
                break
        return out
    finally:
        lio.set_initial_flag(False)
        lio.close()


def test_the_one_call_equals_the_measurement_the_camera_statements_and_the_camera_frame():
    want = _one_call()
    assert len(want) == FRAMES
    lio, n = _lio(True), 0
    try:
        configured = np.concatenate([R_IC.ravel(), T_IC, K])
        for k, ms in enumerate(_sequence()):
            lio.set_color_times(time_last_process=lio.image_time_last_process(), to_rendering=True)
            r = lio.run_measurement(*_args(ms))
            assert r["rc"] == 0
            if not r["processed"]:
                continue
            s = lio.vio_get_camera_state()
            if n < 2:                                    # :1053-1061: all_cloud_frame holds fewer than three frames
                s[1:17] = configured
            else:                                        # :1062-1071: the frame's before -- and not the configured ones any more
                assert not np.array_equal(s[1:17], configured)
            q, t = r["state"][0:4], r["state"][4:7]
            R = _rotation_matrix(q)
            s[24:28], s[28:31] = q, t
            s[17:21] = _quaternion(_matmul(R, s[1:10].reshape(3, 3).tolist()))                          # :1073
            s[21:24] = [a + b for a, b in zip(_matvec(R, s[10:13].tolist()), t)]                          # :1074
            lio.vio_set_camera_state(s)
            res = lio.image_process(_image(k), ms["time_sweep_begin"] + ms["time_sweep_offset"], r["index_frame"] - 1)
            got = _snapshot(lio, r, res)
            kw, w, wres, _ = want[n]
            assert kw == k
            print(f"frame {n + 1}: after flow {res.tracked_after_flow}, after PnP {res.tracked_after_pnp}, accepted {res.pnp_accepted}, "
                  f"updates {res.esikf_iterations} {res.photometric_iterations}, candidates {res.refreshed_candidates}")
            for name in w:
                if got[name] != w[name] and name in ("state", "camera", "eskf"):
                    print(name, np.frombuffer(got[name], np.float64) - np.frombuffer(w[name], np.float64))
                assert got[name] == w[name], (n, name)
            n += 1
            if n == FRAMES:
                break
        assert n == FRAMES
        # the camera updates ran, so that frames 3 - 4 inherited something: both gates were passed in the frames before them
        assert all(res.pnp_accepted and res.esikf_iterations >= 1 for _, _, res, _ in want[:3])
        assert not np.array_equal(want[1][3][1:17], configured) and not np.array_equal(want[1][3][1:17], want[2][3][1:17])
    finally:
        lio.set_initial_flag(False)
        lio.close()


def test_without_an_image_it_is_run_measurement():
    results = []
    for with_image_call in (True, False):
        lio, frames = _lio(True), []
        try:
            for ms in _sequence():
                r = lio.run_measurement_image(*_args(ms), None) if with_image_call else lio.run_measurement(*_args(ms))
                assert r["rc"] == 0
                if r["processed"]:
                    frames.append((np.asarray(r["state"]).tobytes(), r["points_added"], r["iters"], lio.eskf_get_cov().tobytes(), lio.ctx.color_map_size(),
                                   tuple(a.tobytes() for a in lio.ctx.map_download())))
                    if len(frames) == FRAMES:
                        break
            assert lio.image_time_last_process() == -1e5 and lio.image_oft().sizes() == (0, 0, 0, 0)
            results.append(frames)
        finally:
            lio.set_initial_flag(False)
            lio.close()
    assert len(results[0]) == FRAMES and results[0] == results[1]


def test_refusals():
    lio = _lio(False)
    try:
        ms = _sequence()[0]
        img = np.zeros((ROWS, COLS, 3), np.uint8)
        rc = lio.lib.srl_lio_run_measurement_image(None, 0.0, None, None, None, 0, None, None, 0, 0.0, 0.0, capi._ptr(img), ROWS, COLS, 3 * COLS, None, None)
        assert rc == capi.SRL_ERR_BAD_ARG
        with pytest.raises(srl.SrlError) as e:           # no options for the camera frame: refused before the sweep is touched
            lio.run_measurement_image(*_args(ms), img)
        assert e.value.status == capi.SRL_ERR_BAD_ARG
        lio.image_set_options(image_width=COLS, image_height=ROWS)
        for bad in (dict(rows=0), dict(cols=0), dict(stride=3 * COLS - 1)):
            a = dict(rows=ROWS, cols=COLS, stride=3 * COLS)
            a.update(bad)
            it, ia, ig = (np.ascontiguousarray(ms[n], np.float64) for n in ("imu_t", "imu_acc", "imu_gyr"))
            rc = lio.lib.srl_lio_run_measurement_image(lio.h, ms["time_frame"], capi._ptr(it), capi._ptr(ia), capi._ptr(ig), len(it), None, None, 0,
                                                       ms["time_sweep_begin"], ms["time_sweep_offset"], capi._ptr(img), a["rows"], a["cols"], a["stride"], None, None)
            assert rc == capi.SRL_ERR_BAD_ARG, bad
    finally:
        lio.set_initial_flag(False)
        lio.close()
