"""Two host mirrors on one scripted stream of Livox messages: one is fed through srl_lio_feed_livox + srl_lio_run_measurement_queued (the
points never visit the host), the other through srl_lio_run_measurement with the checker's decoded and cut arrays
(tests/livox_checker.py).  Per measurement every field of srl_replay_result and srl_lio_last_frame must be equal bitwise, and the map
size at the end.  One handle at a time: the replay's initialisation flag and G_norm belong to the process, and every handle here starts
from the values a process starts with.

The stream: the sensor rests in a small synthetic room (synth.py).  Measurement 0 carries 3.3 s of IMU samples (the filter initialises
in that one call; its sweep is dropped as the reference drops it), six measurements of 0.1 s follow.  Eight messages; every message is
fed one measurement AHEAD of the cut that consumes it, so each cut is a true prefix of a queue that holds more."""
import functools

import numpy as np
import pytest

import livox_cases as lc
import livox_checker as lk
import sr_livo_amd as srl
from sr_livo_amd import capi, synth

pytestmark = pytest.mark.gpu

T0, REST, DT, RATE = 1000.0, 3.3, 0.1, 200.0
SWEEPS = 6
UNIT, BLIND, PFN = 2, 0.5, 2          # microseconds
OO = dict(init_voxel_size=0.2, init_sample_voxel_size=0.5, init_num_frames=4, num_for_initialization=10, voxel_size=0.2, sample_voxel_size=0.5,
          max_num_points_in_voxel=20, min_distance_points=0.1, initialization=0, acc_cov=0.1, gyr_cov=0.1, b_acc_cov=1e-4, b_gyr_cov=1e-4)


@functools.lru_cache(maxsize=None)
def _stream():
    """-> (measurements, messages): measurement k = (time_frame, imu_t, imu_acc, imu_gyr, time_sweep_begin, time_sweep_offset),
    message k = (points, stamp), the points of measurement k's sweep (one more message lies behind the last cut)"""
    rng = np.random.default_rng(77)
    _, L = synth.map_candidates(555, 1000)
    q0 = synth.quat_from_rotvec([0.0, 0.0, 0.4]); p0 = np.array([2.1, 1.3, 0.05])
    meas, msgs = [], []
    tb = T0
    for k in range(SWEEPS + 2):
        span = REST if k == 0 else DT
        te = tb + span
        n_imu = int(round(RATE * span))
        it = tb + (np.arange(n_imu) + 1) / RATE
        acc = np.array([0.0, 0.0, 9.81]) + rng.normal(0, 0.02, (n_imu, 3))
        gyr = np.array([0.001, -0.0005, 0.0008]) + rng.normal(0, 0.002, (n_imu, 3))
        n = 300 if k == 0 else 1200
        raw = synth.sweep_from_pose(rng, n, L, q0, p0)
        msg = lc.make_message(n, 4000 + k, offset_step=99000 // n)             # lines, distinct shuffled offsets within 99 ms
        msg["x"], msg["y"], msg["z"] = raw[:, 0].astype(np.float32), raw[:, 1].astype(np.float32), raw[:, 2].astype(np.float32)
        msg.setflags(write=False)
        msgs.append((msg, te - DT))
        if k <= SWEEPS:
            meas.append((te, it, acc, gyr, te - DT if k == 0 else tb, DT))
        tb = te
    return meas, msgs


def _lio(mode, enable):
    lio = srl.Lio(0)
    lio.set_initial_flag(False)
    lio.set_g_norm(9.81)
    lio.set_odometry_options(icp=srl.default_opts(max_num_residuals=600), motion_compensation=mode, point_time_enable=int(enable), **OO)
    lio.set_device_subsample(True)
    return lio


def _snapshot(lio, r):
    f = lio.last_frame() if r["processed"] else None
    return dict(counts=tuple((k, r[k]) for k in r if k != "state"), state=np.asarray(r["state"], np.float64).tobytes(),
                frame=None if f is None else tuple(f[k].tobytes() for k in ("raw_point", "point", "imu_point")),
                eskf=lio.eskf_get_state().tobytes(), map=lio.map_size())


def _queued(mode, enable):
    meas, msgs = _stream()
    lio, out, infos = _lio(mode, enable), [], []
    try:
        lio.set_lidar_options(srl.livox_opts(n_scans=lc.N_SCANS, time_unit=UNIT, blind=BLIND, point_filter_num=PFN))
        lio.feed_livox(*msgs[0])
        for k, (te, it, acc, gyr, tsb, tso) in enumerate(meas):
            rep = lio.feed_livox(*msgs[k + 1])                               # one message ahead of the cut
            info = lio.points_info()
            assert info["last_time_lidar"] == msgs[k + 1][1] and info["last_end_time"] == rep["last_end_time"]
            r = lio.run_measurement_queued(te, it, acc, gyr, te, tsb, tso)
            out.append(_snapshot(lio, r))
            infos.append((info["size"], info["front_timestamp"], info["back_timestamp"]))
        return out, infos, lio.points_info()["size"]
    finally:
        lio.set_initial_flag(False)
        lio.close()


def _from_arrays(mode, enable):
    meas, msgs = _stream()
    lio, out, infos = _lio(mode, enable), [], []
    q = lk.PointQueue()

    def push(m):
        q.push(lk.decode(m[0], m[1], lc.N_SCANS, lk.time_unit_scale(UNIT), BLIND, PFN)["records"])
    try:
        push(msgs[0])
        for k, (te, it, acc, gyr, tsb, tso) in enumerate(meas):
            push(msgs[k + 1])
            infos.append(q.info())
            cut = q.cut(te)
            assert len(cut) > 100
            r = lio.run_measurement(te, it, acc, gyr, cut[:, 0:3], cut[:, 4], tsb, tso)
            out.append(_snapshot(lio, r))
        return out, infos, q.info()[0]
    finally:
        lio.set_initial_flag(False)
        lio.close()


@pytest.mark.parametrize("mode,enable", [(capi.MC_IMU, True), (capi.MC_CONSTANT_VELOCITY, False)])
def test_the_queued_stream_equals_the_stream_of_arrays_bitwise(mode, enable):
    got, got_infos, got_left = _queued(mode, enable)
    want, want_infos, want_left = _from_arrays(mode, enable)
    assert len(got) == len(want) == SWEEPS + 1
    for k, (g, w) in enumerate(zip(got, want)):
        print(f"measurement {k}: {dict(w['counts'])} map {w['map']}")
        for name in w:
            assert g[name] == w[name], (k, name)
        assert got_infos[k][0] == want_infos[k][0] and np.float64(got_infos[k][1:]).tobytes() == np.float64(want_infos[k][1:]).tobytes()
    assert [dict(w["counts"])["processed"] for w in want] == [False] + [True] * SWEEPS
    assert all(dict(w["counts"])["frame_points"] > 100 for w in want[1:])
    assert got_left == want_left > 100 and got[-1]["map"] == want[-1]["map"] and want[-1]["map"] > 0


def test_the_unsupported_configuration_and_the_empty_cut():
    meas, msgs = _stream()
    lio = _lio(capi.MC_IMU, True)
    try:
        te, it, acc, gyr, tsb, tso = meas[0]
        with pytest.raises(srl.SrlError) as e:                               # no options yet
            lio.feed_livox(*msgs[0])
        assert e.value.status == capi.SRL_ERR_BAD_ARG
        lio.set_lidar_options(srl.livox_opts(n_scans=lc.N_SCANS, time_unit=UNIT, blind=BLIND, point_filter_num=PFN))
        lio.feed_livox(*msgs[0])
        with pytest.raises(srl.SrlError) as e:                               # a message that is not newer than the last one
            lio.feed_livox(*msgs[0])
        assert e.value.status == capi.SRL_ERR_BAD_ARG
        size = lio.points_info()["size"]
        assert size > 100
        lio.set_device_subsample(False)
        with pytest.raises(srl.SrlError) as e:
            lio.run_measurement_queued(te, it, acc, gyr, te, tsb, tso)
        assert e.value.status == capi.SRL_ERR_UNSUPPORTED and lio.points_info()["size"] == size      # the queue is left uncut
        lio.set_device_subsample(True)
        lio.set_odometry_options(icp=srl.default_opts(max_num_residuals=600), motion_compensation=capi.MC_IMU, point_time_enable=1,
                                 **dict(OO, voxel_size=0.0))
        with pytest.raises(srl.SrlError) as e:
            lio.run_measurement_queued(te, it, acc, gyr, te, tsb, tso)
        assert e.value.status == capi.SRL_ERR_UNSUPPORTED and lio.points_info()["size"] == size
        lio.set_odometry_options(icp=srl.default_opts(max_num_residuals=600), motion_compensation=capi.MC_IMU, point_time_enable=1, **OO)
        # a cut in front of the queue's front: no lidar points, no Measurements element -- nothing changes, the IMU samples included
        before = lio.eskf_init_stats()["num_init_meas"]
        r = lio.run_measurement_queued(te, it, acc, gyr, msgs[0][1] - 1.0, tsb, tso)
        assert not r["processed"] and not r["initialized"] and r["index_frame"] == 0 and lio.points_info()["size"] == size
        assert lio.eskf_init_stats()["num_init_meas"] == before              # tryInit saw nothing
        r = lio.run_measurement_queued(te, it, acc, gyr, te, tsb, tso)       # the same measurement with its sweep: the filter initialises
        assert r["initialized"] and not r["processed"] and lio.points_info()["size"] == 0
    finally:
        lio.set_initial_flag(False)
        lio.close()
