"""PointCloud2 messages through the host mirror (srl_lio_feed_pointcloud2 = lioOptimization::standardCloudHandler): last_end_time carried by
the handle, an overlap that drops a prefix, the refusals, queue growth across its first block, one FIFO shared with the Livox feed, and
two mirrors on one scripted stream -- one fed through srl_lio_feed_pointcloud2 + srl_lio_run_measurement_queued (the points never visit
the host), the other through srl_lio_run_measurement with the checker's decoded and cut arrays (tests/pc2_checker.py,
tests/livox_checker.py's PointQueue).  Per measurement every field of srl_replay_result and srl_lio_last_frame must be equal bitwise, and
the map size at the end.  One handle at a time: the replay's initialisation flag and G_norm belong to the process."""
import functools

import numpy as np
import pytest

import livox_cases as lc
import livox_checker as lk
import pc2_cases as pc
import pc2_checker as pk
import sr_livo_amd as srl
from sr_livo_amd import capi, synth

pytestmark = pytest.mark.gpu

T0, REST, DT, RATE = 1000.0, 3.3, 0.1, 200.0
SWEEPS = 6
BLIND, PFN = 0.5, 2
OO = dict(init_voxel_size=0.2, init_sample_voxel_size=0.5, init_num_frames=4, num_for_initialization=10, voxel_size=0.2, sample_voxel_size=0.5,
          max_num_points_in_voxel=20, min_distance_points=0.1, initialization=0, acc_cov=0.1, gyr_cov=0.1, b_acc_cov=1e-4, b_gyr_cov=1e-4)


def _opts(c):
    return srl.pc2_opts(c["lidar_type"], n_scans=c["n_scans"], scan_rate=c["scan_rate"], point_filter_num=c["pfn"], time_unit=c["unit"], blind=c["blind"])


def _records(d):
    return np.ascontiguousarray(np.concatenate([d["raw"], d["relative_time"][:, None], d["timestamp"][:, None]], axis=1))


def _same(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def _lio(mode=capi.MC_IMU, enable=True):
    lio = srl.Lio(0)
    lio.set_initial_flag(False)
    lio.set_g_norm(9.81)
    lio.set_odometry_options(icp=srl.default_opts(max_num_residuals=600), motion_compensation=mode, point_time_enable=int(enable), **OO)
    lio.set_device_subsample(True)
    return lio


def _queue(lio):
    return _records(lio.ctx.points_queue_download())


@pytest.mark.parametrize("name", ["velo_overlap", "oust_overlap", "robo_dt_last_point_quirk", "yaw_first_point_quirk", "yaw_16_rings_two_messages"])
def test_messages_in_turn_carry_last_end_time_in_the_handle(name):
    c = pc.case_by_name(name)
    want = pk.decode_case(c)
    lio = _lio()
    try:
        lio.set_pc2_options(_opts(c))
        last_end, total = -1.0, np.empty((0, 5))
        for k, (m, w) in enumerate(zip(c["msgs"], want)):
            rep = lio.feed_pointcloud2(m["data"], m["layout"], m["stamp"])
            assert (rep["points"], rep["picked"], rep["appended"]) == (w["points"], w["picked"], w["appended"]), k
            assert _same(rep["last_end_time"], w["last_end_time"]), k
            if w["points"] > 0:
                last_end = w["last_end_time"]                                # an empty message leaves it as it was
            info = lio.points_info()
            assert info["last_time_lidar"] == m["stamp"] and _same(info["last_end_time"], last_end), k
            total = np.vstack([total, w["records"]])
            assert info["size"] == len(total)
        assert _queue(lio).tobytes() == total.tobytes()
        if name.endswith("overlap"):
            assert 0 < want[1]["appended"] < len(range(0, want[1]["points"], c["pfn"])) and not want[1]["all_pass"]      # a prefix was dropped
            assert want[1]["records"][0, 4] > want[0]["last_end_time"]
    finally:
        lio.set_initial_flag(False)
        lio.close()


def test_refusals_of_the_feed():
    c = pc.case_by_name("velo_size_65")
    m = c["msgs"][0]
    lio = _lio()
    try:
        with pytest.raises(srl.SrlError) as e:                               # no options yet
            lio.feed_pointcloud2(m["data"], m["layout"], m["stamp"])
        assert e.value.status == capi.SRL_ERR_BAD_ARG
        for bad in (srl.pc2_opts(capi.LIDAR_LIVOX), srl.pc2_opts(pc.VELO, point_filter_num=0), srl.pc2_opts(pc.VELO, time_unit_scale_value=0.0),
                    srl.pc2_opts(pc.VELO, blind=float("nan"))):
            with pytest.raises(srl.SrlError) as e:
                lio.set_pc2_options(bad)
            assert e.value.status == capi.SRL_ERR_BAD_ARG
        lio.set_pc2_options(_opts(c))
        lio.feed_pointcloud2(m["data"], m["layout"], m["stamp"])
        before = lio.points_info()
        assert before["size"] == 65
        for stamp in (m["stamp"], m["stamp"] - 0.5):                         # a message that is not newer than the last one: the reference's assert
            with pytest.raises(srl.SrlError) as e:
                lio.feed_pointcloud2(m["data"], m["layout"], stamp)
            assert e.value.status == capi.SRL_ERR_BAD_ARG
        r = pc.case_by_name("refused_velo_nan_time")["msgs"][0]              # refused on the device: neither time moves
        with pytest.raises(srl.SrlError) as e:
            lio.feed_pointcloud2(r["data"], r["layout"], m["stamp"] + 1.0)
        assert e.value.status == capi.SRL_ERR_BAD_ARG
        assert lio.points_info() == before
    finally:
        lio.set_initial_flag(False)
        lio.close()


def test_the_queue_grows_across_its_first_block():
    c = pc.case_by_name("robo_size_2049")
    m = c["msgs"][0]
    lio = _lio()
    try:
        # nanoseconds: the absolute stamp in last_end_time (the dt_last_point quirk) shrinks to 1.7 s, less than the 10 s between the messages
        lio.set_pc2_options(srl.pc2_opts(pc.ROBO, time_unit=3, blind=c["blind"]))
        total, last_end = np.empty((0, 5)), -1.0
        for k in range(3):                                                   # 2 049, 4 098 (beyond the 4 096-record block), 6 147
            w = pk.decode(m["data"], m["layout"], pc.ROBO, m["stamp"] + 10.0 * k, last_end, 16, 10, pk.time_unit_scale(3), c["blind"], 1)
            rep = lio.feed_pointcloud2(m["data"], m["layout"], m["stamp"] + 10.0 * k)
            assert rep["appended"] == w["appended"] == 2049
            last_end = w["last_end_time"]
            total = np.vstack([total, w["records"]])
            assert lio.points_info()["size"] == len(total)
            assert _queue(lio).tobytes() == total.tobytes(), k
    finally:
        lio.set_initial_flag(False)
        lio.close()


def test_a_livox_feed_and_a_pointcloud2_feed_keep_one_fifo():
    lio = _lio()
    try:
        lv = lc.make_message(300, 11, offset_step=300000)                    # nanoseconds: 90 ms
        lio.set_lidar_options(srl.livox_opts(n_scans=lc.N_SCANS, time_unit=3, blind=BLIND, point_filter_num=2))
        c = pc.case_by_name("velo_overlap")
        lio.set_pc2_options(_opts(c))
        a = lk.decode(lv, 1000.0, lc.N_SCANS, lk.time_unit_scale(3), BLIND, 2)
        rep = lio.feed_livox(lv, 1000.0)
        assert rep["appended"] == a["appended"] > 100 and _same(lio.points_info()["last_end_time"], a["last_end_time"])
        m = c["msgs"][0]
        # 60 ms later: the PointCloud2 message overlaps the Livox one's end, and the handle's last_end_time -- the Livox report's -- cuts it
        b = pk.decode(m["data"], m["layout"], pc.VELO, 1000.06, a["last_end_time"], c["n_scans"], c["scan_rate"], pk.time_unit_scale(c["unit"]), c["blind"], c["pfn"])
        rep = lio.feed_pointcloud2(m["data"], m["layout"], 1000.06)
        assert rep["appended"] == b["appended"] and 0 < b["appended"] < b["picked"]
        with pytest.raises(srl.SrlError):                                    # one last_time_lidar for both
            lio.feed_livox(lv, 1000.06)
        lv2 = lc.make_message(200, 12, offset_step=300000)
        d = lk.decode(lv2, 1000.3, lc.N_SCANS, lk.time_unit_scale(3), BLIND, 2)
        lio.feed_livox(lv2, 1000.3)
        info = lio.points_info()
        assert info["last_time_lidar"] == 1000.3 and _same(info["last_end_time"], d["last_end_time"])
        want = np.vstack([a["records"], b["records"], d["records"]])
        assert info["size"] == len(want) and _queue(lio).tobytes() == want.tobytes()
    finally:
        lio.set_initial_flag(False)
        lio.close()


@functools.lru_cache(maxsize=None)
def _stream():
    """-> (measurements, messages): measurement k = (time_frame, imu_t, imu_acc, imu_gyr, time_sweep_begin, time_sweep_offset),
    message k = (data, layout, stamp), a Velodyne message with per-point time holding the points of measurement k's sweep (one more message
    lies behind the last cut).  The sensor rests in a small synthetic room, as in tests/test_gpu_livox_stream.py."""
    rng = np.random.default_rng(78)
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
        p = pc.make_points(pc.VELO, n, 5000 + k)                              # distinct shuffled times within 90 ms, in seconds
        p["x"], p["y"], p["z"] = raw[:, 0].astype(np.float32), raw[:, 1].astype(np.float32), raw[:, 2].astype(np.float32)
        m = pc.message(pc.VELO, p, stamp=te - DT, height=4, row_pad=6)
        msgs.append((m["data"], m["layout"], m["stamp"]))
        if k <= SWEEPS:
            meas.append((te, it, acc, gyr, te - DT if k == 0 else tb, DT))
        tb = te
    return meas, msgs


STREAM_OPTS = dict(n_scans=16, scan_rate=10, point_filter_num=PFN, time_unit=0, blind=BLIND)


def _snapshot(lio, r):
    f = lio.last_frame() if r["processed"] else None
    return dict(counts=tuple((k, r[k]) for k in r if k != "state"), state=np.asarray(r["state"], np.float64).tobytes(),
                frame=None if f is None else tuple(f[k].tobytes() for k in ("raw_point", "point", "imu_point")),
                eskf=lio.eskf_get_state().tobytes(), map=lio.map_size())


def _queued(mode):
    meas, msgs = _stream()
    lio, out, infos = _lio(mode, True), [], []
    try:
        lio.set_pc2_options(srl.pc2_opts(pc.VELO, **STREAM_OPTS))
        rep = lio.feed_pointcloud2(*msgs[0])
        # isPointTimeEnable() is what the caller hands to the odometry options
        lio.set_odometry_options(icp=srl.default_opts(max_num_residuals=600), motion_compensation=mode, point_time_enable=rep["given_offset_time"], **OO)
        for k, (te, it, acc, gyr, tsb, tso) in enumerate(meas):
            rep = lio.feed_pointcloud2(*msgs[k + 1])                          # one message ahead of the cut
            assert rep["given_offset_time"] == 1
            info = lio.points_info()
            assert info["last_time_lidar"] == msgs[k + 1][2] and info["last_end_time"] == rep["last_end_time"]
            r = lio.run_measurement_queued(te, it, acc, gyr, te, tsb, tso)
            out.append(_snapshot(lio, r))
            infos.append((info["size"], info["front_timestamp"], info["back_timestamp"]))
        return out, infos, lio.points_info()["size"]
    finally:
        lio.set_initial_flag(False)
        lio.close()


def _from_arrays(mode):
    meas, msgs = _stream()
    lio, out, infos = _lio(mode, True), [], []
    q = lk.PointQueue()
    last_end = [-1.0]

    def push(m):
        w = pk.decode(m[0], m[1], pc.VELO, m[2], last_end[0], 16, 10, pk.time_unit_scale(0), BLIND, PFN)
        assert w["status"] == "ok" and w["given"] == 1
        last_end[0] = w["last_end_time"]
        q.push(w["records"])
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


@pytest.mark.parametrize("mode", [capi.MC_IMU, capi.MC_CONSTANT_VELOCITY])
def test_the_queued_stream_equals_the_stream_of_arrays_bitwise(mode):
    got, got_infos, got_left = _queued(mode)
    want, want_infos, want_left = _from_arrays(mode)
    assert len(got) == len(want) == SWEEPS + 1
    for k, (g, w) in enumerate(zip(got, want)):
        print(f"measurement {k}: {dict(w['counts'])} map {w['map']}")
        for name in w:
            assert g[name] == w[name], (k, name)
        assert got_infos[k][0] == want_infos[k][0] and np.float64(got_infos[k][1:]).tobytes() == np.float64(want_infos[k][1:]).tobytes()
    assert [dict(w["counts"])["processed"] for w in want] == [False] + [True] * SWEEPS
    assert all(dict(w["counts"])["frame_points"] > 100 for w in want[1:])
    assert got_left == want_left > 100 and got[-1]["map"] == want[-1]["map"] and want[-1]["map"] > 0
