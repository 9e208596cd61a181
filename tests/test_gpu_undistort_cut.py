"""srl_frame_undistort_cut -- the time rewrite, the IMU intervals and the undistortion of the resident cut on the device -- against the
existing srl_frame_undistort (itself pinned to the reference, tests/test_gpu_undistort_edges.py) fed the checker's rewritten arrays
(tests/livox_checker.py).  The corrected sweep and imu_point are read through srl_debug_undistorted_download and must be equal bytewise,
for both point_time_enable branches and the three motion-compensation modes; the IMU interval of every point must be the host walk's."""
import numpy as np
import pytest

import livox_cases as lc
import livox_checker as lk
import sr_livo_amd as srl
from sr_livo_amd import capi, synth

pytestmark = pytest.mark.gpu

R_IL = synth.quat_to_rot(synth.quat_from_rotvec([0.02, 0.01, -0.04]))
T_IL = np.array([0.05, 0.02, -0.03])
STAMP = 200.0
MODES = (capi.MC_IMU, capi.MC_CONSTANT_VELOCITY, capi.MC_NONE)


def imu_track(stamps, seed=3):
    rng = np.random.default_rng(seed)
    st = np.zeros((len(stamps), 17))
    q = synth.quat_from_rotvec([0.1, -0.05, 0.3]); p = np.array([1.0, 2.0, 0.3]); v = np.array([1.5, -0.4, 0.1])
    for k in range(len(stamps)):
        st[k, 0] = stamps[k]
        st[k, 1:4] = rng.normal(0, 0.5, 3); st[k, 4:7] = rng.normal(0, 0.3, 3)
        st[k, 7:10] = p; st[k, 10:14] = q; st[k, 14:17] = v
        q = synth.quat_mul(q, synth.quat_from_rotvec(st[k, 4:7] * 0.01)); p = p + v * 0.01; v = v + st[k, 1:4] * 0.01
    return st


@pytest.fixture(scope="module")
def ctx():
    k = srl.Context(0)
    yield k
    k.close()


def fresh_cut(ctx, n=2500, seed=61, late=False):
    """one message (two with `late`: the second starts before the first ends, so the cut is NOT sorted by time) decoded into an empty queue
    and cut whole -> the checker's records of the resident cut.  Microsecond offsets: the message spans [STAMP, STAMP + 0.1) s."""
    opts = srl.livox_opts(n_scans=lc.N_SCANS, time_unit=2, blind=0.5, point_filter_num=1)
    ctx.livox_decode(lc.make_message(2, 1), 1.0, opts)
    ctx.points_clear()
    q = lk.PointQueue()
    feeds = [(lc.make_message(n, seed, offset_step=100000 // n), STAMP)]
    if late:
        feeds.append((lc.make_message(n // 2, seed + 1, offset_step=100000 // n), STAMP + 0.03))
    for msg, stamp in feeds:
        ctx.livox_decode(msg, stamp, opts)
        q.push(lk.decode(msg, stamp, lc.N_SCANS, lk.time_unit_scale(2), 0.5, 1)["records"])
    count, _ = ctx.points_cut(1e9)
    rec = q.cut(1e9)
    assert count == len(rec) > 0
    return rec


def compare(ctx, rec, tb, te, enable, states, mode, expect_fallback=False):
    """the device's undistortion of the cut == srl_frame_undistort on the checker's rewritten arrays, bytewise"""
    before = ctx.points_fallbacks()
    n = ctx.frame_undistort_cut(tb, te, enable, states, mode, R_IL, T_IL)
    keep, rel, alpha = lk.rewrite_times(rec[:, 4], tb, te, enable)
    assert n == len(keep)
    got = ctx.undistorted_download()
    ts, grel, galpha = ctx.frame_point_times(np.arange(n, dtype=np.int32))
    assert ts.tobytes() == rec[keep, 4].tobytes() and grel.tobytes() == rel.tobytes() and galpha.tobytes() == alpha.tobytes()
    assert got["uncorrected"].tobytes() == np.ascontiguousarray(rec[keep, 0:3]).tobytes()
    assert ctx.points_fallbacks() - before == (1 if expect_fallback else 0)
    walk = lk.interval_walk(rel, states[:, 0], tb)
    if mode == capi.MC_IMU:
        assert np.array_equal(got["interval"], walk)
        if not expect_fallback:
            assert lk.preconditions_hold(rel, states[:, 0]) and np.array_equal(lk.interval_rule(rel, states[:, 0], tb), walk)
    # the yardstick (it replaces the undistorted sweep in HBM: the cut stays, so the next compare() starts from the same cut)
    imu, raw = ctx.frame_undistort(rec[keep, 0:3], rel, states, tb, mode, R_IL, T_IL)
    assert got["imu"].tobytes() == imu.tobytes() and got["raw"].tobytes() == raw.tobytes()
    with pytest.raises(srl.SrlError) as e:                                   # the times of a sweep the HOST handed over are not resident
        ctx.frame_point_times(np.zeros(1, np.int32))
    assert e.value.status == capi.SRL_ERR_NO_SWEEP
    return walk, alpha


@pytest.mark.parametrize("enable", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_both_time_branches_and_all_modes(ctx, enable, mode):
    rec = fresh_cut(ctx)
    tb, te = STAMP + 0.01, STAMP + 0.08                                      # points in front of time_begin and behind time_end
    states = imu_track(tb + 0.007 * np.arange(11))
    walk, alpha = compare(ctx, rec, tb, te, enable, states, mode)
    if enable:
        assert (alpha == 1.0 - 1e-5).sum() > 100 and (alpha < 0).sum() > 100     # the clamp, and no clamp below
    else:
        assert 0 < len(alpha) < len(rec) and alpha.min() >= 0 and alpha.max() <= 1
    if mode == capi.MC_IMU and not enable:
        assert walk.min() >= 0 and len(set(walk)) == 10                      # every interval is used
    if mode == capi.MC_IMU and enable:
        assert (walk == -1).all()                                            # the first point lies before the first interval: everything -1


def test_imu_interval_edges(ctx):
    rec = fresh_cut(ctx, n=700, seed=62)
    tb, te = STAMP, STAMP + 0.1
    keep, rel, _ = lk.rewrite_times(rec[:, 4], tb, te, True)
    tp = tb + rel / 1000.0                                                   # the time the walk compares
    # stamps placed so that points sit on the +- 1e-6 boundaries of the interval tests
    on_edges = np.array([tp[0] - 1e-6, tp[100] + 1e-6, tp[200] - 1e-6, tp[300], tp[400] + 1e-6, tp[400] + 1e-6, tp[500] - 1e-6, tp[-1] + 1e-6])
    assert np.all(np.diff(on_edges) >= 0)
    walk, _ = compare(ctx, rec, tb, te, True, imu_track(on_edges), capi.MC_IMU)
    assert walk.min() >= -1 and len(set(walk)) >= 5
    # a point beyond the last interval: it and everything behind it -1, the points in front of it keep theirs
    walk, _ = compare(ctx, rec, tb, te, True, imu_track(np.array([tp[0] - 1e-3, tp[300], tp[600] - 1e-6])), capi.MC_IMU)
    assert walk[0] == 0 and walk[-1] == -1 and 590 < int(np.argmax(walk < 0)) < 612
    # a point before the first interval: everything -1
    walk, _ = compare(ctx, rec, tb, te, True, imu_track(np.array([tp[5], tp[300], tp[-1] + 1.0])), capi.MC_IMU)
    assert (walk == -1).all()
    # one state pair only; and a single state (no interval at all)
    walk, _ = compare(ctx, rec, tb, te, True, imu_track(np.array([tp[0] - 1e-3, tp[-1] + 1e-3])), capi.MC_IMU)
    assert (walk == 0).all()
    walk, _ = compare(ctx, rec, tb, te, True, imu_track(np.array([tp[300]])), capi.MC_IMU)
    assert (walk == -1).all()
    # zero-length intervals
    walk, _ = compare(ctx, rec, tb, te, True, imu_track(np.array([tp[0] - 1e-3, tp[300], tp[300], tp[300], tp[-1] + 1e-3])), capi.MC_IMU)
    assert set(walk) >= {0, 3}


def test_the_fallback_for_a_non_monotone_cut_and_unordered_stamps(ctx):
    rec = fresh_cut(ctx, n=1200, seed=63, late=True)
    assert np.any(np.diff(rec[:, 4]) < 0)
    tb, te = STAMP, STAMP + 0.13
    states = imu_track(tb - 1e-3 + 0.0135 * np.arange(11))
    before = ctx.points_fallbacks()
    walk, _ = compare(ctx, rec, tb, te, True, states, capi.MC_IMU, expect_fallback=True)
    assert ctx.points_fallbacks() == before + 1
    assert 0 < int((walk >= 0).sum()) < len(walk)                            # the walk stops where the times go back
    # the other modes do not look at intervals: no fallback
    compare(ctx, rec, tb, te, False, states, capi.MC_CONSTANT_VELOCITY)
    assert ctx.points_fallbacks() == before + 1
    # state stamps that go back (checked on the host): the fallback again, on a monotone cut
    rec = fresh_cut(ctx, n=700, seed=64)
    bad = states.copy()
    bad[[4, 5], 0] = bad[[5, 4], 0]
    compare(ctx, rec, tb, tb + 0.1, True, bad, capi.MC_IMU, expect_fallback=True)
    assert ctx.points_fallbacks() == before + 2


def test_the_calls_behind_it_work_unchanged(ctx):
    """srl_frame_subsample keys on the uncorrected point; subsample and take give what they give behind srl_frame_undistort"""
    rec = fresh_cut(ctx, n=2500, seed=65)
    tb, te = STAMP, STAMP + 0.1
    states = imu_track(tb - 1e-3 + 0.0102 * np.arange(11))
    n = ctx.frame_undistort_cut(tb, te, True, states, capi.MC_IMU, R_IL, T_IL)
    order = np.random.default_rng(9).permutation(n).astype(np.int32)
    m = ctx.frame_subsample(order, 0.5)
    got = ctx.frame_take_subsampled(None, m=m, want_index=True, want_raw=True, want_imu=True)
    ts, rel, alpha = ctx.frame_point_times(got["index"])
    keep, wrel, walpha = lk.rewrite_times(rec[:, 4], tb, te, True)
    assert rel.tobytes() == wrel[got["index"]].tobytes() and alpha.tobytes() == walpha[got["index"]].tobytes()
    ctx.frame_undistort(rec[:, 0:3], wrel, states, tb, capi.MC_IMU, R_IL, T_IL)
    assert ctx.frame_subsample(order, 0.5) == m
    want = ctx.frame_take_subsampled(None, m=m, want_index=True, want_raw=True, want_imu=True)
    assert 100 < m < n and all(got[k].tobytes() == want[k].tobytes() for k in ("index", "raw", "imu"))


def test_an_empty_cut_and_refusals(ctx):
    fresh_cut(ctx, n=50, seed=66)
    count, front = ctx.points_cut(5.0)                                       # the queue is empty: an empty cut
    assert count == 0 and np.isnan(front)
    states = imu_track(STAMP + 0.01 * np.arange(3))
    assert ctx.frame_undistort_cut(STAMP, STAMP + 0.1, True, states, capi.MC_IMU, R_IL, T_IL) == 0
    assert ctx.frame_point_times(np.zeros(0, np.int32))[0].size == 0
    with pytest.raises(srl.SrlError) as e:
        ctx.frame_point_times(np.zeros(1, np.int32))
    assert e.value.status == capi.SRL_ERR_BAD_ARG
    with pytest.raises(srl.SrlError) as e:
        ctx.frame_undistort_cut(STAMP, STAMP + 0.1, True, states, 7, R_IL, T_IL)
    assert e.value.status == capi.SRL_ERR_BAD_ARG
    with pytest.raises(srl.SrlError) as e:
        ctx.frame_undistort_cut(float("nan"), STAMP + 0.1, True, states, capi.MC_IMU, R_IL, T_IL)
    assert e.value.status == capi.SRL_ERR_BAD_ARG
