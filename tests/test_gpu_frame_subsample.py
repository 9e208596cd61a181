"""buildFrame's subSampleFrame on the device (srl_frame_subsample + srl_frame_take_subsampled, lioOptimization.cpp:838-846 ->
utility.cpp:167-186) against the host's subSampleFrame (srl.grid_sampling: a real std::tr1::unordered_map) applied the way buildFrame
applies it:

    expected = order[grid_sampling(uncorrected[order], size)][perm2]

order = the first shuffle, perm2 = the second one over the kept voxels (random NumPy permutations: the ABI does not care where they
come from).  Index list, corrected raw points and imu_point must be equal bit for bit; so must everything a frame chain computes
behind it, and the host mirror's replays with the switch on and off."""
import os

import numpy as np
import pytest

import sr_livo_amd as srl
from sr_livo_amd import capi, synth

pytestmark = pytest.mark.gpu

INT_MAX = 2**31 - 1
BAD_ARG, NO_SWEEP = -3, -6
R_IL = synth.quat_to_rot(synth.quat_from_rotvec([0.02, 0.01, -0.04]))
T_IL = np.array([0.05, 0.02, -0.03])


def imu_track(rng, S=11, t0=200.0, dt=0.01):
    st = np.zeros((S, 17))
    q = synth.quat_from_rotvec([0.1, -0.05, 0.3]); p = np.array([1.0, 2.0, 0.3]); v = np.array([1.5, -0.4, 0.1])
    for k in range(S):
        st[k, 0] = t0 + k * dt
        st[k, 1:4] = rng.normal(0, 0.5, 3); st[k, 4:7] = rng.normal(0, 0.3, 3)
        st[k, 7:10] = p; st[k, 10:14] = q; st[k, 14:17] = v
        q = synth.quat_mul(q, synth.quat_from_rotvec(st[k, 4:7] * dt)); p = p + v * dt; v = v + st[k, 1:4] * dt
    return st


def room(rng, n):
    """a Livox-like sweep of a box room 4-30 m away (sensor frame)"""
    d = rng.normal(size=(n, 3)); d[:, 2] *= 0.3
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * rng.uniform(4.0, 30.0, (n, 1))


def times(rng, n):
    return np.sort(rng.uniform(0.0, 100.0, n))


def expected(raw, order, size, perm2):
    kept = order[srl.grid_sampling(raw[order], size)]
    return kept if perm2 is None else kept[perm2]


def undistort(ctx, raw, rng, mode, st=None):
    st = imu_track(rng) if st is None else st
    return ctx.frame_undistort(raw, times(rng, len(raw)), st, 200.0, mode, R_IL, T_IL)


def check_frame(ctx, raw, imu, corr, order, size, perm2, used=None):
    want = expected(raw, order, size, perm2)
    m = ctx.frame_subsample(order, size)
    assert m == len(want)
    if used is not None:
        assert ctx.frame_order_used() == used
    got = ctx.frame_take_subsampled(perm2, m=m, want_index=True, want_raw=True, want_imu=True)
    assert np.array_equal(got["index"], want)
    assert np.array_equal(got["raw"], corr[want]) and np.array_equal(got["imu"], imu[want])
    assert ctx.frame_size() == m
    return want


@pytest.fixture(scope="module")
def ctx():
    c = srl.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("n", [1, 2, 1_000, 24_000, 65_536, 131_073, 262_144])
@pytest.mark.parametrize("mode", [capi.MC_CONSTANT_VELOCITY, capi.MC_IMU, capi.MC_NONE])
def test_subsample_equals_the_host_bit_for_bit(ctx, n, mode):
    rng = np.random.default_rng(n * 7 + mode)
    raw = room(rng, n)
    imu, corr = undistort(ctx, raw, rng, mode)
    for size in (0.1, 0.2, 1.5):
        order = rng.permutation(n).astype(np.int32)
        want = expected(raw, order, size, None)
        check_frame(ctx, raw, imu, corr, order, size, rng.permutation(len(want)), used=1 if n <= 1 << 20 else 2)
    # perm = NULL: the container's order
    check_frame(ctx, raw, imu, corr, order, 0.2, None)


def test_edge_cases(ctx):
    rng = np.random.default_rng(3)
    mode = capi.MC_CONSTANT_VELOCITY
    cases = []
    n = 5_000
    cases.append((rng.uniform(0.01, 0.99, (n, 3)), 1.0, 1))                              # every point in one voxel
    keys = np.unique(rng.integers(-3000, 3000, (n, 3)), axis=0)
    cases.append((keys + np.where(keys >= 0, 0.5, -0.5), 1.0, len(keys)))                # every point in its own voxel
    cases.append((rng.uniform(-0.999, 0.999, (n, 3)) * 0.2, 0.2, 1))                     # voxel 0 spans (-size, size): the seam at 0
    cases.append((rng.uniform(-5, 5, (n, 3)), 0.5, None))                                # negative coordinates
    faces = rng.integers(-40, 40, (n, 3)) * 0.25                                         # exact voxel faces (p / size an integer)
    cases.append((faces, 0.25, None))
    cases.append((rng.uniform(-9000, 9000, (n, 3)), 0.1, None))                          # past +-3276.7 m at 0.1 m: the short cast wraps
    dup = room(rng, 2_000)
    cases.append((np.concatenate([dup, dup, dup[:500]]), 0.1, None))                     # duplicate points
    for raw, size, m in cases:
        imu, corr = undistort(ctx, raw, rng, mode)
        order = rng.permutation(len(raw)).astype(np.int32)
        want = expected(raw, order, size, None)
        if m is not None:
            assert len(want) == m
        check_frame(ctx, raw, imu, corr, order, size, rng.permutation(len(want)))
    # the wrap case really reaches past the short range
    big = cases[5][0]
    assert np.any(np.abs(big) / 0.1 > 32767)
    # n = 0
    z = np.zeros((0, 3))
    ctx.frame_undistort(z, np.zeros(0), imu_track(rng), 200.0, mode, R_IL, T_IL)
    assert ctx.frame_subsample(np.zeros(0, np.int32), 0.1) == 0
    got = ctx.frame_take_subsampled(np.zeros(0, np.int32), want_raw=True, want_imu=True)
    assert len(got["index"]) == 0 and ctx.frame_size() == 0


def points_of_keys(keys):
    keys = np.asarray(keys, dtype=np.int64)
    return keys.astype(np.float64) + np.where(keys >= 0, 0.5, -0.5)


def test_overfull_bucket_and_host_replay_fall_back(ctx):
    rng = np.random.default_rng(11)
    mode = capi.MC_NONE
    # 100 voxels -> 199 buckets; x = 199 k: every voxel in bucket 0, more than the device ranks in place -> host replay behind it (3)
    xs = rng.choice(np.arange(-160, 160), size=100, replace=False) * 199
    keys = np.column_stack([xs, np.zeros(100, int), np.zeros(100, int)])
    raw = np.repeat(points_of_keys(keys), 7, axis=0)
    imu, corr = undistort(ctx, raw, rng, mode)
    order = rng.permutation(len(raw)).astype(np.int32)
    want = check_frame(ctx, raw, imu, corr, order, 1.0, rng.permutation(100), used=3)
    assert len(want) == 100
    # the host replay on request (the keypoint selection's switch), and an ordinary frame after it is ordered on the device again
    ctx.set_frame_order_mode(1)
    try:
        check_frame(ctx, raw, imu, corr, order, 1.0, rng.permutation(100), used=2)
    finally:
        ctx.set_frame_order_mode(0)
    raw = room(rng, 4_000)
    imu, corr = undistort(ctx, raw, rng, mode)
    order = rng.permutation(len(raw)).astype(np.int32)
    check_frame(ctx, raw, imu, corr, order, 0.2, rng.permutation(len(expected(raw, order, 0.2, None))), used=1)


def test_frame_beyond_one_million_points():
    rng = np.random.default_rng(12)
    n = (1 << 20) + 3
    raw = room(rng, n)
    c = srl.Context(0)
    try:
        imu, corr = undistort(c, raw, rng, capi.MC_CONSTANT_VELOCITY)
        order = rng.permutation(n).astype(np.int32)
        want = expected(raw, order, 0.1, None)
        check_frame(c, raw, imu, corr, order, 0.1, rng.permutation(len(want)), used=2)
    finally:
        c.close()


def status_of(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except srl.SrlError as e:
        return e.status
    return 0


def test_rejections_leave_the_context_usable():
    rng = np.random.default_rng(13)
    mode = capi.MC_CONSTANT_VELOCITY
    c = srl.Context(0)
    try:
        assert status_of(c.frame_subsample, np.arange(10, dtype=np.int32), 0.1) == NO_SWEEP       # no undistorted sweep
        n = 3_000
        raw = room(rng, n)

        def good():
            imu, corr = undistort(c, raw, rng, mode)
            order = rng.permutation(n).astype(np.int32)
            check_frame(c, raw, imu, corr, order, 0.1, rng.permutation(len(expected(raw, order, 0.1, None))))

        good()
        undistort(c, raw, rng, mode)
        assert status_of(c.frame_take_subsampled, None, m=0) == NO_SWEEP                           # a take without a sub-sample
        good()
        bad_orders = []
        o = rng.permutation(n).astype(np.int32); o[17] = o[1234]; bad_orders.append(o)             # a duplicate
        o = rng.permutation(n).astype(np.int32); o[5] = n; bad_orders.append(o)                    # out of range
        o = rng.permutation(n).astype(np.int32); o[9] = -1; bad_orders.append(o)                   # negative
        bad_orders.append(rng.permutation(n - 1).astype(np.int32))                                 # wrong n
        bad_orders.append(rng.permutation(n + 1).astype(np.int32))
        for o in bad_orders:
            undistort(c, raw, rng, mode)
            assert status_of(c.frame_subsample, o, 0.1) == BAD_ARG
            assert status_of(c.frame_take_subsampled, None, m=0) == NO_SWEEP                       # no sub-sample is left behind
            good()
        for size in (0.0, -1.0, float("nan")):
            assert status_of(c.frame_subsample, rng.permutation(n).astype(np.int32), size) == BAD_ARG
        good()
        # bad second permutations: the sub-sample stays and can be taken again
        imu, corr = undistort(c, raw, rng, mode)
        order = rng.permutation(n).astype(np.int32)
        m = c.frame_subsample(order, 0.1)
        p = rng.permutation(m).astype(np.int32)
        bad_perms = [p[:-1], np.concatenate([p, [0]]), np.where(np.arange(m) == 3, p[4], p), np.where(np.arange(m) == 2, m, p),
                     np.where(np.arange(m) == 2, -5, p)]
        for bp in bad_perms:
            assert status_of(c.frame_take_subsampled, np.asarray(bp, np.int32)) == BAD_ARG
        want = expected(raw, order, 0.1, p)
        got = c.frame_take_subsampled(p, want_raw=True, want_imu=True)
        assert np.array_equal(got["index"], want) and np.array_equal(got["raw"], corr[want]) and np.array_equal(got["imu"], imu[want])
        good()
    finally:
        c.close()


def solve_passes(ctx, q, t, t_last, opts, passes=5):
    """the passes of a solve on the resident keypoints: a damped Gauss-Newton step from every pass's normal equations to the next pose"""
    out = []
    q = np.array(q, float); t = np.array(t, float)
    for _ in range(passes):
        ne, _ = ctx.build_residuals(capi.make_frame(q, t, t_last), opts)
        H = np.array(ne.HtH).reshape(6, 6); g = np.array(ne.Hth)
        out.append((ne.num_residuals, H.copy(), g.copy(), q.copy(), t.copy()))
        dx = -np.linalg.solve(H + 1e3 * np.eye(6), g)
        dx = np.clip(dx, -0.02, 0.02)
        q = synth.quat_mul(q, synth.quat_from_rotvec(dx[:3]))
        t = t + dx[3:]
    ctx.solve_end()
    return out, q, t


@pytest.mark.parametrize("pending", ["armed", "deferred_commit"])
def test_chained_frame_equals_the_host_index_list(pending):
    """keypoint selection, the passes of a solve and the commit on the sub-sampled frame == the same chain after srl_frame_take with the
    host-computed index list: normal equations, poses and map_download, bit for bit; once with an armed launch pending when the frame is
    built, once with the previous frame's deferred commit still in flight."""
    pts, L = synth.map_candidates(4401, 60_000)
    opts = srl.default_opts(max_num_residuals=INT_MAX)
    st = np.zeros((2, 17)); st[:, 0] = [200.0, 200.1]; st[:, 10] = 1.0          # identity motion: corrected == sensor-frame points
    a, b = srl.Context(0), srl.Context(0)
    try:
        for c in (a, b):
            c.map_insert(pts)
            c.set_armed_launch(2)
        rng = np.random.default_rng(4402)
        for f in range(3):
            sw = synth.make_sweep(4410 + f, 30_000, L)
            raw, q, t = sw["raw"], sw["q_pred"], sw["t_pred"]
            order = rng.permutation(len(raw)).astype(np.int32)
            rel_t = times(rng, len(raw))
            results = []
            for c, device in ((a, True), (b, False)):
                imu, corr = c.frame_undistort(raw, rel_t, st, 200.0, capi.MC_CONSTANT_VELOCITY)
                if pending == "armed" and f > 0:
                    c.build_residuals(capi.make_frame(q, t, sw["t_last"]), opts)      # a pass on the previous frame's keypoints: arms the next
                if device:
                    m = c.frame_subsample(order, 0.1)
                    perm = np.random.default_rng(f).permutation(m).astype(np.int32)
                    idx = c.frame_take_subsampled(perm)["index"]
                else:
                    idx = expected(raw, order, 0.1, np.random.default_rng(f).permutation(len(expected(raw, order, 0.1, None))))
                    c.frame_take(idx)
                kp = c.frame_select_keypoints(q, t, 0.25)
                passes, qf, tf = solve_passes(c, q, t, sw["t_last"], opts)
                c.frame_commit(qf, tf, voxel_size=1.0, want_world=False, want_added=(pending != "deferred_commit"))
                results.append((idx, kp, passes, qf, tf))
            (ia, ka, pa, qa, ta), (ib, kb, pb, qb, tb) = results
            assert np.array_equal(ia, ib) and np.array_equal(ka, kb) and len(ka) > 200
            for x, y in zip(pa, pb):
                assert x[0] == y[0] > 100
                for u, v in zip(x[1:], y[1:]):
                    assert np.array_equal(u, v)
            assert np.array_equal(qa, qb) and np.array_equal(ta, tb)
        ka_, ca_, xa_ = a.map_download(); kb_, cb_, xb_ = b.map_download()
        assert np.array_equal(ka_, kb_) and np.array_equal(ca_, cb_) and np.array_equal(xa_, xb_)
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------- the host mirror's replays, switch on and off

def replay(lio, streams):
    out = []
    for ms in streams:
        got = lio.run_measurement(ms["time_frame"], ms["imu_t"], ms["imu_acc"], ms["imu_gyr"], ms["pts_raw"], ms["pts_timestamp"],
                                  ms["time_sweep_begin"], ms["time_sweep_offset"])
        assert got["rc"] == 0
        f = lio.last_frame() if got["processed"] else None
        out.append((got, f, lio.eskf_get_state(), lio.eskf_get_cov(), lio.map_size()))
    return out, lio.ctx.map_download()


def both_switches(oo, icp_p, streams):
    """the same streams through two host mirrors, buildFrame's sub-sample on the device and on the host.  Two runs of one setting in one
    process already differ in the last bits of the filter state (the first differing measurement carries ~1e-15 in the gravity of the
    ESKF state, with the switch on or off alike), so the runs are held to each other at the tolerances of the replay tests and the counts,
    the processed flags and the final map's voxels exactly; the frame build itself is compared bit for bit above."""
    runs = []
    for on in (True, False):
        lio = srl.Lio(0)
        try:
            lio.set_initial_flag(False)
            lio.set_odometry_options(icp=icp_p, **oo)
            lio.set_device_subsample(on)
            runs.append(replay(lio, streams))
        finally:
            lio.set_initial_flag(False)
            lio.close()
    (ra, ma), (rb, mb) = runs
    assert len(ra) == len(rb)
    for (ga, fa, sa, ca, na), (gb, fb, sb, cb, nb) in zip(ra, rb):
        for k in ga:
            if k == "state":
                assert rel(ga[k], gb[k]) < 1e-9
            else:
                assert ga[k] == gb[k], k
        assert (fa is None) == (fb is None)
        if fa is not None:
            assert rel(fa["raw_point"], fb["raw_point"]) < 1e-11 and rel(fa["imu_point"], fb["imu_point"]) < 1e-11
            assert rel(fa["point"], fb["point"]) < 1e-9
        assert rel(sa, sb) < 1e-9 and rel(ca, cb) < 1e-8 and na == nb
    assert np.array_equal(ma[0], mb[0]) and np.array_equal(ma[1], mb[1])
    return ra, ma


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)) if a.size else 0.0


@pytest.fixture(scope="module")
def gref():
    here = os.path.dirname(os.path.abspath(__file__))
    return {k: v for p in ("golden_ref_tu.npz", "golden_ref_tu_part2.npz") for k, v in np.load(os.path.join(here, "golden", p), allow_pickle=False).items()}


@pytest.mark.parametrize("mc", [capi.MC_CONSTANT_VELOCITY, capi.MC_IMU])
def test_node_golden_replay_with_the_switch_on_and_off(gref, mc):
    from replay_reference import REPLAY_OO, REPLAY_SEQ, replay_inputs
    _, parts, _ = replay_inputs()
    oo = dict(REPLAY_OO, motion_compensation=mc)
    icp_p = srl.default_opts(max_num_residuals=REPLAY_SEQ["max_num_residuals"])
    runs, (k, c, x) = both_switches(oo, icp_p, parts)
    pre = f"run{mc}"
    row = 0
    for i, (got, f, eskf_state, eskf_cov, map_points) in enumerate(runs):
        if not got["processed"]:
            continue
        assert i == int(gref[f"{pre}_measurement"][row]) and got["success"]
        assert got["frame_points"] == int(gref[f"{pre}_frame_points"][row])
        assert rel(got["state"], gref[f"{pre}_state"][row]) < 1e-9
        assert rel(eskf_state, gref[f"{pre}_eskf_state"][row]) < 1e-9
        assert rel(eskf_cov, gref[f"{pre}_eskf_cov"][row]) < 1e-8
        assert map_points == int(gref[f"{pre}_map_points"][row])
        assert rel(f["raw_point"].sum(0), gref[f"{pre}_raw_sum"][row]) < 1e-11 and rel(f["point"].sum(0), gref[f"{pre}_point_sum"][row]) < 1e-9
        row += 1
    assert row == len(gref[f"{pre}_measurement"]) == 9
    order = np.lexsort((k[:, 2], k[:, 1], k[:, 0]))
    assert np.array_equal(k[order], gref[f"{pre}_map_keys"]) and np.array_equal(c[order], gref[f"{pre}_map_counts"])
    assert np.array_equal(x[order], gref[f"{pre}_map_xyz"])


@pytest.mark.parametrize("mc", [capi.MC_CONSTANT_VELOCITY, capi.MC_IMU])
def test_reference_loop_replay_with_the_switch_on_and_off(oracle_lib, oracle_backend, mc):
    from replay_reference import OracleReplay
    pts, L = synth.map_candidates(555, 60_000)
    meas, gt, _ = synth.make_sequence(31, 7, 24_000, L)
    oo = dict(init_voxel_size=0.2, init_sample_voxel_size=1.0, init_num_frames=6, num_for_initialization=10, voxel_size=0.2,
              sample_voxel_size=1.5, max_num_points_in_voxel=20, min_distance_points=0.1, motion_compensation=mc, initialization=0,
              point_time_enable=1, acc_cov=0.1, gyr_cov=0.1, b_acc_cov=1e-4, b_gyr_cov=1e-4)
    icp_p = srl.default_opts(max_num_residuals=600)
    runs, (kg, cg, _) = both_switches(oo, icp_p, meas)
    ref = OracleReplay(oracle_lib, oracle_backend, oo, oracle_lib.opts_from_product(icp_p))
    processed = 0
    for ms, (got, f, _, eskf_cov, _) in zip(meas, runs):
        want = ref.run_measurement(ms)
        assert got["processed"] == (want is not None)
        if want is None:
            continue
        processed += 1
        assert got["success"] and want["success"]
        assert got["frame_points"] == want["frame_points"] and got["keypoints"] == want["keypoints"]
        assert got["iters"] == want["iters"] and got["num_residuals"] == want["num_residuals"]
        assert got["points_added"] == want["points_added"]
        assert rel(got["state"], want["state"]) < 1e-9
        fo = ref.frames[-1]
        assert rel(f["raw_point"], fo["raw"]) < 1e-11 and rel(f["imu_point"], fo["imu_point"]) < 1e-11
        assert rel(f["point"], fo["point"]) < 1e-9
        assert rel(eskf_cov, ref.e.get_cov()) < 1e-8
    assert processed == ref.index_frame - 1 and processed >= 9
    ko, co, _ = ref.m.export()
    assert np.array_equal(kg, ko) and np.array_equal(cg, co)
