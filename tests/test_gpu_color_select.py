"""Selecting the colour map's points for projection on the device (srl_color_map_select: rgbMapTracker::selectPointsForProjection,
rgbMapTracker.cpp:45-152) against the sequential restatement of tests/select_checker.py -- which tests/test_select_checker_reference.py
pins to the reference's own translation units -- and against the records of tests/golden/golden_color_select.npz.

Every comparison is bit for bit, through the C-ABI: the records (index, pool position, registered index, position, u, v) and the totals
of every call.  The golden file holds the records of every call but those at minimum_dis 0.4, of which it holds the number and a CRC-32
(the file has to stay small): a mismatch there is reported by golden_check as "records (CRC)" without a position, and the comparison
with the checker in front of it in the same test names the records that differ."""
import ctypes as C
import os

import numpy as np
import pytest

import color_checker as cc
import render_checker as rk
import select_checker as sk
import sr_livo_amd as srl
from sr_livo_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRL_ERR_BAD_ARG, SRL_ERR_NO_MAP = -3, -5               # include/srlivo_hip.h: srl_status


def _cam(c):
    return capi.ColorCamera((C.c_double * 4)(*c.q), (C.c_double * 3)(*c.t), c.fx, c.fy, c.cx, c.cy, c.fov_margin)


def _ctx(opt=rk.OPT):
    ctx = srl.Context(0)
    ctx.color_map_create(capi.default_color_opts(size_voxel_map=opt[0], max_num_points_in_voxel=opt[1], min_distance_points=opt[2], add_point_step=opt[3]))
    return ctx


def _scene_ctx(batches=3):
    """a device map holding the scene; the visited list of every insertion as the device returned it"""
    ctx = _ctx()
    visited = [ctx.color_map_insert(cc.scene_batch(j), rk.BATCH_TIMES[j], 0.0)[2] for j in range(3)]
    if batches == 4:
        visited.append(ctx.color_map_insert(sk.extra_batch(), sk.EXTRA_BATCH_TIME, 0.0)[2])
    return ctx, visited


def _opts(md=10.0, skip=1, use_all=False, dmin=sk.MINIMUM_DEPTH, dmax=sk.MAXIMUM_DEPTH):
    return capi.default_color_select_opts(minimum_dis=md, skip_step=skip, use_all_points=1 if use_all else 0, minimum_depth=dmin, maximum_depth=dmax)


def _same(got, want, what=""):
    rec, tot = got
    w_rec, w_tot = want[0], want[1]
    assert tot.as_tuple() == sk.totals_tuple(w_tot), (what, tot.as_tuple(), w_tot)
    assert rec.dtype == w_rec.dtype == capi.COLOR_SELECTED_DTYPE == sk.SELECTED_DTYPE
    assert rec.tobytes() == w_rec.tobytes(), (what, np.flatnonzero(rec != w_rec)[:8] if len(rec) == len(w_rec) else (len(rec), len(w_rec)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_color_select.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def scene():
    ctx, visited = _scene_ctx()
    yield ctx, visited
    ctx.close()


# ------------------------------------------------------------------------------------------------ 1. list mode over the scene's poses
def test_list_mode_preconditions_from_the_checker_alone():
    """cells with more than one candidate: every (10, 1) call has at least 100.  At minimum_dis 40 the smaller image has about
    375 x 500 / 40^2 = 117 cells in all, so no call of the (40, 3) set can be asked for 100: the set has them over its calls, and every
    call of it has them in at least a third of the cells an image of its size has (39 and 64), so that no one call carries the others"""
    several = {0: [], 2: []}
    for (k, s, m), (_, _, cells) in zip(sk.SEQUENCE, sk.sequence_results()):
        if s in several:
            _, rows, cols, _ = sk.scene_camera(k, sk.MARGINS[m])
            several[s].append((sk.rule_census(cells)[0], rows * cols // (40 * 40) // 3))
    print("cells with several candidates (and the floor of a (40, 3) call):", several)
    assert min(n for n, _ in several[0]) >= 100
    assert sum(n for n, _ in several[2]) >= 100 and all(n >= floor for n, floor in several[2])


def test_list_mode_equals_the_restatement_and_the_golden(scene, golden):
    ctx, visited = scene
    _, chk_visited = sk.scene_map()
    for a, b in zip(visited, chk_visited):
        assert np.array_equal(a, b)
    assert np.array_equal(golden["sequence"], np.array(sk.SEQUENCE))
    for n, ((k, s, m), want) in enumerate(zip(sk.SEQUENCE, sk.sequence_results())):
        cam, rows, cols, lists = sk.scene_camera(k, sk.MARGINS[m])
        voxels = np.concatenate([visited[j] for j in lists])
        md, skip = sk.PARAMETER_SETS[s]
        got = ctx.color_map_select(_cam(cam), rows, cols, voxels, _opts(md, skip))
        _same(got, want, (k, s, m))
        assert sk.golden_check(golden, "s%d" % n, got[0], got[1].as_tuple()) is None, (k, s, m)
        assert got[1].selected > 50 and (np.diff(got[0]["index"]) > 0).all() and (got[0]["index"] % skip == 0).all()


# ------------------------------------------------------------------------------------------------ 2. all-points mode
def test_all_points_by_the_flag_and_by_an_empty_list_before_and_after_a_further_insertion(golden):
    ctx, visited = _scene_ctx()
    try:
        for batches in (3, 4):
            if batches == 4:
                # list mode first, so that the tails exist and have to follow the growth
                cam, rows, cols, _ = sk.scene_camera(0, 0.005)
                _same(ctx.color_map_select(_cam(cam), rows, cols, visited[2], _opts()), sk.select_sequential(sk.scene_map(3)[0], cam, rows, cols, visited[2]))
                more = ctx.color_map_insert(sk.extra_batch(), sk.EXTRA_BATCH_TIME, 0.0)[2]
                assert np.array_equal(more, sk.scene_map(4)[1][3])
                smap = sk.scene_map(4)[0]
                _same(ctx.color_map_select(_cam(cam), rows, cols, more, _opts(7.5, 2)), sk.select_sequential(smap, cam, rows, cols, more, 7.5, 2), "tails after growth")
            assert ctx.color_map_size()[2] == len(sk.scene_map(batches)[0].chk.registered)
            for n, ((k, margin), want) in enumerate(zip(sk.ALL_POINTS_CAMERAS, sk.all_points_results(batches))):
                cam, rows, cols, lists = sk.scene_camera(k, margin)
                by_flag = ctx.color_map_select(_cam(cam), rows, cols, visited[0], _opts(use_all=True))       # the list is ignored
                by_empty = ctx.color_map_select(_cam(cam), rows, cols, None, _opts(use_all=False))           # `&& size()` (:74)
                _same(by_flag, want, (batches, n))
                _same(by_empty, want, (batches, n))
                assert sk.golden_check(golden, "a%d_%d" % (batches, n), by_flag[0], by_flag[1].as_tuple()) is None
                assert (by_flag[0]["index"] == by_flag[0]["point_index"]).all() and by_flag[1].candidates == ctx.color_map_size()[2]
                reg = ctx.color_registered_download()
                assert np.array_equal(reg["batch_index"][by_flag[0]["index"]], by_flag[0]["pool"])            # pool = batch_index of the registered download
    finally:
        ctx.close()


def test_the_tails_follow_a_growth_of_the_voxel_array():
    """the tail array comes with the first list-mode selection (4 500 voxel records behind a 3 000-point batch) and grows by copy when an
    11 000-point batch makes the voxel array grow: the voxels the second batch left alone keep the tails swept before it"""
    first, second = cc.scene_batch(0)[:3000], cc.scene_batch(1)
    smap = sk.SelectMap(*rk.OPT)
    ctx = _ctx()
    try:
        cam, rows, cols, _ = sk.scene_camera(0, 0.005)
        v0 = ctx.color_map_insert(first, rk.BATCH_TIMES[0], 0.0)[2]
        smap.insert(first, rk.BATCH_TIMES[0], 0.0)
        assert ctx.color_map_size()[1] < 4096
        _same(ctx.color_map_select(_cam(cam), rows, cols, v0, _opts()), sk.select_sequential(smap, cam, rows, cols, v0), "before the growth")
        v1 = ctx.color_map_insert(second, rk.BATCH_TIMES[1], 0.0)[2]
        smap.insert(second, rk.BATCH_TIMES[1], 0.0)
        left_alone = set(map(tuple, v0)) - set(map(tuple, v1))
        both = np.concatenate([v0, v1])
        want = sk.select_sequential(smap, cam, rows, cols, both)
        held_by_old_tails = sum(1 for r in want[0] if tuple(both[r["index"]]) in left_alone)
        assert len(left_alone) > 100 and held_by_old_tails > 20, (len(left_alone), held_by_old_tails)
        _same(ctx.color_map_select(_cam(cam), rows, cols, both, _opts()), want, "after the growth")
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 3. the float-depth rule
def test_the_float_depth_rule_on_two_thin_shells(golden):
    smap, want = sk.shell_scene()
    several, below_not_nearest, tie_not_nearest = sk.rule_census(want[2])
    print("shells: cells with several candidates %d; holder set below the float minimum and not the nearest %d; tie at the float minimum and "
          "holder not the nearest %d" % (several, below_not_nearest, tie_not_nearest))
    assert below_not_nearest >= 20 and tie_not_nearest >= 20                # from the checker alone, before the device is asked
    ctx = _ctx(sk.SHELL_OPT)
    try:
        ctx.color_map_insert(sk.shell_points(), 1.0, 0.0)
        assert ctx.color_map_size() == smap.chk.sizes()
        got = ctx.color_map_select(_cam(sk.shell_camera()), sk.SHELL_ROWS, sk.SHELL_COLS, None, _opts(10.0, 1, True))
        _same(got, want, "shells")
        assert sk.golden_check(golden, "shell", got[0], got[1].as_tuple()) is None
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 4. an unknown key in the list
def test_an_unknown_key_takes_no_index(scene):
    ctx, visited = scene
    smap, _ = sk.scene_map()
    cam, rows, cols, _ = sk.scene_camera(0, 0.005)
    unknown = np.array([[30000, 30000, 30000]], np.int32)
    assert tuple(unknown[0]) not in smap.chk.voxels
    base = visited[0][:601]
    mixed = np.concatenate([base[:301], unknown, base[301:]])               # 301 known entries in front: the parity of every later index changes
    want = sk.select_sequential(smap, cam, rows, cols, mixed, 10.0, 2)
    got = ctx.color_map_select(_cam(cam), rows, cols, mixed, _opts(10.0, 2))
    _same(got, want)
    assert got[1].unknown == 1 and got[1].candidates == 601
    # the indices are ranks among the known entries: the same selection as without the entry
    _same(ctx.color_map_select(_cam(cam), rows, cols, base, _opts(10.0, 2)), (want[0], dict(want[1], unknown=0)))
    assert (got[0]["index"] > 301).any() and (got[0]["index"] % 2 == 0).all()
    # a list of unknown keys alone is list mode with nothing in it
    rec, tot = ctx.color_map_select(_cam(cam), rows, cols, np.repeat(unknown, 3, 0), _opts())
    assert len(rec) == 0 and tot.as_tuple() == (0, 0, 0, 0, 0, 0, 0, 3)


# ------------------------------------------------------------------------------------------------ 5. depth limits
def test_depth_limits_cut_on_both_sides_and_a_depth_at_a_limit_is_kept(scene):
    ctx, visited = scene
    smap, _ = sk.scene_map()
    cam, rows, cols, lists = sk.scene_camera(0, 0.005)
    voxels = np.concatenate([visited[j] for j in lists])
    # the limits are the depths of two candidates of the call: those two are kept (neither > nor <), what lies beyond them is not
    accepted, _ = sk._visit(smap, cam, rows, cols, voxels, 10.0, 1, False, 0.0, 1e9)
    depths = np.sort(np.array([a[2] for a in accepted]))
    dmin, dmax = float(depths[len(depths) // 4]), float(depths[3 * len(depths) // 4])
    want = sk.select_sequential(smap, cam, rows, cols, voxels, 10.0, 1, False, dmin, dmax)
    assert want[1]["far"] > 0 and want[1]["near"] > 0
    at_limit = [c for cand in want[2].values() for c in cand if c[1] in (dmin, dmax)]
    assert {c[1] for c in at_limit} == {dmin, dmax}
    got = ctx.color_map_select(_cam(cam), rows, cols, voxels, _opts(10.0, 1, False, dmin, dmax))
    _same(got, want)
    # ... and one ulp inside the limits they are gone
    tighter = sk.select_sequential(smap, cam, rows, cols, voxels, 10.0, 1, False, float(np.nextafter(dmin, np.inf)), float(np.nextafter(dmax, -np.inf)))
    assert tighter[1]["far"] > want[1]["far"] and tighter[1]["near"] > want[1]["near"]
    _same(ctx.color_map_select(_cam(cam), rows, cols, voxels, _opts(10.0, 1, False, float(np.nextafter(dmin, np.inf)), float(np.nextafter(dmax, -np.inf)))), tighter)


# ------------------------------------------------------------------------------------------------ 6. nothing else moved
def test_a_selection_moves_nothing_else_and_two_runs_give_the_same_bytes():
    chk = cc.ColorChecker(*rk.OPT)
    ctx = _ctx()
    try:
        visited = []
        for j in range(3):
            visited.append(ctx.color_map_insert(cc.scene_batch(j), rk.BATCH_TIMES[j], 0.0)[2])
            chk.insert(cc.scene_batch(j), rk.BATCH_TIMES[j], 0.0)
        ctx.map_insert(cc.scene_batch(0))                                  # a LiDAR map beside the colour map
        assert ctx.map_size()[1] > 100
        rc = rk.RenderChecker(chk)
        cam_r, which, obs_time, voxels = rk.render_call(0, visited)
        ctx.color_image_upload(rk.scene_image(which))
        ctx.color_map_render(_cam(cam_r), voxels, obs_time)
        rc.render(cam_r, rk.scene_image(which), voxels, obs_time)

        def snapshot():
            lidar = ctx.map_download()
            return (b"".join(np.ascontiguousarray(a).tobytes() for a in ctx.color_map_download()), rk.state_bytes(ctx.color_map_download_rgb()),
                    rk.state_bytes(ctx.color_registered_rgb()), ctx.color_registered_download().tobytes(), b"".join(a.tobytes() for a in lidar),
                    ctx.color_map_size(), ctx.map_size())
        before = snapshot()
        cam, rows, cols, lists = sk.scene_camera(1, -0.4)
        runs = []
        for _ in range(2):
            a = ctx.color_map_select(_cam(cam), rows, cols, voxels, _opts(7.5, 2))
            b = ctx.color_map_select(_cam(cam), rows, cols, None, _opts(use_all=True))
            runs.append((a[0].tobytes(), a[1].as_tuple(), b[0].tobytes(), b[1].as_tuple()))
        assert runs[0] == runs[1] and len(runs[0][0]) > 0 and len(runs[0][2]) > 0
        assert snapshot() == before
        # a render after the selections equals the checker
        cam_r, which, obs_time, voxels = rk.render_call(1, visited)
        ctx.color_image_upload(rk.scene_image(which))
        got = ctx.color_map_render(_cam(cam_r), voxels, obs_time)
        want = rc.render(cam_r, rk.scene_image(which), voxels, obs_time)
        assert got.as_tuple() == tuple(want[name] for name in rk.TOTALS)
        assert rk.state_bytes(ctx.color_map_download_rgb()) == rk.state_bytes(rc.map_state())
    finally:
        ctx.close()


def test_a_second_context_gives_the_same_bytes(scene):
    ctx, visited = scene
    other, visited2 = _scene_ctx()
    try:
        cam, rows, cols, lists = sk.scene_camera(3, -0.4)
        voxels = np.concatenate([visited[j] for j in lists])
        for o in (_opts(0.4, 1), _opts(10.0, 1, True)):
            a, b = ctx.color_map_select(_cam(cam), rows, cols, voxels, o), other.color_map_select(_cam(cam), rows, cols, voxels, o)
            assert a[0].tobytes() == b[0].tobytes() and a[1].as_tuple() == b[1].as_tuple() and len(a[0]) > 0
    finally:
        other.close()


# ------------------------------------------------------------------------------------------------ 7. capacity
def test_capacity(scene):
    ctx, visited = scene
    cam, rows, cols, lists = sk.scene_camera(0, 0.005)
    voxels = np.ascontiguousarray(visited[0])
    o = _opts()
    lib = ctx.lib
    tot = capi.ColorSelectTotals()
    assert lib.srl_color_map_select(ctx.h, C.byref(_cam(cam)), rows, cols, capi._ptr(voxels), len(voxels), C.byref(o), None, 0, C.byref(tot)) == capi.SRL_OK
    n = tot.selected
    assert n > 100
    full = tot.as_tuple()
    out = np.full(n, 7, dtype=capi.COLOR_SELECTED_DTYPE)
    tot = capi.ColorSelectTotals()
    assert lib.srl_color_map_select(ctx.h, C.byref(_cam(cam)), rows, cols, capi._ptr(voxels), len(voxels), C.byref(o), capi._ptr(out), n - 1,
                                    C.byref(tot)) == SRL_ERR_BAD_ARG
    assert tot.as_tuple() == full and (out["index"] == 7).all()             # the totals filled, nothing copied
    assert lib.srl_color_map_select(ctx.h, C.byref(_cam(cam)), rows, cols, capi._ptr(voxels), len(voxels), C.byref(o), capi._ptr(out), n,
                                    C.byref(tot)) == capi.SRL_OK
    want = sk.select_sequential(sk.scene_map()[0], cam, rows, cols, voxels)
    assert out.tobytes() == want[0].tobytes() and tot.as_tuple() == full == sk.totals_tuple(want[1])
    assert lib.srl_color_map_select(ctx.h, C.byref(_cam(cam)), rows, cols, capi._ptr(voxels), len(voxels), C.byref(o), capi._ptr(out), n, None) == capi.SRL_OK


# ------------------------------------------------------------------------------------------------ 8. the mirror
def test_the_mirrors_methods_give_the_records_of_the_c_call():
    lio = srl.Lio(0)
    ctx = _ctx()
    try:
        o = rk.OPT
        lio.set_color_map_options(capi.default_color_opts(size_voxel_map=o[0], max_num_points_in_voxel=o[1], min_distance_points=o[2], add_point_step=o[3]))
        lio.set_color_times(time_last_process=0.0)
        cam, rows, cols, _ = sk.scene_camera(0, 0.005)
        for j in range(2):
            pts = cc.scene_batch(j)
            lio.add_points_to_map_at(pts, rk.BATCH_TIMES[j], to_rendering=(j == 1))      # false, then true: the list of both sweeps moves over
            ctx.color_map_insert(pts, rk.BATCH_TIMES[j], 0.0)
        voxels, _ = lio.color_visited(1)                                   # voxels_recent_visited
        assert len(voxels) > 1000
        a = lio.refresh_points_for_projection(_cam(cam), rows, cols)
        b = ctx.color_map_select(_cam(cam), rows, cols, voxels, _opts())
        assert a[0].tobytes() == b[0].tobytes() and a[1].as_tuple() == b[1].as_tuple() and len(a[0]) > 100
        a = lio.select_points_for_projection(_cam(cam), rows, cols, 7.5, 2, use_all_points=True)
        b = ctx.color_map_select(_cam(cam), rows, cols, voxels, _opts(7.5, 2, True))
        assert a[0].tobytes() == b[0].tobytes() and a[1].as_tuple() == b[1].as_tuple() and len(a[0]) > 100
        rec, tot = lio.refresh_points_for_projection(_cam(cam), 0, cols)    # a frame without an image size: nothing (rgbMapTracker.cpp:30)
        assert len(rec) == 0 and tot.as_tuple() == (0,) * 8
        assert np.array_equal(lio.color_visited(1)[0], voxels)              # the list is the caller's: not consumed
    finally:
        ctx.close(); lio.close()


def test_an_empty_map_and_a_map_of_one_point():
    ctx = srl.Context(0)
    try:
        cam, rows, cols, _ = sk.scene_camera(0, 0.005)
        one = np.zeros((1, 3), np.int32)
        o = _opts()
        assert ctx.lib.srl_color_map_select(ctx.h, C.byref(_cam(cam)), rows, cols, capi._ptr(one), 1, C.byref(o), None, 0, None) == SRL_ERR_NO_MAP
        ctx.color_map_create()
        # an empty map: every key is unknown; all points: nothing
        assert ctx.color_map_select(_cam(cam), rows, cols, one)[1].as_tuple() == (0, 0, 0, 0, 0, 0, 0, 1)
        assert ctx.color_map_select(_cam(cam), rows, cols, None)[1].as_tuple() == (0,) * 8
        ctx.color_map_insert(np.array([[0.05, 0.05, 0.05]]), 1.0, 0.0)
        rec, tot = ctx.color_map_select(_cam(rk.Camera((0.5, -0.5, 0.5, -0.5), (-3.0, 0.05, 0.05), 200.0, 200.0, cols / 2.0, rows / 2.0, 0.005)), rows, cols, one)
        assert tot.as_tuple() == (1, 1, 0, 0, 0, 0, 1, 0) and rec["pool"][0] == 0 and rec["point_index"][0] == 0 and rec["index"][0] == 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ refusals, armed launches
def test_refusals_leave_the_totals_zero():
    ctx = srl.Context(0)
    try:
        lib = ctx.lib
        cam, rows, cols, _ = sk.scene_camera(0, 0.005)
        one = np.zeros((1, 3), np.int32)

        def call(camera=None, r=rows, c=cols, voxels=one, n=1, o=None, capacity=0, with_cam=True, with_opts=True):
            tot = capi.ColorSelectTotals(7, 7, 7, 7, 7, 7, 7, 7)
            camera = _cam(cam) if camera is None else camera
            o = _opts() if o is None else o
            rc = lib.srl_color_map_select(ctx.h, C.byref(camera) if with_cam else None, r, c, capi._ptr(voxels), n, C.byref(o) if with_opts else None, None,
                                          capacity, C.byref(tot))
            assert rc == capi.SRL_OK or tot.as_tuple() == (0,) * 8
            return rc
        assert call() == SRL_ERR_NO_MAP
        ctx.color_map_create()
        ctx.color_map_insert(cc.scene_batch(0)[:500], 1.0, 0.0)
        assert call() == capi.SRL_OK
        assert call(with_cam=False) == SRL_ERR_BAD_ARG and call(with_opts=False) == SRL_ERR_BAD_ARG
        assert call(voxels=None, n=1) == SRL_ERR_BAD_ARG and call(n=-1) == SRL_ERR_BAD_ARG and call(capacity=-1) == SRL_ERR_BAD_ARG
        for kw in (dict(md=0.0), dict(md=-1.0), dict(md=float("nan")), dict(md=float("inf")), dict(md=65536.5), dict(skip=0), dict(skip=-2),
                   dict(dmin=float("nan")), dict(dmax=float("nan"))):
            assert call(o=_opts(**kw)) == SRL_ERR_BAD_ARG, kw
        assert call(o=_opts(md=65536.0)) == capi.SRL_OK
        assert call(r=1) == SRL_ERR_BAD_ARG and call(c=1) == SRL_ERR_BAD_ARG and call(r=8193, c=8192) == SRL_ERR_BAD_ARG
        assert call(r=8192, c=8192) == capi.SRL_OK and call(r=2, c=2) == capi.SRL_OK
        for field, value, want in (("fov_margin", 0.5, SRL_ERR_BAD_ARG), ("fov_margin", -4.001, SRL_ERR_BAD_ARG), ("fov_margin", float("nan"), SRL_ERR_BAD_ARG),
                                   ("fov_margin", -4.0, capi.SRL_OK), ("fov_margin", 0.0, capi.SRL_OK), ("fov_margin", 0.499, capi.SRL_OK),
                                   ("fx", float("inf"), SRL_ERR_BAD_ARG), ("cy", float("nan"), SRL_ERR_BAD_ARG)):
            bad = _cam(cam)
            setattr(bad, field, value)
            assert call(camera=bad) == want, (field, value)
        bad = _cam(cam)
        bad.t_world_camera[1] = float("nan")
        assert call(camera=bad) == SRL_ERR_BAD_ARG
        bad = _cam(cam)
        for k, q in enumerate((1e-160, 1e-160, 0.0, 0.0)):                 # finite, but inverse() divides by the squared norm: the matrix is not
            bad.q_world_camera[k] = q
        assert call(camera=bad) == SRL_ERR_BAD_ARG
        ctx.comm_set_host_callbacks(2, 0, lambda a: None, lambda v: [v, v])       # more than one rank
        assert call() == capi.SRL_ERR_UNSUPPORTED
        ctx.comm_set_host_callbacks(1, 0, None, None)
        assert call() == capi.SRL_OK
    finally:
        ctx.close()


class _EskfAdapter:
    def __init__(self, lio): self.lio = lio
    def set_noise(self, *a): self.lio.eskf_set_noise(*a)
    def scale_init_cov(self): self.lio.eskf_scale_init_cov()
    def init_imu(self, a, g): self.lio.eskf_init_imu(a, g)
    def predict(self, dt, a, g): self.lio.eskf_predict(dt, a, g)
    def get_state(self): return self.lio.eskf_get_state()
    def set_state(self, s): self.lio.eskf_set_state(s)


def test_a_selection_cancels_an_armed_launch_and_the_next_solve_is_unchanged():
    from sr_livo_amd import synth
    n_kp, map_pts, pattern, seed = synth.CONFIGS["C1"]
    cands, L = synth.map_candidates(seed, map_pts)
    sweep = synth.make_sweep(seed + 1000, n_kp, L, pattern=pattern)
    lio = srl.Lio(0)
    try:
        lio.add_points_to_map(cands)
        prior_state = synth.eskf_prior(_EskfAdapter(lio), sweep["q_pred"], sweep["t_pred"], sweep["vel"]).copy()
        prior_cov = lio.eskf_get_cov().copy()
        state0 = np.concatenate([sweep["q_pred"], sweep["t_pred"], sweep["vel"], np.zeros(6)])
        lio.resident_sweep(sweep["raw"])
        solve = lio.bound_solver(srl.default_opts(max_num_residuals=2**31 - 1), prior_state, prior_cov, state0, sweep["t_last"], 100, n_kp)
        lio.ctx.set_armed_launch(0)
        solve()
        ref = (solve.state.copy(), lio.eskf_get_state().copy(), lio.eskf_get_cov().copy())
        lio.ctx.color_map_create()
        pts = cc.scene_batch(0)
        visited = lio.ctx.color_map_insert(pts, 1.0, 0.0)[2]
        smap = sk.SelectMap(*rk.OPT); smap.insert(pts, 1.0, 0.0)
        cam, rows, cols, _ = sk.scene_camera(0, 0.005)
        lio.ctx.set_armed_launch(2)                                        # a launch armed behind every eligible pass
        solve()
        s0 = lio.ctx.arm_stats()
        assert s0["armed"] > 0
        _same(lio.ctx.color_map_select(_cam(cam), rows, cols, visited, _opts()), sk.select_sequential(smap, cam, rows, cols, visited))
        s1 = lio.ctx.arm_stats()
        assert s1["cancelled"] + s1["expired"] > s0["cancelled"] + s0["expired"] and s1["fired"] == s0["fired"]      # (left by itself if the host was slow)
        solve()
        assert np.array_equal(solve.state, ref[0]) and np.array_equal(lio.eskf_get_state(), ref[1]) and np.array_equal(lio.eskf_get_cov(), ref[2])
    finally:
        lio.ctx.set_armed_launch(1)
        lio.close()
