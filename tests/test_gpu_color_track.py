"""Keeping the camera tracker's point set on the device (srl_color_map_track_update: opticalFlowTracker::updateAndAppendTrackPoints,
opticalFlowTracker.cpp:13-102) against the sequential restatement of tests/track_checker.py and the records of
tests/golden/golden_color_track.npz.

Every comparison is byte for byte, through the C-ABI: the records (pool position, u, v, flag), both outcome arrays and the totals of
every call of track_checker.cases() -- the sizes around a wave and a workgroup, budgets around the number of winners, full sets whose
first processed candidate wins or loses, repeats, unknown positions and duplicates, three cell sizes, both margins."""
import ctypes as C
import os

import numpy as np
import pytest

import color_checker as cc
import render_checker as rk
import select_checker as sk
import track_checker as tk
import sr_livo_amd as srl
from sr_livo_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRL_ERR_BAD_ARG, SRL_ERR_NO_MAP = -3, -5               # include/srlivo_hip.h: srl_status


def _cam(c):
    return capi.ColorCamera((C.c_double * 4)(*c.q), (C.c_double * 3)(*c.t), c.fx, c.fy, c.cx, c.cy, c.fov_margin)


def _scene_ctx():
    """the device map of tests/test_gpu_color_select.py's _scene_ctx: the scene's three insertions"""
    ctx = srl.Context(0)
    opt = rk.OPT
    ctx.color_map_create(capi.default_color_opts(size_voxel_map=opt[0], max_num_points_in_voxel=opt[1], min_distance_points=opt[2], add_point_step=opt[3]))
    for j in range(3):
        ctx.color_map_insert(cc.scene_batch(j), rk.BATCH_TIMES[j], 0.0)
    return ctx


def _opts(md, maximum):
    return capi.default_color_track_opts(mini_distance=md, maximum_tracked_points=maximum)


def _call(ctx, case, **kw):
    _, k, margin, tracked, cand, md, maximum = case
    cam, rows, cols, _ = sk.scene_camera(k, margin)
    return ctx.color_map_track_update(_cam(cam), rows, cols, tracked, cand, _opts(md, maximum), **kw)


def _same(got, want, what=""):
    rec, t_out, c_out, tot = got
    assert tot.as_tuple() == tk.totals_tuple(want[3]), (what, tot.as_tuple(), tk.totals_tuple(want[3]))
    assert rec.dtype == want[0].dtype == capi.COLOR_TRACK_POINT_DTYPE == tk.TRACK_POINT_DTYPE
    assert t_out.tobytes() == want[1].tobytes(), (what, np.flatnonzero(t_out != want[1])[:8], t_out[t_out != want[1]][:8], want[1][t_out != want[1]][:8])
    assert c_out.tobytes() == want[2].tobytes(), (what, np.flatnonzero(c_out != want[2])[:8], c_out[c_out != want[2]][:8], want[2][c_out != want[2]][:8])
    assert rec.tobytes() == want[0].tobytes(), (what, np.flatnonzero(rec != want[0])[:8] if len(rec) == len(want[0]) else (len(rec), len(want[0])))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_color_track.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def scene():
    ctx = _scene_ctx()
    yield ctx
    ctx.close()


# ------------------------------------------------------------------------------------------------ what the sequence holds
def test_preconditions_from_the_checker_alone():
    """every branch over the sequence, and the sizes and cases that have to appear, counted by the checker"""
    cases, results = tk.cases(), tk.case_results()
    census = {name: sum(r[4][name] for r in results) for name in tk.CENSUS}
    print("census over the sequence:", census)
    for name, floor in (("kept_flagged", 20), ("second_strike", 20), ("beyond_twice", 20), ("kept_outside", 20), ("behind", 5),
                        ("occupied_by_tracked", 50), ("occupied_by_candidate", 50), ("already_tracked", 20), ("readded", 10)):
        assert census[name] >= floor, (name, census[name])
    assert {0, 1, 63, 64, 65, 300} <= {len(c[3]) for c in cases}
    assert {0, 1, 255, 256, 257} <= {len(c[4]) for c in cases} and max(len(c[4]) for c in cases) > 3000
    assert {10.0, 7.5, 0.4} <= {c[5] for c in cases} and {0.005, -0.4} <= {c[2] for c in cases}
    by_name = {c[0]: (c, r) for c, r in zip(cases, results)}
    # the several thousand: both all-points selections at minimum_dis 10, every candidate reached
    c, r = by_name["both"]
    assert len(c[4]) == sum(len(s[0]) for s in sk.all_points_results(3)) and not (r[2] == tk.NOT_REACHED).any() and r[3]["cut"] == 0
    # budgets: more than the winners, exactly the winners, one
    free = by_name["budget_more"][1]
    s0, winners = free[3]["kept"], free[3]["added"]
    assert winners > 100 and free[3]["cut"] == 0 and by_name["budget_more"][0][6] - s0 > winners
    c, r = by_name["budget_exact"]
    assert c[6] - s0 == winners and r[3]["added"] == winners and r[3]["cut"] == 0 and (r[2] == tk.NOT_REACHED).sum() > 0
    c, r = by_name["budget_one_less"]
    assert r[3]["added"] == winners - 1 and r[3]["cut"] == 1
    c, r = by_name["budget_1"]
    assert c[6] - s0 == 1 and r[3]["added"] == 1 and r[3]["cut"] == winners - 1
    # full sets
    for label, added in (("wins", 1), ("loses", 0)):
        for which, delta in (("equal", 0), ("above", -5)):
            c, r = by_name["full_%s_%s" % (which, label)]
            assert c[6] == s0 + delta == r[3]["kept"] + delta and r[3]["added"] == added and r[2][0] == (tk.ADDED if added else tk.REFUSED)
            assert (r[2][1:] >= tk.CUT).all() and r[3]["cut"] > 100
    assert by_name["full_zero"][1][3]["added"] == 1 and by_name["full_negative"][1][3]["added"] == 1 and by_name["full_negative"][0][6] < 0
    # repeats, unknown positions, duplicates
    r = by_name["odd"][1]
    assert r[3]["cand_unknown"] == 4 and r[3]["unknown"] == 2 and r[3]["duplicate"] >= 20 and r[3]["already_tracked"] > 300


def test_every_call_of_the_sequence_equals_the_restatement_and_the_golden(scene, golden):
    assert [str(n) for n in golden["names"]] == [c[0] for c in tk.cases()]
    assert scene.color_map_size()[0] == len(tk.pool_positions())
    for case, want in zip(tk.cases(), tk.case_results()):
        got = _call(scene, case)
        _same(got, want, case[0])
        assert tk.golden_check(golden, case[0], got[0], got[1], got[2], got[3].as_tuple()) is None, case[0]
        kept = got[3].kept
        assert np.array_equal(got[0]["pool"][:kept], case[3]["pool"][got[1] <= tk.KEPT_FLAGGED])            # the kept points in input order
        assert np.array_equal(got[0]["pool"][kept:], case[4][got[2] == tk.ADDED]) and (got[0]["flagged"][kept:] == 0).all()


def test_the_same_call_twice_and_without_any_optional_output(scene):
    by_name = {c[0]: c for c in tk.cases()}
    for name in ("narrow", "odd", "full_equal_wins"):
        first, second = _call(scene, by_name[name]), _call(scene, by_name[name])
        assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes() and first[2].tobytes() == second[2].tobytes()
        assert first[3].as_tuple() == second[3].as_tuple()
        _, k, margin, tracked, cand, md, maximum = by_name[name]
        cam, rows, cols, _ = sk.scene_camera(k, margin)
        tot = capi.ColorTrackTotals()
        o = _opts(md, maximum)
        rc = scene.lib.srl_color_map_track_update(scene.h, C.byref(_cam(cam)), rows, cols, capi._ptr(tracked), len(tracked), capi._ptr(cand), len(cand), C.byref(o),
                                                  None, 0, None, None, C.byref(tot))
        assert rc == capi.SRL_OK and tot.as_tuple() == first[3].as_tuple()
        assert scene.lib.srl_color_map_track_update(scene.h, C.byref(_cam(cam)), rows, cols, capi._ptr(tracked), len(tracked), capi._ptr(cand), len(cand),
                                                    C.byref(o), None, 0, None, None, None) == capi.SRL_OK


def test_a_capacity_below_the_records_is_refused_with_the_totals_and_the_same_call_then_succeeds(scene):
    case = {c[0]: c for c in tk.cases()}["track1"]
    want = tk.case_results()[[c[0] for c in tk.cases()].index("track1")]
    _, k, margin, tracked, cand, md, maximum = case
    cam, rows, cols, _ = sk.scene_camera(k, margin)
    need = len(want[0])
    out = np.full(need, -1, dtype=capi.COLOR_TRACK_POINT_DTYPE)
    t_out, c_out = np.full(len(tracked), 77, np.uint8), np.full(len(cand), 77, np.uint8)
    tot = capi.ColorTrackTotals()
    o = _opts(md, maximum)

    def call(capacity):
        return scene.lib.srl_color_map_track_update(scene.h, C.byref(_cam(cam)), rows, cols, capi._ptr(tracked), len(tracked), capi._ptr(cand), len(cand),
                                                    C.byref(o), capi._ptr(out), capacity, capi._ptr(t_out), capi._ptr(c_out), C.byref(tot))
    assert call(need - 1) == SRL_ERR_BAD_ARG
    assert tot.as_tuple() == tk.totals_tuple(want[3]) and (out["pool"] == -1).all() and (t_out == 77).all() and (c_out == 77).all()      # nothing copied
    assert call(need) == capi.SRL_OK
    _same((out, t_out, c_out, tot), want, "after the refusal")


def test_a_selection_before_and_after_is_unchanged(scene):
    cam, rows, cols, _ = sk.scene_camera(0, 0.005)
    so = capi.default_color_select_opts(use_all_points=1)
    before = scene.color_map_select(_cam(cam), rows, cols, None, so)
    assert before[0].tobytes() == sk.all_points_results(3)[0][0].tobytes()
    size = scene.color_map_size()
    _call(scene, {c[0]: c for c in tk.cases()}["narrow"])
    after = scene.color_map_select(_cam(cam), rows, cols, None, so)
    assert before[0].tobytes() == after[0].tobytes() and before[1].as_tuple() == after[1].as_tuple() and scene.color_map_size() == size


def test_a_map_nothing_was_inserted_into_knows_no_position():
    ctx = srl.Context(0)
    try:
        ctx.color_map_create()
        cam, rows, cols, _ = sk.scene_camera(0, 0.005)
        tracked = np.zeros(3, capi.COLOR_TRACK_POINT_DTYPE)
        rec, t_out, c_out, tot = ctx.color_map_track_update(_cam(cam), rows, cols, tracked, np.arange(5, dtype=np.int32))
        assert len(rec) == 0 and (t_out == tk.UNKNOWN).all() and (c_out == tk.CAND_UNKNOWN).all()
        assert tot.as_tuple() == (3, 0, 0, 0, 0, 3, 0, 5, 0, 5, 0, 0, 0, 0)
        rec, t_out, c_out, tot = ctx.color_map_track_update(_cam(cam), rows, cols, tracked[:0], np.zeros(0, np.int32))
        assert len(rec) == 0 and tot.as_tuple() == (0,) * 14
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_totals_zero():
    ctx = srl.Context(0)
    try:
        lib = ctx.lib
        cam, rows, cols, _ = sk.scene_camera(0, 0.005)
        one_t = np.zeros(1, capi.COLOR_TRACK_POINT_DTYPE)
        one_c = np.zeros(1, np.int32)

        def call(camera=None, r=rows, c=cols, t=one_t, n=1, cand=one_c, nc=1, o=None, capacity=0, with_cam=True, with_opts=True):
            tot = capi.ColorTrackTotals(*([7] * 14))
            camera = _cam(cam) if camera is None else camera
            o = _opts(10.0, 300) if o is None else o
            rc = lib.srl_color_map_track_update(ctx.h, C.byref(camera) if with_cam else None, r, c, capi._ptr(t), n, capi._ptr(cand), nc,
                                                C.byref(o) if with_opts else None, None, capacity, None, None, C.byref(tot))
            assert rc == capi.SRL_OK or tot.as_tuple() == (0,) * 14
            return rc
        assert call() == SRL_ERR_NO_MAP
        ctx.color_map_create()
        ctx.color_map_insert(cc.scene_batch(0)[:500], 1.0, 0.0)
        assert call() == capi.SRL_OK
        assert call(with_cam=False) == SRL_ERR_BAD_ARG and call(with_opts=False) == SRL_ERR_BAD_ARG
        assert call(t=None) == SRL_ERR_BAD_ARG and call(cand=None) == SRL_ERR_BAD_ARG and call(n=-1) == SRL_ERR_BAD_ARG and call(nc=-1) == SRL_ERR_BAD_ARG
        assert call(capacity=-1) == SRL_ERR_BAD_ARG
        assert call(n=capi.SRL_COLOR_TRACK_MAX_POINTS + 1) == SRL_ERR_BAD_ARG and call(nc=capi.SRL_COLOR_TRACK_MAX_CANDIDATES + 1) == SRL_ERR_BAD_ARG
        for md in (0.0, -1.0, float("nan"), float("inf"), 65536.5):
            assert call(o=_opts(md, 300)) == SRL_ERR_BAD_ARG, md
        assert call(o=_opts(65536.0, 300)) == capi.SRL_OK
        assert call(r=1) == SRL_ERR_BAD_ARG and call(c=1) == SRL_ERR_BAD_ARG and call(r=8193, c=8192) == SRL_ERR_BAD_ARG
        assert call(r=8192, c=8192) == capi.SRL_OK and call(r=2, c=2) == capi.SRL_OK
        for field, value, want in (("fov_margin", 0.5, SRL_ERR_BAD_ARG), ("fov_margin", -4.001, SRL_ERR_BAD_ARG), ("fov_margin", float("nan"), SRL_ERR_BAD_ARG),
                                   ("fov_margin", -4.0, capi.SRL_OK), ("fov_margin", 0.499, capi.SRL_OK), ("fx", float("inf"), SRL_ERR_BAD_ARG),
                                   ("cy", float("nan"), SRL_ERR_BAD_ARG)):
            bad = _cam(cam)
            setattr(bad, field, value)
            assert call(camera=bad) == want, (field, value)
        ctx.comm_set_host_callbacks(2, 0, lambda a: None, lambda v: [v, v])       # more than one rank
        assert call() == capi.SRL_ERR_UNSUPPORTED
        ctx.comm_set_host_callbacks(1, 0, None, None)
        assert call() == capi.SRL_OK
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the loop of imageProcessing::process
def test_the_loop_of_process_through_the_mirrors_handles(scene):
    """select -> srl_oft_init -> a second gray image through srl_flow_track_image -> all-ones providers for the fundamental matrix and PnP
    -> trackedForVio into srl_color_map_vio_rows -> updateAndAppendTrackPoints (imageProcessing.cpp:137-161).  The set sizes at every
    step, the mirror's order (ascending pool position) and the point set behind the update, which is the checker's."""
    import flow_checker as fc
    cam, rows, cols, _ = sk.scene_camera(0, 0.005)
    sel, sel_tot = scene.color_map_select(_cam(cam), rows, cols, None, capi.default_color_select_opts(use_all_points=1))
    assert sel_tot.selected > 1000
    tex = fc.texture(77, rows, cols)
    gray0, gray1 = fc.crop(tex, rows, cols, 0, 0), fc.crop(tex, rows, cols, -2, -3)       # the content moves by (+3, +2) pixels
    oft = srl.Oft(scene)
    try:
        first = sel[:300]
        oft.init(first, gray0, 10.0)
        order = np.sort(first["pool"])
        assert oft.sizes() == (300, 0, 300, 0) and np.array_equal(oft.pose_map(0)["pool"], order)
        oft.set_fundamental_provider(lambda last, cur, status: (status.__setitem__(slice(None), 1), 0)[1])
        oft.set_pnp_provider(lambda xyz, uv: (0, np.arange(len(uv))))
        n_cur = oft.track_image(gray1, 10.1, rows, cols)
        cur = oft.pose_map(1)
        assert 100 < n_cur <= 300 and len(cur) == n_cur and (np.diff(cur["pool"]) > 0).all() and set(cur["pool"]) <= set(order)
        by_pool = {int(r["pool"]): r for r in first}
        moved = np.array([[r["u"] - by_pool[int(r["pool"])]["u"], r["v"] - by_pool[int(r["pool"])]["v"]] for r in cur])
        assert np.abs(np.median(moved, axis=0) - (3.0, 2.0)).max() < 0.25          # the device's flow, not a stand-in
        assert oft.sizes() == (300, n_cur, 300, 0) and oft.times() == (10.1, 10.1)
        assert oft.remove_outlier_using_ransac_pnp(1) is True
        assert oft.sizes() == (n_cur, n_cur, n_cur, 0) and oft.pose_map(0).tobytes() == cur.tobytes()
        vio = oft.tracked_for_vio()
        assert np.array_equal(vio["pool"], cur["pool"]) and np.array_equal(vio["match_u"], cur["u"].astype(np.float64))
        vel = np.stack([vio["vel_u"], vio["vel_v"]], 1)
        assert np.abs(np.median(vel, axis=0) - (30.0, 20.0)).max() < 2.5 and (vel != 0).any(axis=1).all()
        args = capi.ColorVioArgs(_cam(cam), 0.0, (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), capi.SRL_VIO_REPROJECTION, 1, 1)
        sums, _, outcome = scene.color_map_vio_rows(args, vio)
        assert sums.used == n_cur and (outcome == 0).all()
        tracked = oft.pose_map(0)
        tot = oft.update_and_append_track_points(_cam(cam), rows, cols, sel, tk.MINI_DISTANCE)
        want = tk.track_update_sequential(tk.pool_positions(), cam, rows, cols, tracked, sel["pool"], tk.MINI_DISTANCE, tk.MAXIMUM_TRACKED_POINTS)
        assert tot.as_tuple() == tk.totals_tuple(want[3]) and tot.tracked_in == n_cur and tot.kept + tot.added == 300 and tot.added > 0
        after = oft.pose_map(0)
        assert after.tobytes() == np.sort(want[0], order="pool").tobytes() and oft.sizes() == (300, n_cur, 300, tot.flagged)
    finally:
        oft.close()
