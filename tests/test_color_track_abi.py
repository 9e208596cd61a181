"""CPU-only contract of the tracker's point set: srl_color_map_track_update's declarations, layouts, defaults and the refusals made before
a device is touched, and the host-only paths of the mirror's opticalFlowTracker (srl_oft_*, csrc/host/opticalFlowTracker.cpp) with
ctypes callbacks as providers -- the < 30 return, the two reduce_vector rounds, the acceptance loop and the velocity, the PnP rebuild
and the flags of points that left the set flagged -- against a short Python restatement of opticalFlowTracker.cpp:111-186, :267-323."""
import ctypes as C
import math
import os
import re

import numpy as np

import sr_livo_amd as srl
import track_checker as tk
from sr_livo_amd import capi

SRL_ERR_BAD_ARG = -3          # include/srlivo_hip.h: srl_status
CSRC = os.path.join(os.path.dirname(capi.INCLUDE_DIR), "sr_livo_amd", "csrc")
F32 = np.float32
NEW = ("srl_color_track_opts_default", "srl_color_map_track_update", "srl_oft_create", "srl_oft_destroy", "srl_oft_set_maximum_tracked_points",
       "srl_oft_set_flow_provider", "srl_oft_set_fundamental_provider", "srl_oft_set_pnp_provider", "srl_oft_set_update_provider", "srl_oft_set_track_points",
       "srl_oft_init", "srl_oft_track_image", "srl_oft_remove_outlier_using_ransac_pnp", "srl_oft_update_and_append_track_points", "srl_oft_sizes",
       "srl_oft_times", "srl_oft_pose_map", "srl_oft_tracked_for_vio")


def _fields(header, struct):
    m = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", header, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return tuple(re.findall(r"\b([A-Za-z_]+)(?:\[\d+\])?\s*[,;]", body))


def test_the_entry_points_are_declared_and_exported():
    lib = srl.load_library()
    for name in NEW:
        assert name in srl.declared_symbols() and hasattr(lib, name), name
    hip = open(os.path.join(capi.INCLUDE_DIR, "srlivo_hip.h")).read()
    assert re.search(r"\bint srl_color_map_track_update\(srl_ctx \*ctx, const srl_color_camera \*cam, int image_rows, int image_cols,", hip)
    assert "#define SRL_COLOR_TRACK_MAX_POINTS     65536" in hip and capi.SRL_COLOR_TRACK_MAX_POINTS == 65536
    assert "#define SRL_COLOR_TRACK_MAX_CANDIDATES 1048576" in hip and capi.SRL_COLOR_TRACK_MAX_CANDIDATES == 1048576
    assert ("SRL_TRACK_KEPT = 0, SRL_TRACK_KEPT_FLAGGED = 1, SRL_TRACK_DROPPED = 2, SRL_TRACK_BEHIND = 3, SRL_TRACK_UNKNOWN = 4, "
            "SRL_TRACK_DUPLICATE = 5") in hip
    assert (capi.SRL_TRACK_KEPT, capi.SRL_TRACK_KEPT_FLAGGED, capi.SRL_TRACK_DROPPED, capi.SRL_TRACK_BEHIND, capi.SRL_TRACK_UNKNOWN,
            capi.SRL_TRACK_DUPLICATE) == (tk.KEPT, tk.KEPT_FLAGGED, tk.DROPPED, tk.BEHIND, tk.UNKNOWN, tk.DUPLICATE) == tuple(range(6))
    assert re.search(r"SRL_TRACK_CAND_ADDED = 0, SRL_TRACK_CAND_ALREADY_TRACKED = 1, SRL_TRACK_CAND_UNKNOWN = 2, SRL_TRACK_CAND_REFUSED = 3, "
                     r"SRL_TRACK_CAND_OCCUPIED = 4,\s+SRL_TRACK_CAND_CUT = 5, SRL_TRACK_CAND_NOT_REACHED = 6", hip)
    assert (capi.SRL_TRACK_CAND_ADDED, capi.SRL_TRACK_CAND_ALREADY_TRACKED, capi.SRL_TRACK_CAND_UNKNOWN, capi.SRL_TRACK_CAND_REFUSED,
            capi.SRL_TRACK_CAND_OCCUPIED, capi.SRL_TRACK_CAND_CUT, capi.SRL_TRACK_CAND_NOT_REACHED) == \
        (tk.ADDED, tk.ALREADY_TRACKED, tk.CAND_UNKNOWN, tk.REFUSED, tk.OCCUPIED, tk.CUT, tk.NOT_REACHED) == tuple(range(7))
    # the function is no longer named as the caller's
    for path in (os.path.join(capi.INCLUDE_DIR, "srlivo_hip.h"), os.path.join(CSRC, "host", "imageProcessing.h")):
        assert not re.search(r"and\s+updateAndAppendTrackPoints\s+stay with the caller|equalisation and updateAndAppendTrackPoints", open(path).read()), path


def test_structures_have_one_layout_on_both_sides_and_the_defaults():
    hip = open(os.path.join(capi.INCLUDE_DIR, "srlivo_hip.h")).read()
    assert capi.COLOR_TRACK_POINT_DTYPE.itemsize == 16 and capi.COLOR_TRACK_POINT_DTYPE == tk.TRACK_POINT_DTYPE
    assert C.sizeof(capi.ColorTrackOpts) == 16 and C.sizeof(capi.ColorTrackTotals) == 14 * 8
    assert _fields(hip, "srl_color_track_point") == capi.COLOR_TRACK_POINT_DTYPE.names
    assert _fields(hip, "srl_color_track_opts") == tuple(f for f, _ in capi.ColorTrackOpts._fields_)
    assert _fields(hip, "srl_color_track_totals") == tuple(f for f, _ in capi.ColorTrackTotals._fields_) == tk.TOTALS
    src = open(os.path.join(CSRC, "srl_color_track.hip")).read()
    assert "static_assert(sizeof(srl_color_track_point) == 16" in src and "static_assert(sizeof(srl_color_track_totals) == 14 * 8" in src
    o = capi.default_color_track_opts()
    assert (o.mini_distance, o.maximum_tracked_points, o.reserved) == (tk.MINI_DISTANCE, tk.MAXIMUM_TRACKED_POINTS, 0) == (10.0, 300, 0)
    srl.load_library().srl_color_track_opts_default(None)


def test_refusals_without_a_context_zero_the_totals_and_copy_nothing():
    lib = srl.load_library()
    cam = capi.ColorCamera((C.c_double * 4)(1, 0, 0, 0), (C.c_double * 3)(0, 0, 0), 200.0, 200.0, 320.0, 240.0, 0.005)
    o = capi.default_color_track_opts()
    t = np.zeros(2, capi.COLOR_TRACK_POINT_DTYPE)
    c = np.zeros(3, np.int32)
    out = np.full(5, -1, capi.COLOR_TRACK_POINT_DTYPE)
    t_out, c_out = np.full(2, 9, np.uint8), np.full(3, 9, np.uint8)

    def call(ctx=None, camera=cam, rows=480, cols=640, tracked=t, n=2, cand=c, nc=3, opts=o, capacity=5):
        tot = capi.ColorTrackTotals(*([7] * 14))
        rc = lib.srl_color_map_track_update(ctx, C.byref(camera) if camera is not None else None, rows, cols, capi._ptr(tracked), n, capi._ptr(cand), nc,
                                            C.byref(opts) if opts is not None else None, capi._ptr(out), capacity, capi._ptr(t_out), capi._ptr(c_out),
                                            C.byref(tot))
        assert tot.as_tuple() == (0,) * 14 and (out["pool"] == -1).all() and (t_out == 9).all() and (c_out == 9).all()
        return rc
    # every refusal made before a device is touched, on a NULL context: the context is the first of them
    for kw in (dict(), dict(camera=None), dict(opts=None), dict(tracked=None), dict(cand=None), dict(n=-1), dict(nc=-1), dict(capacity=-1),
               dict(n=capi.SRL_COLOR_TRACK_MAX_POINTS + 1), dict(nc=capi.SRL_COLOR_TRACK_MAX_CANDIDATES + 1), dict(rows=1), dict(cols=1),
               dict(opts=capi.default_color_track_opts(mini_distance=0.0)), dict(opts=capi.default_color_track_opts(mini_distance=float("nan"))),
               dict(opts=capi.default_color_track_opts(mini_distance=65536.5)), dict(n=0, nc=0)):
        assert call(**kw) == SRL_ERR_BAD_ARG, kw
    assert lib.srl_color_map_track_update(None, None, 0, 0, None, 0, None, 0, None, None, 0, None, None, None) == SRL_ERR_BAD_ARG
    # the mirror's handles
    assert lib.srl_oft_create(None, None) == SRL_ERR_BAD_ARG and lib.srl_oft_destroy(None) == capi.SRL_OK
    n = C.c_int(5)
    assert lib.srl_oft_track_image(None, None, 0, 0, 0, 0.0, 0, 0, C.byref(n)) == SRL_ERR_BAD_ARG and n.value == 0
    assert lib.srl_oft_pose_map(None, 0, None, 0, C.byref(n)) == SRL_ERR_BAD_ARG and lib.srl_oft_tracked_for_vio(None, None, 0, C.byref(n)) == SRL_ERR_BAD_ARG
    assert lib.srl_oft_sizes(None, None, None, None, None) == SRL_ERR_BAD_ARG and lib.srl_oft_remove_outlier_using_ransac_pnp(None, 1, C.byref(n)) == SRL_ERR_BAD_ARG


# ------------------------------------------------------------------------------------------------ the mirror's host-only paths
ROWS, COLS = 480, 640


def _records(n, seed=5):
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, capi.COLOR_SELECTED_DTYPE)
    rec["pool"] = rng.permutation(4 * n)[:n].astype(np.int32)                # not in pool order: the mirror sorts
    rec["index"] = np.arange(n)
    rec["x"], rec["y"], rec["z"] = rng.normal(size=(3, n)).astype(F32)
    rec["u"] = rng.uniform(20, COLS - 20, n).astype(F32)
    rec["v"] = rng.uniform(20, ROWS - 20, n).astype(F32)
    return rec


def _flow(shift):
    """a stand-in flow: every point moves by `shift` (some out of the 5 % margin), every seventh is lost"""
    def fn(gray, rows, cols, stride, prev, nxt, status):
        nxt[:] = prev + np.asarray(shift, F32)
        status[:] = 1
        status[::7] = 0
        return 0
    return fn


def _available(x, y):
    """if2dPointsAvailable(x, y, 1.0, 0.05) on the frame (lioOptimization.cpp:48-60)"""
    u, v = float(x), float(y)
    return u / 1.0 >= 0.05 * COLS + 1 and math.ceil(u / 1.0) < (1 - 0.05) * COLS and v / 1.0 >= 0.05 * ROWS + 1 and math.ceil(v / 1.0) < (1 - 0.05) * ROWS


def _track_image_restated(last_map, shift, fmask_step, dt):
    """trackImage :124-171 on a dict pool -> (u, v) walked by ascending pool: (cur map, velocities)"""
    pools = sorted(last_map)
    last = [last_map[p] for p in pools]
    cur = [(F32(u + F32(shift[0])), F32(v + F32(shift[1]))) for u, v in last]
    keep = [i for i in range(len(pools)) if i % 7 != 0]                       # reduce_vector by the flow's status
    keep = [i for k, i in enumerate(keep) if k % fmask_step != 0]             # ... and by the fundamental matrix's
    cur_map, vel = {}, {}
    for i in keep:
        if _available(*cur[i]):
            cur_map[pools[i]] = cur[i]
            if dt < 1e-5:
                pv = (F32(1e-3), F32(1e-3))
            else:
                pv = (F32(float(F32(cur[i][0] - last[i][0])) / dt), F32(float(F32(cur[i][1] - last[i][1])) / dt))      # Point2f - Point2f, then / double
            vel[pools[i]] = (float(pv[0]), float(pv[1]))
    return cur_map, vel


def test_track_image_reduces_accepts_and_forms_the_velocity_as_restated():
    gray = np.zeros((ROWS, COLS), np.uint8)
    rec = _records(120)
    for shift, t0, t1 in (((3.25, -1.5), 1.0, 1.1), ((-9.0, 14.0), 2.0, 2.0 + 1e-6), ((0.1, 0.3), 5.0, 5.0333)):
        oft = srl.Oft(None)
        try:
            oft.set_flow_provider(_flow(shift))
            oft.init(rec, gray, t0)
            assert oft.sizes() == (120, 0, 120, 0) and oft.times() == (t0, t0)
            assert np.array_equal(oft.pose_map(0)["pool"], np.sort(rec["pool"]))                    # ascending pool position
            # no fundamental-matrix provider: refused, not defaulted
            try:
                oft.track_image(gray, t1, ROWS, COLS)
                raise AssertionError("accepted without a provider")
            except srl.SrlError as e:
                assert e.status == SRL_ERR_BAD_ARG

            def fundamental(last, cur, status):
                status[:] = 1
                status[::5] = 0
                return 0
            oft.set_fundamental_provider(fundamental)
            n_cur = oft.track_image(gray, t1, ROWS, COLS)
            last_map = {int(r["pool"]): (r["u"], r["v"]) for r in rec}
            want_cur, want_vel = _track_image_restated(last_map, shift, 5, t1 - t0)
            got = oft.pose_map(1)
            assert n_cur == len(want_cur) == len(got) and 20 < n_cur < 120
            assert [int(p) for p in got["pool"]] == sorted(want_cur)
            assert all(want_cur[int(r["pool"])] == (r["u"], r["v"]) for r in got)
            # the last map is untouched and the vectors are rebuilt from it (:180-182)
            assert oft.sizes()[:3] == (120, n_cur, 120) and oft.times() == (t1, t1)
            vio = oft.tracked_for_vio()
            assert np.array_equal(vio["pool"], np.sort(rec["pool"])) and len(want_vel) == n_cur
            for r in vio:
                assert (r["vel_u"], r["vel_v"]) == want_vel.get(int(r["pool"]), (0.0, 0.0))
                assert (r["match_u"], r["match_v"]) == tuple(float(x) for x in last_map[int(r["pool"])])
            if t1 - t0 < 1e-5:
                assert set(want_vel.values()) == {(float(F32(1e-3)), float(F32(1e-3)))}
        finally:
            oft.close()


def test_fewer_than_thirty_points_only_move_the_time_and_an_empty_image_only_clears():
    gray = np.zeros((ROWS, COLS), np.uint8)
    calls = []
    oft = srl.Oft(None)
    try:
        def flow(gray_, rows, cols, stride, prev, nxt, status):
            calls.append(len(prev))
            nxt[:] = prev
            return 0
        oft.set_flow_provider(flow)
        oft.set_fundamental_provider(lambda last, cur, status: 1 / 0)
        oft.init(_records(29), gray, 1.0)
        assert calls == [29]
        assert oft.track_image(gray, 1.5, ROWS, COLS) == 0 and calls == [29]                      # :128-132
        assert oft.times() == (1.5, 1.5) and oft.sizes() == (29, 0, 29, 0)
        assert oft.track_image(None, 1.75, ROWS, COLS) == 0 and oft.times() == (1.5, 1.75)         # cur_image.empty(): the last time stays
    finally:
        oft.close()


def test_the_pnp_rebuild_and_its_gates():
    gray = np.zeros((ROWS, COLS), np.uint8)
    rec = _records(60, seed=9)
    oft = srl.Oft(None)
    try:
        oft.set_flow_provider(_flow((1.0, 1.0)))
        oft.set_fundamental_provider(lambda last, cur, status: (status.__setitem__(slice(None), 1), 0)[1])
        oft.init(rec, gray, 1.0)
        assert oft.remove_outlier_using_ransac_pnp(1) is False                                  # :286-289: fewer than 10 in the current map
        oft.track_image(gray, 1.1, ROWS, COLS)
        cur = oft.pose_map(1)
        seen = {}

        def pnp(xyz, uv):
            seen["xyz"], seen["uv"] = xyz.copy(), uv.copy()
            return 0, np.arange(len(uv))[::-3]                               # inliers in descending order: the maps sort them again
        try:
            oft.remove_outlier_using_ransac_pnp(1)
            raise AssertionError("accepted without a provider")
        except srl.SrlError as e:
            assert e.status == SRL_ERR_BAD_ARG
        oft.set_pnp_provider(lambda xyz, uv: (-3, []))                                          # the caught cv::Exception
        assert oft.remove_outlier_using_ransac_pnp(1) is False and oft.sizes()[:2] == (60, len(cur))
        oft.set_pnp_provider(pnp)
        assert oft.remove_outlier_using_ransac_pnp(0) is True and oft.sizes()[:2] == (60, len(cur))      # no removal: only the vectors are rebuilt
        by_pool = {int(r["pool"]): r for r in rec}
        assert np.array_equal(seen["uv"], np.stack([cur["u"], cur["v"]], 1))
        assert np.array_equal(seen["xyz"], np.array([[by_pool[int(p)][k] for k in ("x", "y", "z")] for p in cur["pool"]], F32))
        assert oft.remove_outlier_using_ransac_pnp(1) is True
        inl = np.sort(np.arange(len(cur))[::-3])
        for which in (0, 1):
            m = oft.pose_map(which)
            assert m.tobytes() == cur[inl].tobytes()                        # both maps hold the inliers' CURRENT pixels (:314-315)
        assert oft.sizes()[:3] == (len(inl), len(inl), len(inl))
        oft.set_pnp_provider(lambda xyz, uv: (0, [len(uv)]))                                     # an index outside the list
        try:
            oft.remove_outlier_using_ransac_pnp(1)
            raise AssertionError("accepted a bad inlier index")
        except srl.SrlError as e:
            assert e.status == SRL_ERR_BAD_ARG
    finally:
        oft.close()


def test_a_point_that_left_the_set_flagged_comes_back_flagged():
    """through an update provider that keeps every second point flagged, drops the others and adds the first candidates with flag 0, as
    the device call returns them"""
    gray = np.zeros((ROWS, COLS), np.uint8)
    rec = _records(40, seed=3)
    cam = capi.ColorCamera((C.c_double * 4)(1, 0, 0, 0), (C.c_double * 3)(0, 0, 0), 200.0, 200.0, 320.0, 240.0, 0.005)
    log = []

    def update(camera, rows, cols, tracked, cand, opts, out, tot):
        log.append((tracked.copy(), cand.copy(), opts.mini_distance, opts.maximum_tracked_points, len(out)))
        kept = tracked[::2].copy()
        kept["flagged"] = 1 - kept["flagged"] if log[-1][3] == 77 else 1
        held = set(int(p) for p in kept["pool"])
        new = [int(p) for p in cand if int(p) not in held][:5]
        out[:len(kept)] = kept
        for k, p in enumerate(new):
            out[len(kept) + k] = (p, 1.5, 2.5, 0)
        tot.tracked_in, tot.kept, tot.flagged, tot.dropped, tot.candidates, tot.added = len(tracked), len(kept), int(kept["flagged"].sum()), len(tracked) - len(kept), \
            len(cand), len(new)
        return 0
    oft = srl.Oft(None)
    try:
        oft.set_flow_provider(_flow((0.0, 0.0)))
        oft.set_update_provider(update)
        oft.init(rec, gray, 1.0)
        order = np.sort(rec["pool"])
        none = np.zeros(0, capi.COLOR_SELECTED_DTYPE)
        tot = oft.update_and_append_track_points(cam, ROWS, COLS, none, 7.5)
        assert (tot.kept, tot.flagged, tot.added) == (20, 20, 0) and log[-1][2:] == (7.5, 300, 40) and not log[-1][0]["flagged"].any()
        assert np.array_equal(log[-1][0]["pool"], order)                     # the tracked list goes out in ascending pool order
        m = oft.pose_map(0)
        assert np.array_equal(m["pool"], order[::2]) and (m["flagged"] == 1).all() and oft.sizes() == (20, 0, 20, 20)
        # the flagged points leave through the PnP rebuild: their flags stay with the points
        oft.set_track_points(rec[:0])
        assert oft.sizes() == (0, 0, 0, 20)
        cands = np.zeros(8, capi.COLOR_SELECTED_DTYPE)
        cands["pool"] = [order[0], order[1], order[2], 9000, order[4], 9001, 9002, 9003]
        cands["x"] = np.arange(8)
        tot = oft.update_and_append_track_points(cam, ROWS, COLS, cands)
        assert tot.added == 5 and log[-1][2:] == (10.0, 300, 8) and len(log[-1][0]) == 0
        m = oft.pose_map(0)
        assert [int(p) for p in m["pool"]] == sorted([int(order[0]), int(order[1]), int(order[2]), 9000, int(order[4])])
        assert {int(r["pool"]): int(r["flagged"]) for r in m} == {int(order[0]): 1, int(order[1]): 0, int(order[2]): 1, 9000: 0, int(order[4]): 1}
        assert (m["u"] == 1.5).all() and (m["v"] == 2.5).all()
        # ... and go into the next call as flagged; what the first loop keeps unflagged or drops loses its flag
        oft.set_maximum_tracked_points(77)
        oft.update_and_append_track_points(cam, ROWS, COLS, none)
        sent = log[-1][0]
        assert {int(r["pool"]): int(r["flagged"]) for r in sent} == {int(order[0]): 1, int(order[1]): 0, int(order[2]): 1, 9000: 0, int(order[4]): 1}
        assert log[-1][3] == 77
        m = oft.pose_map(0)
        assert [int(r["flagged"]) for r in m] == [1 - int(r["flagged"]) for r in sent[::2]]
        assert oft.sizes()[3] == 20 - 3 + sum(1 - int(r["flagged"]) for r in sent[::2])          # the three tracked flags were reset, the kept ones set anew
    finally:
        oft.close()
