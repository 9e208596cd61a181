"""The coloured cloud from the device colour map (srl_color_map_export_cloud: the loops of lioOptimization::pubColorPoints,
threadPubColorPoints and saveColorPoints, lioOptimization.cpp:1210-1426) against the sequential restatement of
tests/cloud_export_checker.py -- which tests/test_cloud_export_checker_reference.py pins to the reference's own rgbPoint -- and against the
records of tests/golden/golden_color_cloud.npz.  Every comparison is bytewise, through the C-ABI: the records, their registered indices
and the totals.  Beyond one scan launch (131 072 elements) and beyond two levels (1 048 576) the export is compared with a NumPy filter of
the device's own srl_color_registered_download + srl_color_registered_rgb, which tests/test_gpu_color_map.py and
tests/test_gpu_color_render.py pin."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import cloud_export_checker as ck
import color_checker as cc
import render_checker as rk
import select_checker as sk
import sr_livo_amd as srl
from sr_livo_amd import capi
from test_gpu_color_select import _EskfAdapter, _cam, _ctx, _opts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRL_ERR_BAD_ARG, SRL_ERR_NO_MAP = -3, -5               # include/srlivo_hip.h: srl_status
VIEWS = (0, 1, 3, 9)


def _copts(mv=1, reverse=False, since=-math.inf):
    return capi.default_color_cloud_opts(minimum_views=mv, reverse=1 if reverse else 0, since=since)


def _same_cloud(got, want, what=""):
    rec, idx, tot = got
    w_rec, w_idx, w_tot = want
    assert tot.as_tuple() == ck.totals_tuple(w_tot), (what, tot.as_tuple(), w_tot)
    assert tot.scanned == tot.published + tot.below_views + tot.stale
    assert rec.dtype == w_rec.dtype == capi.COLOR_CLOUD_DTYPE
    assert rec.tobytes() == w_rec.tobytes(), (what, np.flatnonzero(rec != w_rec)[:8] if len(rec) == len(w_rec) else (len(rec), len(w_rec)))
    assert np.array_equal(idx, w_idx), what


def _render(ctx, k, visited):
    cam, which, obs_time, voxels = rk.render_call(k, visited)
    ctx.color_image_upload(rk.scene_image(which))
    return ctx.color_map_render(_cam(cam), voxels, obs_time)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_color_cloud.npz"), allow_pickle=False)


# ------------------------------------------------------------------------------------------------ 1. the render scene
def test_the_scene_after_every_render_equals_the_restatement_and_the_golden(golden):
    golden_calls = {(k, mv, reverse, first, since): n for n, (k, mv, reverse, since, first) in enumerate(ck.GOLDEN_CALLS)}
    assert np.array_equal(golden["calls"], np.array([[c[0], c[1], int(c[2]), c[4]] for c in ck.GOLDEN_CALLS]))
    seen_golden = 0
    ctx = _ctx()
    try:
        visited = [ctx.color_map_insert(cc.scene_batch(j), rk.BATCH_TIMES[j], 0.0)[2] for j in range(3)]
        size = ctx.color_map_size()[2]
        assert size == len(ck.scene_registered()[0]) == 24388 and size <= 131072      # one scan launch
        # never rendered: no colour state, every point black at minimum_views 0, none at 1; and still no state afterwards
        _same_cloud(ctx.color_map_export_cloud(opts=_copts(0)), ck.pub_color_points(ck.never_rendered(), 0), "never rendered")
        rec, _, tot = ctx.color_map_export_cloud(opts=_copts(1))
        assert len(rec) == 0 and tot.as_tuple() == (size, 0, size, 0)
        rec, _, tot = ctx.color_map_export_cloud(opts=_copts(0, since=0.5))       # the time of a point never observed is 0
        assert len(rec) == 0 and tot.as_tuple() == (size, 0, 0, size)
        assert not any(a.any() for a in ctx.color_map_download_rgb())
        for k in range(len(rk.RENDERS)):
            _render(ctx, k, visited)
            for mv in VIEWS:
                for reverse in (False, True):
                    got = ctx.color_map_export_cloud(opts=_copts(mv, reverse))
                    _same_cloud(got, ck.scene_export(k, mv, reverse), (k, mv, reverse))
                    assert (np.diff(got[1]) < 0).all() if reverse else (np.diff(got[1]) > 0).all()
            for (gk, gmv, grev, gfirst, gsince), n in golden_calls.items():
                if gk == k:
                    rec, idx, tot = ctx.color_map_export_cloud(first=gfirst, opts=_copts(gmv, grev, gsince))
                    assert rec.tobytes() == golden["g%d_records" % n].tobytes() and np.array_equal(idx, golden["g%d_index" % n])
                    assert tot.as_tuple() == tuple(int(v) for v in golden["g%d_totals" % n])
                    assert len(rec) > 1000
                    seen_golden += 1
        assert seen_golden == len(ck.GOLDEN_CALLS)
        # windows, after the last render
        k = len(rk.RENDERS) - 1
        for mv in (0, 1, 3):
            whole_up, whole_dn = ck.scene_export(k, mv, False), ck.scene_export(k, mv, True)
            for first, count in ((11, 5), (1023, 2), (0, 0), (size, -1), (size - 1, 1)):
                for reverse, whole in ((False, whole_up), (True, whole_dn)):
                    got = ctx.color_map_export_cloud(first, count, _copts(mv, reverse))
                    _same_cloud(got, ck.export(ck.scene_registered()[k], first, count, mv, reverse), (first, count, mv, reverse))
                    inside = (whole[1] >= first) & (whole[1] < first + (count if count >= 0 else size - first))
                    assert got[0].tobytes() == whole[0][inside].tobytes() and np.array_equal(got[1], whole[1][inside])      # the slice of the whole
            got = ctx.color_map_export_cloud(1, -1, _copts(mv, True))           # saveColorPoints' range
            _same_cloud(got, ck.save_color_points(ck.scene_registered()[k], mv), ("save", mv))
            assert got[0].tobytes() == (whole_dn[0][:-1] if whole_dn[1][-1] == 0 else whole_dn[0]).tobytes()
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def rendered():
    """a device map holding the scene after all six renders"""
    ctx = _ctx()
    visited = [ctx.color_map_insert(cc.scene_batch(j), rk.BATCH_TIMES[j], 0.0)[2] for j in range(3)]
    for k in range(len(rk.RENDERS)):
        _render(ctx, k, visited)
    yield ctx, visited
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. since
def test_since_cuts_by_observation_time(rendered):
    ctx, _ = rendered
    k = len(rk.RENDERS) - 1
    for since in (10.3, 10.6):
        for mv, reverse in ((0, False), (1, False), (1, True), (3, False)):
            got = ctx.color_map_export_cloud(opts=_copts(mv, reverse, since))
            _same_cloud(got, ck.scene_export(k, mv, reverse, since), (since, mv, reverse))
            assert got[2].stale > 0 and got[2].published > 0
    a, b = ctx.color_map_export_cloud(opts=_copts(1, False, -math.inf)), ctx.color_map_export_cloud(opts=capi.default_color_cloud_opts())
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and a[2].as_tuple() == b[2].as_tuple() and a[2].stale == 0
    rec, _, tot = ctx.color_map_export_cloud(opts=_copts(0, False, math.inf))    # every finite time lies below +inf
    assert len(rec) == 0 and tot.stale == tot.scanned


# ------------------------------------------------------------------------------------------------ 3. the mirror: saveColorPoints skips index 0
def test_the_mirror_saves_descending_without_index_0_and_publishes_with_it():
    lio = srl.Lio(0)
    ctx = _ctx()
    try:
        o = rk.OPT
        lio.set_color_map_options(capi.default_color_opts(size_voxel_map=o[0], max_num_points_in_voxel=o[1], min_distance_points=o[2], add_point_step=o[3]))
        lio.set_color_times(time_last_process=0.0)
        for j in range(2):
            pts = cc.scene_batch(j)
            lio.add_points_to_map_at(pts, rk.BATCH_TIMES[j], to_rendering=(j == 1))
            ctx.color_map_insert(pts, rk.BATCH_TIMES[j], 0.0)
        voxels, _ = lio.color_visited(1)
        pose, which, obs_time, _ = rk.RENDERS[0]
        cam = rk.scene_camera(rk.POSES[pose], which)
        for c in (lio.ctx, ctx):
            c.color_image_upload(rk.scene_image(which))
        lio.render_points_in_recent_voxel(_cam(cam), obs_time)
        ctx.color_map_render(_cam(cam), voxels, obs_time)
        size = ctx.color_map_size()[2]
        rec, idx, tot = lio.color_cloud(1, 0)                               # saveColorPoints
        assert 0 not in idx and (np.diff(idx) < 0).all() and len(idx) == size - 1 and idx[0] == size - 1 and idx[-1] == 1
        want = ctx.color_map_export_cloud(1, -1, _copts(0, True))
        assert rec.tobytes() == want[0].tobytes() and np.array_equal(idx, want[1]) and tot.as_tuple() == want[2].as_tuple() == (size - 1, size - 1, 0, 0)
        rec, idx, tot = lio.color_cloud(0, 0)                               # pubColorPoints
        assert idx[0] == 0 and np.array_equal(idx, np.arange(size)) and tot.as_tuple() == (size, size, 0, 0)
        for which_loop, mv in ((0, 1), (1, 1), (0, 3)):
            got = lio.color_cloud(which_loop, mv)
            want = ctx.color_map_export_cloud(1 if which_loop else 0, -1, _copts(mv, bool(which_loop)))
            assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and got[2].as_tuple() == want[2].as_tuple()
        assert lio.color_cloud(0, 1)[2].published > 1000 and lio.color_cloud(0, 1)[2].below_views > 1000
        # the mirror's own methods, through their view: a first small cloud, then one that outgrows the buffers, then a smaller one again
        for which_loop, mv, with_index in ((0, 9, True), (1, 0, True), (0, 1, False), (1, 3, True), (0, 0, True)):
            got = lio.color_cloud_view(which_loop, mv, with_index)
            want = ctx.color_map_export_cloud(1 if which_loop else 0, -1, _copts(mv, bool(which_loop)))
            assert got[0].tobytes() == want[0].tobytes() and got[2].as_tuple() == want[2].as_tuple(), (which_loop, mv)
            assert (got[1] is None) if not with_index else np.array_equal(got[1], want[1])
        # the topics are slices of the one cloud
        p = lio.color_cloud(0, 1)[2].published
        sizes = lio.color_topic_sizes(p)
        assert sizes.sum() == p and len(sizes) == p // 1000 + 1 and (sizes[:-1] == 1000).all()
        # the handle's size query and a capacity that is too small
        n, tot = C.c_int64(), capi.ColorCloudTotals()
        assert lio.lib.srl_lio_color_cloud(lio.h, 0, 1, None, None, 0, C.byref(n), C.byref(tot)) == capi.SRL_OK and n.value == p == tot.published
        out = np.zeros(p, capi.COLOR_CLOUD_DTYPE)
        assert lio.lib.srl_lio_color_cloud(lio.h, 0, 1, capi._ptr(out), None, p - 1, C.byref(n), C.byref(tot)) == SRL_ERR_BAD_ARG
        assert n.value == p and not out.view(np.uint8).any()
    finally:
        ctx.close(); lio.close()


# ------------------------------------------------------------------------------------------------ 4. capacity
def test_capacity_and_two_runs(rendered):
    ctx, _ = rendered
    lib = ctx.lib
    o = _copts(1)
    tot = capi.ColorCloudTotals()
    assert lib.srl_color_map_export_cloud(ctx.h, 0, -1, C.byref(o), None, None, 0, C.byref(tot)) == capi.SRL_OK
    n, full = tot.published, tot.as_tuple()
    assert n > 1000
    out = np.full(n, 7, np.uint8).repeat(16).view(capi.COLOR_CLOUD_DTYPE)
    idx = np.full(n, 7, np.int32)
    before = out.tobytes()
    tot = capi.ColorCloudTotals()
    assert lib.srl_color_map_export_cloud(ctx.h, 0, -1, C.byref(o), capi._ptr(out), capi._ptr(idx), n - 1, C.byref(tot)) == SRL_ERR_BAD_ARG
    assert tot.as_tuple() == full and out.tobytes() == before and (idx == 7).all()      # the totals filled, nothing copied
    assert lib.srl_color_map_export_cloud(ctx.h, 0, -1, C.byref(o), capi._ptr(out), capi._ptr(idx), n, C.byref(tot)) == capi.SRL_OK
    want = ck.scene_export(len(rk.RENDERS) - 1, 1, False)
    assert out.tobytes() == want[0].tobytes() and np.array_equal(idx, want[1]) and tot.as_tuple() == full
    again = np.zeros(n, capi.COLOR_CLOUD_DTYPE)
    assert lib.srl_color_map_export_cloud(ctx.h, 0, -1, C.byref(o), capi._ptr(again), None, n, None) == capi.SRL_OK      # no indices, no totals
    assert again.tobytes() == out.tobytes()
    only = np.zeros(n, np.int32)
    assert lib.srl_color_map_export_cloud(ctx.h, 0, -1, C.byref(o), None, capi._ptr(only), n, None) == capi.SRL_OK       # the indices alone
    assert np.array_equal(only, idx)


def test_refusals_leave_the_totals_zero():
    ctx = srl.Context(0)
    try:
        lib = ctx.lib

        def call(first=0, count=-1, o=None, capacity=0, with_opts=True):
            tot = capi.ColorCloudTotals(7, 7, 7, 7)
            o = _copts() if o is None else o
            rc = lib.srl_color_map_export_cloud(ctx.h, first, count, C.byref(o) if with_opts else None, None, None, capacity, C.byref(tot))
            assert rc == capi.SRL_OK or tot.as_tuple() == (0,) * 4
            return rc, tot.as_tuple()
        assert call()[0] == SRL_ERR_NO_MAP
        ctx.color_map_create()
        assert call() == (capi.SRL_OK, (0,) * 4)                            # an empty map: an empty range
        ctx.color_map_insert(cc.scene_batch(0)[:500], 1.0, 0.0)
        size = ctx.color_map_size()[2]
        assert call() == (capi.SRL_OK, (size, 0, size, 0))
        assert call(with_opts=False)[0] == SRL_ERR_BAD_ARG and call(first=-1)[0] == SRL_ERR_BAD_ARG and call(capacity=-1)[0] == SRL_ERR_BAD_ARG
        assert call(o=_copts(since=math.nan))[0] == SRL_ERR_BAD_ARG
        assert call(first=size - 1, count=2)[0] == SRL_ERR_BAD_ARG and call(first=size + 1)[0] == SRL_ERR_BAD_ARG
        assert call(first=size - 1, count=1)[0] == capi.SRL_OK and call(first=size)[0] == capi.SRL_OK and call(first=3, count=0) == (capi.SRL_OK, (0,) * 4)
        ctx.comm_set_host_callbacks(2, 0, lambda a: None, lambda v: [v, v])       # more than one rank
        assert call()[0] == capi.SRL_ERR_UNSUPPORTED
        ctx.comm_set_host_callbacks(1, 0, None, None)
        assert call()[0] == capi.SRL_OK
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 5. beyond one scan launch, beyond two levels
def _lattice(nx, ny, nz, x0=0.0):
    """a 0.05-m lattice: eight points per 0.1-m voxel, every point in a grid cell of its own (0.01 m): all of them register"""
    g = np.mgrid[0:nx, 0:ny, 0:nz].reshape(3, -1).T.astype(np.float64)
    return g * 0.05 + np.array([x0 + 0.025, 0.025 - ny * 0.025, 0.025 - nz * 0.025])


def _downloads(ctx):
    """the path the export replaces: the device's own registered records and their colour state"""
    stored = ctx.color_registered_download()
    rgb, n_rgb, _, _, _ = ctx.color_registered_rgb()
    assert np.array_equal(stored["point_index"], np.arange(len(stored)))
    assert rgb.min() >= 0 and rgb.max() <= 255
    return stored, rgb, n_rgb


def _numpy_cloud(downloads, mv, reverse, first=0, count=None):
    """... and the host's filter over them"""
    stored, rgb, n_rgb = downloads
    idx = np.arange(len(stored), dtype=np.int32)[first:None if count is None else first + count]
    if reverse:
        idx = idx[::-1]
    idx = idx[n_rgb[idx] >= mv]
    rec = np.zeros(len(idx), capi.COLOR_CLOUD_DTYPE)
    for f in ("x", "y", "z"):
        rec[f] = stored[f][idx]
    rec["b"], rec["g"], rec["r"], rec["a"] = rgb[idx, 0], rgb[idx, 1], rgb[idx, 2], 255
    return rec, idx


@pytest.mark.parametrize("shape, threshold", [((40, 64, 64), 131072), ((2 * 66, 90, 90), 1048576)], ids=["two launches", "three levels"])
def test_the_scan_regimes_equal_a_filter_of_the_devices_own_downloads(shape, threshold):
    ctx = _ctx()
    try:
        visited = []
        half = shape[0] // 2
        for part in range(2):                                               # two insertions, each below the 1 M points one insertion takes
            pts = _lattice(half, shape[1], shape[2], x0=part * half * 0.05)
            assert len(pts) <= 1048576
            visited.append(ctx.color_map_insert(pts, 1.0 + part, 0.0, want_outcome=False, want_stored=False)[2])
        size = ctx.color_map_size()[2]
        assert size > threshold and size == shape[0] * shape[1] * shape[2]
        # one image over the visited lists, from inside the lattice: what the camera sees has N_rgb 1, the rest 0
        cam = rk.scene_camera((0.1, 0.35, 0.02, (-2.0, 0.0, 0.3)), 0)
        ctx.color_image_upload(rk.scene_image(0))
        ctx.color_map_render(_cam(cam), np.concatenate(visited), 10.0)
        down = _downloads(ctx)
        n_rgb = down[2]
        for mv in (0, 1):
            for reverse in (False, True):
                want_rec, want_idx = _numpy_cloud(down, mv, reverse)
                rec, idx, tot = ctx.color_map_export_cloud(opts=_copts(mv, reverse))
                assert rec.tobytes() == want_rec.tobytes() and np.array_equal(idx, want_idx), (mv, reverse)
                assert tot.as_tuple() == (size, len(want_rec), size - len(want_rec), 0)
        classes = (int((n_rgb == 0).sum()), int((n_rgb == 1).sum()))
        print("registered %d; N_rgb 0: %d, 1: %d" % ((size,) + classes))
        assert min(classes) > 1000 and sum(classes) == size                 # both classes, and no other
        for edge in (131072, 1048576):
            if edge < size:
                for first, count in ((edge - 5, 12), (edge - 700, 1400), (edge, 3), (edge - 1, 1)):
                    for reverse in (False, True):
                        want_rec, want_idx = _numpy_cloud(down, 1, reverse, first, count)
                        rec, idx, tot = ctx.color_map_export_cloud(first, count, _copts(1, reverse))
                        assert rec.tobytes() == want_rec.tobytes() and np.array_equal(idx, want_idx) and tot.scanned == count, (first, count, reverse)
        # a range that itself takes the next path and does not start at 0
        want_rec, want_idx = _numpy_cloud(down, 1, True, 7, size - 9)
        rec, idx, _ = ctx.color_map_export_cloud(7, size - 9, _copts(1, True))
        assert size - 9 > threshold and rec.tobytes() == want_rec.tobytes() and np.array_equal(idx, want_idx)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 6. existing calls unchanged
def test_a_render_and_a_select_after_an_export_give_the_bits_they_give_without_one():
    def run(with_exports):
        ctx = _ctx()
        try:
            visited = [ctx.color_map_insert(cc.scene_batch(j), rk.BATCH_TIMES[j], 0.0)[2] for j in range(3)]
            ctx.map_insert(cc.scene_batch(0))                               # a LiDAR map beside the colour map
            out = []
            for k in range(3):
                if with_exports:
                    ctx.color_map_export_cloud(opts=_copts(k, bool(k & 1)))
                out.append(_render(ctx, k, visited).as_tuple())
                if with_exports:
                    ctx.color_map_export_cloud(5, 1000, _copts(0, True, 10.05))
                cam, rows, cols, lists = sk.scene_camera(k, 0.005)
                rec, tot = ctx.color_map_select(_cam(cam), rows, cols, np.concatenate([visited[j] for j in lists]), _opts())
                out += [rec.tobytes(), tot.as_tuple()]
            out += [rk.state_bytes(ctx.color_map_download_rgb()), rk.state_bytes(ctx.color_registered_rgb()), ctx.color_registered_download().tobytes(),
                    b"".join(np.ascontiguousarray(a).tobytes() for a in ctx.color_map_download()), b"".join(a.tobytes() for a in ctx.map_download()),
                    ctx.color_map_size(), ctx.map_size()]
            return out
        finally:
            ctx.close()
    a, b = run(False), run(True)
    assert a == b and len(a[1]) > 0
    assert a[-7] == rk.state_bytes(rk.scene_sequence()[2][2])              # ... and they are the checker's


def test_an_export_cancels_an_armed_launch_and_the_next_solve_is_unchanged():
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
        lio.ctx.color_map_insert(pts, 1.0, 0.0)
        chk = cc.ColorChecker(*rk.OPT); chk.insert(pts, 1.0, 0.0)
        lio.ctx.set_armed_launch(2)                                        # a launch armed behind every eligible pass
        solve()
        s0 = lio.ctx.arm_stats()
        assert s0["armed"] > 0
        n = len(chk.registered)
        reg = ck.Registered(chk.registered_arrays()[0], np.zeros((n, 3), np.int16), np.zeros(n, np.int16), np.zeros(n))
        _same_cloud(lio.ctx.color_map_export_cloud(opts=_copts(0, True)), ck.export(reg, 0, -1, 0, True))
        s1 = lio.ctx.arm_stats()
        assert s1["cancelled"] + s1["expired"] > s0["cancelled"] + s0["expired"] and s1["fired"] == s0["fired"]      # (left by itself if the host was slow)
        solve()
        assert np.array_equal(solve.state, ref[0]) and np.array_equal(lio.eskf_get_state(), ref[1]) and np.array_equal(lio.eskf_get_cov(), ref[2])
    finally:
        lio.ctx.set_armed_launch(1)
        lio.close()
