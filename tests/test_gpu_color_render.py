"""Rendering an image into the colour voxel map on the device (srl_color_image_upload / srl_color_map_render /
srl_color_map_download_rgb / srl_color_registered_rgb: rgbMapTracker::renderPointsInRecentVoxel, rgbMapTracker.cpp:176-237) against the
sequential restatement of tests/render_checker.py -- which tests/test_render_checker_reference.py pins to the reference's own
translation units -- and against the recorded states of tests/golden/golden_color_render.npz.

Every comparison is bit for bit, through the C-ABI: the per-point state (rgb, N_rgb, cov_rgb, observe_distance, last_observe_time) in
both download orders, and the totals of every call."""
import ctypes as C
import os

import numpy as np
import pytest

import color_checker as cc
import render_checker as rk
import sr_livo_amd as srl
from sr_livo_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRL_ERR_BAD_ARG, SRL_ERR_UNSUPPORTED, SRL_ERR_NO_MAP, SRL_ERR_NO_SWEEP = -3, -4, -5, -6      # include/srlivo_hip.h: srl_status




def _cam(c):
    return capi.ColorCamera((C.c_double * 4)(*c.q), (C.c_double * 3)(*c.t), c.fx, c.fy, c.cx, c.cy, c.fov_margin)


def _ctx():
    ctx = srl.Context(0)
    o = rk.OPT
    ctx.color_map_create(capi.default_color_opts(size_voxel_map=o[0], max_num_points_in_voxel=o[1], min_distance_points=o[2], add_point_step=o[3]))
    return ctx


def _scene_ctx():
    """a device map holding the scene; the visited list of every insertion as the device returned it"""
    ctx = _ctx()
    visited = [ctx.color_map_insert(cc.scene_batch(j), rk.BATCH_TIMES[j], 0.0)[2] for j in range(3)]
    return ctx, visited


def _totals(t):
    return t.as_tuple()


def _want_totals(d):
    return tuple(d[name] for name in rk.TOTALS)


def _same_state(ctx, checker, what=""):
    """both download orders against the checker"""
    got_map, got_reg = ctx.color_map_download_rgb(), ctx.color_registered_rgb()
    want_map, want_reg = checker.map_state(), checker.registered_state()
    for name, g, w in zip(("rgb", "n_rgb", "cov_rgb", "observe_distance", "last_observe_time"), got_map, want_map):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, "map order", name, np.flatnonzero((g != w).reshape(len(g), -1).any(1))[:8])
    for name, g, w in zip(("rgb", "n_rgb", "cov_rgb", "observe_distance", "last_observe_time"), got_reg, want_reg):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, "registered order", name)
    return got_map, got_reg


def _render(ctx, checker, cam, which, voxels, obs_time, upload=True):
    if upload:
        ctx.color_image_upload(rk.scene_image(which))
    got = ctx.color_map_render(_cam(cam), voxels, obs_time)
    want = checker.render(cam, rk.scene_image(which), voxels, obs_time)
    assert _totals(got) == _want_totals(want), (_totals(got), want)
    return got


@pytest.fixture(scope="module")
def golden_render():
    return rk.golden_unpack(np.load(os.path.join(ROOT, "tests", "golden", "golden_color_render.npz"), allow_pickle=False))


def _run_sequence(ctx, visited):
    """the scene's renders on the device: totals and the raw bytes of both downloads after every render"""
    out = []
    for k in range(len(rk.RENDERS)):
        cam, which, obs_time, voxels = rk.render_call(k, visited)
        ctx.color_image_upload(rk.scene_image(which))                     # the two sizes alternate: the image buffer is re-used and re-shaped
        tot = ctx.color_map_render(_cam(cam), voxels, obs_time)
        out.append((_totals(tot), ctx.color_map_download_rgb(), ctx.color_registered_rgb()))
    return out


# ------------------------------------------------------------------------------------------------ 1. the sequence
def test_the_sequence_equals_the_restatement_and_the_golden_in_both_orders(golden_render):
    _, w_totals, w_map, w_reg = rk.scene_sequence()
    g_totals, g_map = golden_render
    chk_map, chk_visited = rk.scene_map()
    ctx, visited = _scene_ctx()
    try:
        for a, b in zip(visited, chk_visited):
            assert np.array_equal(a, b)
        # a map never rendered: zeros, without an allocation
        assert not any(a.any() for a in ctx.color_map_download_rgb()) and not any(a.any() for a in ctx.color_registered_rgb())
        got = _run_sequence(ctx, visited)
        for k, (tot, m, r) in enumerate(got):
            assert tot == _want_totals(w_totals[k]) == g_totals[k], (k, tot, w_totals[k])
            assert rk.state_bytes(m) == rk.state_bytes(w_map[k]), k
            assert rk.state_bytes(m) == rk.state_bytes(g_map[k]), k
            assert rk.state_bytes(r) == rk.state_bytes(w_reg[k]), k
        # a window of the registered list
        part = ctx.color_registered_rgb(11, 5)
        assert rk.state_bytes(part) == rk.state_bytes([a[11:16] for a in got[-1][2]])
        # rendering touched nothing of the map itself
        keys, counts, times, xyz, pidx = ctx.color_map_download()
        w = chk_map.map_arrays()
        assert np.array_equal(keys, w[0]) and np.array_equal(counts, w[1]) and times.tobytes() == w[2].tobytes()
        assert xyz.tobytes() == w[3].tobytes() and np.array_equal(pidx, w[4])
    finally:
        ctx.close()


def test_two_runs_give_the_same_bits():
    runs = []
    for _ in range(2):
        ctx, visited = _scene_ctx()
        try:
            runs.append(_run_sequence(ctx, visited))
        finally:
            ctx.close()
    for (ta, ma, ra), (tb, mb, rb) in zip(*runs):
        assert ta == tb and rk.state_bytes(ma) == rk.state_bytes(mb) and rk.state_bytes(ra) == rk.state_bytes(rb)


# ------------------------------------------------------------------------------------------------ 2. repeats, duplicates, empty and unknown
def _small_map():
    """a fresh checker + device map of the scene's first batch, and its visited list"""
    chk = cc.ColorChecker(*rk.OPT)
    ctx = _ctx()
    pts = cc.scene_batch(0)
    visited = ctx.color_map_insert(pts, 1.0, 0.0)[2]
    assert np.array_equal(visited, chk.insert(pts, 1.0, 0.0)[2])
    return ctx, chk, visited


def test_a_repeated_render_runs_the_update_again_with_a_zero_time_step():
    ctx, chk, visited = _small_map()
    try:
        rc = rk.RenderChecker(chk)
        cam = rk.scene_camera(rk.POSES[0], 0)
        first = _render(ctx, rc, cam, 0, visited, 5.0)
        again = _render(ctx, rc, cam, 0, visited, 5.0, upload=False)
        assert first.first > 100 and again.first == 0 and again.updated == first.first + first.updated
        _same_state(ctx, rc)
    finally:
        ctx.close()


def test_a_list_with_duplicates_equals_the_list_rendered_entry_by_entry():
    ctx, chk, visited = _small_map()
    ctx2 = _ctx()
    try:
        ctx2.color_map_insert(cc.scene_batch(0), 1.0, 0.0)
        rng = np.random.default_rng(5)
        voxels = visited[rng.integers(0, 400, 240)]                        # 240 entries out of 400 voxels: many named twice or more
        assert len({tuple(v) for v in voxels}) < 200
        rc = rk.RenderChecker(chk)
        cam = rk.scene_camera(rk.POSES[0], 0)
        ctx.color_image_upload(rk.scene_image(0)); ctx2.color_image_upload(rk.scene_image(0))
        for cx in (ctx, ctx2):                                             # a first observation from farther away, so that the repeats update
            cx.color_map_render(_cam(rk.scene_camera(rk.POSES[0], 0)), visited[:400], 4.0)
        rc.render(cam, rk.scene_image(0), visited[:400], 4.0)
        whole = _render(ctx, rc, cam, 0, voxels, 5.0, upload=False)
        parts = np.zeros(7, np.int64)
        for v in voxels:
            parts += np.array(_totals(ctx2.color_map_render(_cam(cam), v[None, :], 5.0)))
        assert tuple(int(p) for p in parts) == _totals(whole) and whole.updated > 100
        assert rk.state_bytes(ctx.color_map_download_rgb()) == rk.state_bytes(ctx2.color_map_download_rgb())
        _same_state(ctx, rc)
    finally:
        ctx.close(); ctx2.close()


def test_an_empty_list_and_an_unknown_key_change_nothing():
    ctx, chk, visited = _small_map()
    try:
        rc = rk.RenderChecker(chk)
        cam = rk.scene_camera(rk.POSES[0], 0)
        _render(ctx, rc, cam, 0, visited, 5.0)
        before = rk.state_bytes(ctx.color_map_download_rgb())
        assert _totals(ctx.color_map_render(_cam(cam), np.zeros((0, 3), np.int32), 6.0)) == (0,) * 7
        unknown = np.array([[30000, 30000, 30000], [100000, 0, 0], [-30000, 5, 5]], np.int32)     # absent; outside a voxel's 16 bits; absent
        assert all(tuple(k) not in chk.voxels for k in unknown.tolist())
        tot = ctx.color_map_render(_cam(cam), unknown, 6.0)
        assert _totals(tot) == (0, 0, 0, 0, 0, 0, 3)
        assert rk.state_bytes(ctx.color_map_download_rgb()) == before
        # ... and beside known ones it is counted and otherwise ignored
        mixed = np.concatenate([unknown[:1], visited[:50], unknown[1:]])
        got = _render(ctx, rc, cam, 0, mixed, 6.0, upload=False)
        assert got.unknown == 3 and got.listed > 0
        _same_state(ctx, rc)
    finally:
        ctx.close()


def test_refusals_on_a_device():
    ctx = srl.Context(0)
    try:
        cam = _cam(rk.scene_camera(rk.POSES[0], 0))
        one = np.zeros((1, 3), np.int32)
        lib = ctx.lib
        img = rk.scene_image(0)
        assert lib.srl_color_image_upload(ctx.h, capi._ptr(img), img.shape[0], img.shape[1], img.strides[0]) == SRL_ERR_NO_MAP
        assert lib.srl_color_map_render(ctx.h, C.byref(cam), capi._ptr(one), 1, 1.0, None) == SRL_ERR_NO_MAP
        assert lib.srl_color_map_download_rgb(ctx.h, None, None, None, None, None, 0) == SRL_ERR_NO_MAP
        assert lib.srl_color_registered_rgb(ctx.h, 0, 0, None, None, None, None, None) == SRL_ERR_NO_MAP
        ctx.color_map_create()
        assert lib.srl_color_map_render(ctx.h, C.byref(cam), capi._ptr(one), 1, 1.0, None) == SRL_ERR_NO_SWEEP      # no image yet
        assert lib.srl_color_image_upload(ctx.h, capi._ptr(img), img.shape[0], img.shape[1], img.shape[1] * 3 - 1) == SRL_ERR_BAD_ARG
        assert lib.srl_color_image_upload(ctx.h, capi._ptr(img), 1, img.shape[1], img.strides[0]) == SRL_ERR_BAD_ARG
        ctx.color_image_upload(img)
        tot = capi.ColorRenderTotals(7, 7, 7, 7, 7, 7, 7)
        assert lib.srl_color_map_render(ctx.h, C.byref(cam), capi._ptr(one), -1, 1.0, C.byref(tot)) == SRL_ERR_BAD_ARG and tot.as_tuple() == (0,) * 7
        assert lib.srl_color_map_render(ctx.h, C.byref(cam), None, 1, 1.0, None) == SRL_ERR_BAD_ARG
        assert lib.srl_color_map_render(ctx.h, None, capi._ptr(one), 1, 1.0, None) == SRL_ERR_BAD_ARG
        assert lib.srl_color_map_render(ctx.h, C.byref(cam), capi._ptr(one), 1, float("nan"), None) == SRL_ERR_BAD_ARG
        for field, value in (("fov_margin", 0.0), ("fov_margin", -0.01), ("fx", float("inf"))):
            bad = _cam(rk.scene_camera(rk.POSES[0], 0))
            setattr(bad, field, value)
            assert lib.srl_color_map_render(ctx.h, C.byref(bad), capi._ptr(one), 1, 1.0, None) == SRL_ERR_BAD_ARG
        bad = _cam(rk.scene_camera(rk.POSES[0], 0))
        bad.q_world_camera[2] = float("nan")
        assert lib.srl_color_map_render(ctx.h, C.byref(bad), capi._ptr(one), 1, 1.0, None) == SRL_ERR_BAD_ARG
        assert lib.srl_color_map_render(ctx.h, C.byref(cam), None, 0, 1.0, C.byref(tot)) == capi.SRL_OK and tot.as_tuple() == (0,) * 7
        # an empty map: every key is unknown
        assert _totals(ctx.color_map_render(cam, one, 1.0)) == (0, 0, 0, 0, 0, 0, 1)
        # one voxel named more often than a mark word counts: refused, nothing rendered
        ctx.color_map_insert(np.array([[0.05, 0.05, 0.05]]), 1.0, 0.0)
        many = np.zeros((70000, 3), np.int32)
        assert lib.srl_color_map_render(ctx.h, C.byref(cam), capi._ptr(many), len(many), 1.0, None) == SRL_ERR_UNSUPPORTED
        assert not any(a.any() for a in ctx.color_map_download_rgb())
        assert _totals(ctx.color_map_render(cam, many[:3], 1.0))[0] == 3   # ... and the next call is a normal one
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 3. growth, rebuilds, another image size
def test_state_survives_pool_growth_a_table_rebuild_and_another_image_size():
    chk = cc.ColorChecker(*rk.OPT)
    rc = rk.RenderChecker(chk)
    ctx = _ctx()
    try:
        first = cc.scene_batch(0)[:1500]
        v0 = ctx.color_map_insert(first, 1.0, 0.0)[2]
        assert np.array_equal(v0, chk.insert(first, 1.0, 0.0)[2])
        cam_a, cam_b = rk.scene_camera(rk.POSES[0], 0), rk.scene_camera(rk.POSES[1], 1)
        _render(ctx, rc, cam_a, 0, v0, 5.0)
        _same_state(ctx, rc, "before growth")
        size0, rebuilds0 = ctx.color_map_size(), ctx.color_map_rebuilds()
        lists = [v0]
        for j in range(3):                                                 # the pool starts at 4 096 records, the voxel table at 8 192 slots
            pts = cc.scene_batch(j)
            v = ctx.color_map_insert(pts, 2.0 + j, 0.0)[2]
            assert np.array_equal(v, chk.insert(pts, 2.0 + j, 0.0)[2])
            lists.append(v)
            _same_state(ctx, rc, f"after insertion {j}")                   # the new points are as reset() leaves them, the old keep their state
            ctx.color_image_upload(rk.scene_image(j % 2))                  # an image of another size in between, never rendered ...
            _render(ctx, rc, cam_b if j % 2 == 0 else cam_a, 1 - j % 2, np.concatenate(lists), 6.0 + j)      # ... and the other one rendered
            _same_state(ctx, rc, f"after render {j}")
        size1, rebuilds1 = ctx.color_map_size(), ctx.color_map_rebuilds()
        assert size0[0] < 4096 < size1[0] and rebuilds1[0] > rebuilds0[0] and rebuilds1[1] > rebuilds0[1]
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 4. the insertion is not disturbed
def test_insertions_with_renders_in_between_equal_insertions_alone():
    chk = cc.ColorChecker(*rk.OPT)
    ctx = _ctx()
    try:
        lists = []
        for j in range(3):
            pts = cc.scene_batch(j)
            outcome, stored, visited, tot = ctx.color_map_insert(pts, rk.BATCH_TIMES[j], 0.0)
            w_outcome, w_stored, w_visited = chk.insert(pts, rk.BATCH_TIMES[j], 0.0)
            assert np.array_equal(outcome, w_outcome) and stored.tobytes() == w_stored.tobytes() and np.array_equal(visited, w_visited)
            assert ctx.color_map_size() == chk.sizes()
            lists.append(visited)
            ctx.color_image_upload(rk.scene_image(j % 2))
            ctx.color_map_render(_cam(rk.scene_camera(rk.POSES[j], j % 2)), np.concatenate(lists), 10.0 + j)
        keys, counts, times, xyz, pidx = ctx.color_map_download()
        w = chk.map_arrays()
        assert np.array_equal(keys, w[0]) and np.array_equal(counts, w[1]) and times.tobytes() == w[2].tobytes()
        assert xyz.tobytes() == w[3].tobytes() and np.array_equal(pidx, w[4])
        reg = ctx.color_registered_download()
        rx, rkeys, rs = chk.registered_arrays()
        assert np.stack([reg["x"], reg["y"], reg["z"]], 1).tobytes() == rx.tobytes() and np.array_equal(reg["slot"].astype(np.int32), rs)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 5. the host mirror
def test_the_mirrors_method_gives_the_state_of_the_c_calls():
    lio = srl.Lio(0)
    ctx = _ctx()
    try:
        o = rk.OPT
        lio.set_color_map_options(capi.default_color_opts(size_voxel_map=o[0], max_num_points_in_voxel=o[1], min_distance_points=o[2], add_point_step=o[3]))
        lio.set_color_times(time_last_process=0.0)
        cam = rk.scene_camera(rk.POSES[0], 0)
        for j in range(2):
            pts = cc.scene_batch(j)
            lio.add_points_to_map_at(pts, rk.BATCH_TIMES[j], to_rendering=(j == 1))      # false, then true: the list of both sweeps moves over
            ctx.color_map_insert(pts, rk.BATCH_TIMES[j], 0.0)
        voxels, _ = lio.color_visited(1)                                   # voxels_recent_visited
        assert len(voxels) > 1000
        lio.ctx.color_image_upload(rk.scene_image(0)); ctx.color_image_upload(rk.scene_image(0))
        for t in (5.0, 5.2):
            a = lio.render_points_in_recent_voxel(_cam(cam), t)
            b = ctx.color_map_render(_cam(cam), voxels, t)
            assert _totals(a) == _totals(b) and a.listed > 0
        assert rk.state_bytes(lio.ctx.color_map_download_rgb()) == rk.state_bytes(ctx.color_map_download_rgb())
        assert rk.state_bytes(lio.ctx.color_registered_rgb()) == rk.state_bytes(ctx.color_registered_rgb())
        assert np.array_equal(lio.color_visited(1)[0], voxels)              # the lists are the caller's: not consumed
    finally:
        ctx.close(); lio.close()


# ------------------------------------------------------------------------------------------------ 6. armed launches
class _EskfAdapter:
    def __init__(self, lio): self.lio = lio
    def set_noise(self, *a): self.lio.eskf_set_noise(*a)
    def scale_init_cov(self): self.lio.eskf_scale_init_cov()
    def init_imu(self, a, g): self.lio.eskf_init_imu(a, g)
    def predict(self, dt, a, g): self.lio.eskf_predict(dt, a, g)
    def get_state(self): return self.lio.eskf_get_state()
    def set_state(self, s): self.lio.eskf_set_state(s)


def test_a_render_cancels_an_armed_launch_and_the_next_solve_is_unchanged():
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
        # a colour map beside the LiDAR map, rendered between two solves
        lio.ctx.color_map_create()
        pts = cc.scene_batch(0)
        visited = lio.ctx.color_map_insert(pts, 1.0, 0.0)[2]
        chk = cc.ColorChecker(*rk.OPT); chk.insert(pts, 1.0, 0.0)
        rc = rk.RenderChecker(chk)
        cam = rk.scene_camera(rk.POSES[0], 0)
        lio.ctx.color_image_upload(rk.scene_image(0))
        lio.ctx.set_armed_launch(2)                                        # a launch armed behind every eligible pass
        solve()
        s0 = lio.ctx.arm_stats()
        assert s0["armed"] > 0
        _render(lio.ctx, rc, cam, 0, visited, 5.0, upload=False)          # the launch waiting behind the solve's last pass is cancelled
        s1 = lio.ctx.arm_stats()
        assert s1["cancelled"] + s1["expired"] > s0["cancelled"] + s0["expired"] and s1["fired"] == s0["fired"]      # (left by itself if the host was slow)
        solve()
        assert np.array_equal(solve.state, ref[0]) and np.array_equal(lio.eskf_get_state(), ref[1]) and np.array_equal(lio.eskf_get_cov(), ref[2])
        lio.ctx.color_image_upload(rk.scene_image(1))                      # the upload cancels one too
        s2 = lio.ctx.arm_stats()
        assert s2["cancelled"] + s2["expired"] > s1["cancelled"] + s1["expired"]
        solve()
        assert np.array_equal(solve.state, ref[0])
        _same_state(lio.ctx, rc)
    finally:
        lio.ctx.set_armed_launch(1)
        lio.close()
