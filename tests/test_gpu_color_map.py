"""The colour voxel map on the device (srl_color_map_*: addPointToColorMap, lioOptimization.cpp:448-518, as addPointsToMap calls it at
:538-539) against the sequential restatement of tests/color_checker.py -- which tests/test_color_checker_reference.py pins to the
reference's own translation units -- and against the recorded results of tests/golden/golden_color_map.npz.

Every comparison is bit for bit and in order: outcome bytes, stored records (position, voxel, slot, batch index, point_index), the
visited list, and the downloads (the map in creation order with the points in slot order, the registered list, the sizes)."""
import os

import numpy as np
import pytest

import color_checker as cc
import sr_livo_amd as srl
from sr_livo_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRL_ERR_BAD_ARG, SRL_ERR_NO_MAP, SRL_ERR_NO_SWEEP = -3, -5, -6      # include/srlivo_hip.h: srl_status


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_records(got, want):
    assert got.dtype == capi.COLOR_STORED_DTYPE == cc.STORED_DTYPE
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)[:8]


def _check_insert(ctx, chk, pts, tse, tlp=0.0, call=None):
    """one insertion on the device and in the checker: everything the call returns"""
    before = ctx.color_map_size()
    outcome, stored, visited, tot = call() if call else ctx.color_map_insert(pts, tse, tlp)
    w_outcome, w_stored, w_visited = chk.insert(pts, tse, tlp)
    assert np.array_equal(outcome, w_outcome), np.flatnonzero(outcome != w_outcome)[:8]
    _same_records(stored, w_stored)
    assert visited.dtype == np.int32 and np.array_equal(visited, w_visited)
    assert (tot.stored, tot.registered, tot.visited) == (len(w_stored), int((w_stored["point_index"] >= 0).sum()), len(w_visited))
    assert tot.created == int(((w_outcome >> 1) & 1).sum())
    after = ctx.color_map_size()
    assert after == chk.sizes()
    assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (tot.stored, tot.created, tot.registered)
    return outcome, stored, visited


def _check_downloads(ctx, chk):
    keys, counts, times, xyz, pidx = ctx.color_map_download()
    w = chk.map_arrays()
    assert np.array_equal(keys, w[0]) and np.array_equal(counts, w[1])
    assert times.tobytes() == w[2].tobytes()
    assert np.array_equal(_bits(xyz), _bits(w[3])) and np.array_equal(pidx, w[4])
    reg = ctx.color_registered_download()
    rx, rk, rs = chk.registered_arrays()
    assert np.array_equal(_bits(np.stack([reg["x"], reg["y"], reg["z"]], 1)), _bits(rx))
    assert np.array_equal(np.stack([reg["kx"], reg["ky"], reg["kz"]], 1), rk) and np.array_equal(reg["slot"].astype(np.int32), rs)
    assert np.array_equal(reg["point_index"], np.arange(len(reg)))
    if len(reg) > 10:          # a window of the list
        part = ctx.color_registered_download(7, 3)
        assert part.tobytes() == reg[7:10].tobytes()
    return keys, counts, times, xyz, pidx, reg


def _ctx(opt):
    ctx = srl.Context(0)
    ctx.color_map_create(capi.default_color_opts(size_voxel_map=opt[0], max_num_points_in_voxel=opt[1], min_distance_points=opt[2], add_point_step=opt[3]))
    return ctx


@pytest.fixture(scope="module")
def golden_color():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "golden_color_map.npz"), allow_pickle=False))


# ------------------------------------------------------------------------------------------------ 1. three batches x four option sets
@pytest.mark.parametrize("o", range(len(cc.OPTION_SETS)))
def test_three_batches_equal_the_restatement_and_the_golden(o, golden_color):
    opt = cc.OPTION_SETS[o]
    ctx, chk = _ctx(opt), cc.ColorChecker(*opt)
    try:
        t = 1.0
        for j in range(3):
            pts = cc.scene_batch(j)
            outcome, stored, visited = _check_insert(ctx, chk, pts, t)
            t += 1.0 + j           # (the harness of the reference pin stamps batches with 1 + LiDAR voxels: any increasing times do)
            assert np.array_equal(outcome, golden_color[f"o{o}_b{j}_outcome"])
            assert np.array_equal(visited.astype(np.int16), golden_color[f"o{o}_b{j}_visited"]) and np.abs(visited).max() < 32768
            assert np.array_equal(stored["batch_index"], golden_color[f"o{o}_b{j}_batch_index"])
            assert np.array_equal(stored["point_index"], golden_color[f"o{o}_b{j}_point_index"])
            assert np.array_equal(stored["slot"].astype(np.uint8), golden_color[f"o{o}_b{j}_slot"])
            assert np.array_equal(np.stack([stored["kx"], stored["ky"], stored["kz"]], 1), golden_color[f"o{o}_b{j}_keys"])
            # the positions are the FP32 roundings of the inputs: no more to record
            assert np.array_equal(_bits(np.stack([stored["x"], stored["y"], stored["z"]], 1)), _bits(pts[stored["batch_index"]].astype(np.float32)))
        _check_downloads(ctx, chk)
        assert ctx.color_map_size() == tuple(int(v) for v in golden_color[f"o{o}_sizes"])
        # the branches the scene is there to reach (the alias box sits one wrap of the 0.01 m grid away: 655.36 m)
        assert min(chk.n_refused_full, chk.n_stored_not_registered, chk.n_created, chk.n_retouched) > 0
        if opt[2] == 0.01:
            assert min(chk.n_stored_not_registered_other_voxel, chk.n_registered_after_unstored) > 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 2. the time rule
def test_equal_times_and_time_last_process():
    opt = cc.OPTION_SETS[0]
    ctx, chk = _ctx(opt), cc.ColorChecker(*opt)
    try:
        a, b, c = (cc.scene_batch(j)[:5000] for j in range(3))
        _, _, v0 = _check_insert(ctx, chk, a, 7.0)
        _, _, v1 = _check_insert(ctx, chk, b, 7.0)                   # the same sweep time: re-touched voxels are not listed again
        assert len(v0) and len(v1)
        assert not (set(map(tuple, v0)) & set(map(tuple, v1)))
        _, _, v2 = _check_insert(ctx, chk, c, 7.0 + 5e-6)             # within 1e-5 of the stamp: still the same time for stamped voxels
        _, _, v3 = _check_insert(ctx, chk, a, 9.0, 9.0 + 9e-6)        # |time_sweep_end - time_last_process| <= 1e-5: nothing is listed or stamped
        assert len(v3) == 0
        _, _, v4 = _check_insert(ctx, chk, a, 9.0, 0.0)               # ... so the same time lists them afterwards
        assert len(v4) > 0
        _, _, v5 = _check_insert(ctx, chk, b, 8.0, -1e5)              # an EARLIER time is a different time
        assert len(v5) > 0 and len(v2) < len(cc.ColorChecker(*opt).insert(c, 7.0 + 5e-6)[2])
        _check_downloads(ctx, chk)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 3. the points srl_frame_commit left in HBM
def test_null_points_take_the_committed_frame():
    opt = cc.OPTION_SETS[0]
    a, b = _ctx(opt), _ctx(opt)
    chk = cc.ColorChecker(*opt)
    try:
        assert a.lib.srl_color_map_insert(a.h, None, 0, 1.0, 0.0, None, None, 0, None, 0, None) == SRL_ERR_BAD_ARG      # no frame was ever committed
        q = synth.quat_from_rotvec([0.01, -0.02, 0.3])
        t = np.array([0.4, -0.2, 0.1])
        for j in range(2):
            raw = cc.scene_batch(j)
            a.frame_upload(raw)
            world, _ = a.frame_commit(q, t, voxel_size=1.0)
            got = _check_insert(a, chk, world, 2.0 + j, call=lambda: a.color_map_insert(None, 2.0 + j, 0.0))
            host = b.color_map_insert(world, 2.0 + j, 0.0)
            assert np.array_equal(got[0], host[0]) and got[1].tobytes() == host[1].tobytes() and np.array_equal(got[2], host[2])
        for x, y in zip(a.color_map_download(), b.color_map_download()):
            assert x.tobytes() == y.tobytes()
        a.frame_upload(cc.scene_batch(2))                               # a newer frame, not committed
        assert a.lib.srl_color_map_insert(a.h, None, 0, 5.0, 0.0, None, None, 0, None, 0, None) == SRL_ERR_NO_SWEEP
        assert a.color_map_size() == chk.sizes()
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 4. edges
def test_no_points_one_point_and_refused_arguments():
    ctx = srl.Context(0)
    try:
        pts = cc.scene_batch(0)[:16]
        assert ctx.lib.srl_color_map_insert(ctx.h, capi._ptr(pts), 16, 1.0, 0.0, None, None, 0, None, 0, None) == SRL_ERR_NO_MAP
        assert ctx.lib.srl_color_map_size(ctx.h, None, None, None, None) == SRL_ERR_NO_MAP
        for bad in (dict(size_voxel_map=0.0), dict(size_voxel_map=float("nan")), dict(min_distance_points=-0.01), dict(min_distance_points=float("inf")),
                    dict(max_num_points_in_voxel=0), dict(max_num_points_in_voxel=256), dict(add_point_step=0)):
            o = capi.default_color_opts(**bad)
            assert ctx.lib.srl_color_map_create(ctx.h, o) == SRL_ERR_BAD_ARG, bad
        assert ctx.lib.srl_color_map_create(ctx.h, None) == SRL_ERR_BAD_ARG
        opt = (0.1, 255, 0.01, 1)
        ctx.color_map_create(capi.default_color_opts(max_num_points_in_voxel=255))
        assert ctx.lib.srl_color_map_create(ctx.h, capi.default_color_opts()) == SRL_ERR_BAD_ARG      # the options hold for the map's life
        chk = cc.ColorChecker(*opt)
        tot = capi.ColorTotals(9, 9, 9, 9)
        assert ctx.lib.srl_color_map_insert(ctx.h, capi._ptr(pts), 0, 1.0, 0.0, None, None, 0, None, 0, tot) == 0
        assert (tot.stored, tot.created, tot.registered, tot.visited) == (0, 0, 0, 0) and ctx.color_map_size() == (0, 0, 0, 0)
        assert ctx.lib.srl_color_map_insert(ctx.h, capi._ptr(pts), -1, 1.0, 0.0, None, None, 0, None, 0, None) == SRL_ERR_BAD_ARG
        rec = np.zeros(16, capi.COLOR_STORED_DTYPE)
        assert ctx.lib.srl_color_map_insert(ctx.h, capi._ptr(pts), 16, 1.0, 0.0, None, capi._ptr(rec), 15, None, 0, None) == SRL_ERR_BAD_ARG
        assert ctx.color_map_size() == (0, 0, 0, 0)
        _check_insert(ctx, chk, pts[:1], 1.0)
        _check_insert(ctx, chk, pts[:1], 1.0)                           # the same point again: stored, not registered, not listed
        _check_insert(ctx, chk, pts, 2.0)
        out = ctx.color_map_insert(pts, 3.0, want_outcome=False, want_stored=False, want_visited=False)     # every output optional
        chk.insert(pts, 3.0)
        assert out[:3] == (None, None, None) and out[3].stored == 16
        _check_downloads(ctx, chk)
        ctx.comm_set_host_callbacks(2, 0, lambda a: None, lambda v: [v, v])       # more than one rank: refused, nothing inserted
        assert ctx.lib.srl_color_map_insert(ctx.h, capi._ptr(pts), 16, 4.0, 0.0, None, None, 0, None, 0, None) == capi.SRL_ERR_UNSUPPORTED
        ctx.comm_set_host_callbacks(1, 0, None, None)
        assert ctx.color_map_size() == chk.sizes()
        ctx.color_map_destroy()
        assert ctx.lib.srl_color_map_size(ctx.h, None, None, None, None) == SRL_ERR_NO_MAP
        ctx.color_map_create()                                          # a new map starts empty
        assert ctx.color_map_size() == (0, 0, 0, 0)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 5. a frame beyond the one-launch scans and sorts
def test_a_frame_of_262144_points():
    rng = np.random.default_rng(9200)
    n = 262_144
    pts = np.stack([rng.uniform(-30, 30, n), rng.uniform(-30, 30, n), -1.7 + 0.3 * rng.standard_normal(n)], 1)
    pts[: n // 8] = np.stack([rng.uniform(0, 3, n // 8), rng.uniform(0, 3, n // 8), rng.uniform(0, 0.05, n // 8)], 1)      # a dense slab: full voxels, shared grid cells
    pts = pts[rng.permutation(n)]
    for opt in ((0.25, 5, 0.05, 1), (0.1, 20, 0.01, 3)):
        ctx, chk = _ctx(opt), cc.ColorChecker(*opt)
        try:
            _check_insert(ctx, chk, pts, 1.0)
            _check_insert(ctx, chk, pts[::-1], 2.0)
            _check_downloads(ctx, chk)
            assert chk.n_refused_full > 0 and chk.n_stored_not_registered > 0
        finally:
            ctx.close()


# ------------------------------------------------------------------------------------------------ 6. a long run: both tables rebuild
def test_forty_five_batches_rebuild_both_tables_and_two_runs_agree():
    opt = cc.OPTION_SETS[0]
    chk = cc.ColorChecker(*opt)
    runs = []
    for run in range(2):
        ctx = _ctx(opt)
        try:
            log = []
            for j in range(45):
                pts = cc.scene_batch(j)
                if run == 0:
                    got = _check_insert(ctx, chk, pts, 1.0 + j)
                else:
                    got = ctx.color_map_insert(pts, 1.0 + j)[:3]
                log.append(b"".join(x.tobytes() for x in got))
            if run == 0:
                dl = _check_downloads(ctx, chk)
                vt, gt = ctx.color_map_rebuilds()
                assert vt >= 3 and gt >= 3, (vt, gt)
            else:
                dl = ctx.color_map_download() + (ctx.color_registered_download(),)
            runs.append((log, [x.tobytes() for x in dl], ctx.color_map_size()))
        finally:
            ctx.close()
    assert runs[0] == runs[1]


# ------------------------------------------------------------------------------------------------ 7. the LiDAR side does not notice
def test_the_lidar_side_is_bit_identical_with_a_colour_insertion_between_the_passes():
    cands, L = synth.map_candidates(9301, 120_000)
    sw = synth.make_sweep(9302, 8192, L)
    opts = srl.default_opts(max_num_residuals=2**31 - 1)
    rng = np.random.default_rng(9303)
    poses = [(synth.quat_mul(sw["q_gt"], synth.quat_from_rotvec(0.7 ** k * rng.normal(0, 0.004, 3))), sw["t_gt"] + 0.7 ** k * (sw["t_pred"] - sw["t_gt"]))
             for k in range(4)]
    results = []
    for with_colour in (False, True):
        ctx = srl.Context(0)
        try:
            if with_colour:
                ctx.color_map_create()
            ctx.map_insert(cands)
            ctx.sweep_upload(sw["raw"])
            ctx.set_taps(True)
            out = []
            for k, (q, t) in enumerate(poses):
                neq, _ = ctx.build_residuals(capi.make_frame(q, t, sw["t_last"]), opts)      # passes 1.. start from the bounds of the pass before
                ids, status, ncand = ctx.fetch_neighbors()
                res = ctx.fetch_residuals()
                out.append((bytes(neq), ids.tobytes(), status.tobytes(), ncand.tobytes(), b"".join(res[key].tobytes() for key in sorted(res))))
                if with_colour:
                    tot = ctx.color_map_insert(cc.scene_batch(k), 1.0 + k)[3]
                    assert tot.stored > 0
            out.append(tuple(x.tobytes() for x in ctx.map_download()))
            out.append(ctx.map_size())
            results.append(out)
        finally:
            ctx.close()
    assert results[0] == results[1]


# ------------------------------------------------------------------------------------------------ 8. the mirror's lists (lioOptimization.cpp:523-550)
def test_the_mirror_keeps_the_visited_lists_as_the_reference_does():
    opt = cc.OPTION_SETS[0]
    chk = cc.ColorChecker(*opt)
    lio = srl.Lio(0)
    try:
        lio.set_color_map_options()
        lio.set_color_times(time_last_process=0.0)
        temp, recent, new = [], np.zeros((0, 3), np.int32), 0
        kw = dict(voxel_size=1.0, cap=20, min_dist=0.1)
        for j, rendering in enumerate((False, False, True, False, True)):
            pts = cc.scene_batch(j)
            lio.add_points_to_map_at(pts, 1.0 + j, to_rendering=rendering, **kw)
            _, w_stored, w_visited = chk.insert(pts, 1.0 + j, 0.0)
            if rendering:
                temp = []
            before = sum(len(x) for x in temp)
            temp.append(w_visited)
            if rendering:
                recent, new = np.concatenate(temp), sum(len(x) for x in temp) - before
            got_temp, got_new = lio.color_visited(0)
            got_recent, _ = lio.color_visited(1)
            assert np.array_equal(got_temp, np.concatenate(temp)) and np.array_equal(got_recent, recent) and got_new == new
            _same_records(lio.color_stored(), w_stored)
        # the commit path: the colour insertion reads the frame's world points from HBM
        raw = cc.scene_batch(7)
        lio.ctx.frame_upload(raw)
        lio.set_color_times(time_last_process=0.0, commit_time_sweep_end=20.0, to_rendering=True)
        state = np.zeros(16); state[0] = 1.0
        world, _ = lio.commit_frame(state, **kw)
        assert np.array_equal(world, raw)
        _, w_stored, w_visited = chk.insert(raw, 20.0, 0.0)
        got_recent, got_new = lio.color_visited(1)
        assert np.array_equal(got_recent, w_visited) and got_new == len(w_visited)
        _same_records(lio.color_stored(), w_stored)
        assert lio.ctx.color_map_size() == chk.sizes()
    finally:
        lio.close()


def test_a_mirror_without_the_options_inserts_as_before():
    pts = cc.scene_batch(0)
    a, b = srl.Lio(0), srl.Lio(0)
    try:
        a.add_points_to_map(pts, voxel_size=1.0, cap=20, min_dist=0.1)
        b.add_points_to_map_at(pts, 3.0, to_rendering=True, voxel_size=1.0, cap=20, min_dist=0.1)
        for x, y in zip(a.ctx.map_download(), b.ctx.map_download()):
            assert x.tobytes() == y.tobytes()
        assert len(b.color_visited(0)[0]) == 0 and len(b.color_stored()) == 0
        assert b.lib.srl_color_map_size(b.ctx.h, None, None, None, None) == SRL_ERR_NO_MAP      # no colour map came into being
    finally:
        a.close(); b.close()
