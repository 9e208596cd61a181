"""The colour map's never-cleared device structures across the wraps of their numbers ("never cleared per call"):

  cm->scratch     srl_color_map_insert        16-bit epoch, 32-bit call counter
  cm->sel_cells   srl_color_map_select        epoch, counter; the companions minw, d_sel_last, d_sel_first hold 0xFFFFFFFF - counter
  cm->trk_pool    srl_color_map_track_update  epoch, counter (companion tag)
  cm->trk_cells   the same call               epoch, counter (companion tag)
  cm->d_mark      srl_color_map_render        16-bit render epoch

A structure is cleared only when its number wraps (an epoch behind 0xFFFF, a counter behind 0xFFFFFFFE, both to 1): once in 65 535 calls
at the earliest, so no test reaches a wrap by calling.  srl_debug_set_color_epochs moves the numbers next to their ends and
srl_debug_color_epochs reads them back; every sequence here has three phases -- calls on a fresh map that write the numbers 1 ... k into many
slots, the jump, and the calls across the wrap: two on the last numbers, the wrapping one, and at least k more that use 1 ... k again with
other content -- and asserts from the read-back that exactly one call took its number from its last value to 1.

What every call returns is compared byte for byte with the sequential checkers of tests/ (color_checker, render_checker, select_checker,
track_checker), which have no epochs.  Removing any one of the fills at a wrap (the epoch's or the counter's in srl_epoch_table_begin, the
selection's companions', the render's) makes a test of this file fail; the epoch's only shows on a table crossed twice
(test_insert_epoch_wraps_twice_on_the_smallest_table says why).  Also here: the render's limit of 65 535 occurrences of one voxel, at the
limit and beyond it."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import color_checker as cc
import render_checker as rk
import select_checker as sk
import track_checker as tk
import vio_checker as vc
import sr_livo_amd as srl
from sr_livo_amd import capi

pytestmark = pytest.mark.gpu
SRL_ERR_BAD_ARG, SRL_ERR_UNSUPPORTED, SRL_ERR_NO_MAP = -3, -4, -5            # include/srlivo_hip.h: srl_status
LAST = {"epoch": 0xFFFF, "counter": 0xFFFFFFFE}                              # the last value of a number of either family
FAMILIES = ("counter", "epoch")


def _cam(c):
    return capi.ColorCamera((C.c_double * 4)(*c.q), (C.c_double * 3)(*c.t), c.fx, c.fy, c.cx, c.cy, c.fov_margin)


def _ctx():
    ctx = srl.Context(0)
    o = rk.OPT
    ctx.color_map_create(capi.default_color_opts(size_voxel_map=o[0], max_num_points_in_voxel=o[1], min_distance_points=o[2], add_point_step=o[3]))
    return ctx


def _scene_ctx():
    """a device map holding the scene of the checkers (three insertions) and the visited list of every insertion"""
    ctx = _ctx()
    visited = [ctx.color_map_insert(cc.scene_batch(j), rk.BATCH_TIMES[j], 0.0)[2] for j in range(3)]
    return ctx, visited


def _jump(ctx, family, k=2):
    ctx.set_color_epochs(k if family == "epoch" else -1, k if family == "counter" else -1)


class _Watch:
    """the read-back around every call of a sequence: `names` are the numbers the calls under watch advance"""

    def __init__(self, ctx, names):
        self.ctx, self.names = ctx, tuple(names)
        self.last = tuple(LAST["epoch" if n.endswith("epoch") else "counter"] for n in self.names)
        self.crossings, self.calls_after = 0, 0

    def read(self):
        e = self.ctx.color_epochs()
        return tuple(e[n] for n in self.names)

    def call(self, fn, *a, **kw):
        before = self.read()
        out = fn(*a, **kw)
        after = self.read()
        if after == (1,) * len(self.names) and before != (0,) * len(self.names):      # (0: a structure never used)
            assert before == self.last, (self.names, before)             # the wrapping call: from the last value to 1
            self.crossings += 1
        else:
            assert after == tuple(b + 1 for b in before), (self.names, before, after)
            self.calls_after += 1 if self.crossings else 0
        return out

    def done(self, crossings=1, calls_after=0):
        assert self.crossings == crossings and self.calls_after >= calls_after, (self.names, self.crossings, self.calls_after)


# ------------------------------------------------------------------------------------------------ the hooks themselves
def test_the_hooks_read_back_move_forward_only_and_refuse_without_a_map():
    ctx = srl.Context(0)
    try:
        out = (C.c_uint32 * 9)()
        assert ctx.lib.srl_debug_color_epochs(ctx.h, out) == SRL_ERR_NO_MAP
        assert ctx.lib.srl_debug_set_color_epochs(ctx.h, 2, 2) == SRL_ERR_NO_MAP
        ctx.color_map_create()
        assert ctx.color_epochs() == dict.fromkeys(capi.Context.COLOR_EPOCHS, 0)
        assert ctx.lib.srl_debug_color_epochs(ctx.h, None) == SRL_ERR_BAD_ARG
        for bad in ((-2, -1), (-1, -2), (0x10000, -1)):
            assert ctx.lib.srl_debug_set_color_epochs(ctx.h, *bad) == SRL_ERR_BAD_ARG
        ctx.set_color_epochs(-1, -1)
        assert ctx.color_epochs() == dict.fromkeys(capi.Context.COLOR_EPOCHS, 0)
        ctx.set_color_epochs(5, -1)
        e = ctx.color_epochs()
        assert [e[n] for n in capi.Context.COLOR_EPOCHS] == [0xFFFA] * 4 + [0] * 4 + [0xFFFA]
        ctx.set_color_epochs(-1, 7)
        e = ctx.color_epochs()
        assert [e[n] for n in capi.Context.COLOR_EPOCHS] == [0xFFFA] * 4 + [0xFFFFFFF7] * 4 + [0xFFFA]
        # backward: refused, and nothing moves -- not even the family that could
        assert ctx.lib.srl_debug_set_color_epochs(ctx.h, 6, 3) == SRL_ERR_BAD_ARG
        assert ctx.lib.srl_debug_set_color_epochs(ctx.h, 3, 8) == SRL_ERR_BAD_ARG
        assert ctx.color_epochs() == e
        ctx.set_color_epochs(5, 7)                                         # where they are: not backward
        ctx.set_color_epochs(0, 0)
        e = ctx.color_epochs()
        assert [e[n] for n in capi.Context.COLOR_EPOCHS] == [0xFFFF] * 4 + [0xFFFFFFFE] * 4 + [0xFFFF]
        # one insertion moves the scratch table's numbers alone: the next call wraps
        ctx.color_map_insert(cc.scene_batch(0)[:100], 1.0, 0.0)
        e = ctx.color_epochs()
        assert (e["scratch_epoch"], e["scratch_counter"], e["select_epoch"], e["render_epoch"]) == (1, 1, 0xFFFF, 0xFFFF)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the render's mark words
def _render_lists(visited, groups):
    """the scene's visited lists split by voxel into `groups` disjoint lists (a voxel's group: its first occurrence, counted round robin);
    every list keeps the repeats of its voxels and names its first 300 entries twice more and the first 100 a fourth time"""
    entries = np.concatenate(visited)
    first = {}
    for e in entries.tolist():
        first.setdefault(tuple(e), len(first))
    group = np.array([first[tuple(e)] % groups for e in entries.tolist()])
    lists = []
    for g in range(groups):
        own = entries[group == g]
        lists.append(np.concatenate([own, own[:300], own[:300], own[:100]]))
    return lists


def test_render_epoch_wrap():
    """the mark words of lists A1, A2, A3 carry the epochs 1, 2, 3; behind the wrap the renders of epochs 1, 2, 3 name other voxels.  Without
    the fill at the wrap the voxels of A1 (A2, A3) would be rendered again, with the multiplicity they had"""
    chk, chk_visited = rk.scene_map()
    rc = rk.RenderChecker(chk)
    ctx, visited = _scene_ctx()
    try:
        for a, b in zip(visited, chk_visited):
            assert np.array_equal(a, b)
        lists = _render_lists(visited, 7)
        keys = [{tuple(e) for e in l.tolist()} for l in lists]
        assert all(not (keys[a] & keys[b]) for a in range(7) for b in range(a)) and min(len(k) for k in keys) > 2000
        watch = _Watch(ctx, ("render_epoch",))

        def render(call, which_list):
            cam, which, _, _ = rk.render_call(call % len(rk.RENDERS), visited)
            obs_time = 10.0 + 0.13 * call
            ctx.color_image_upload(rk.scene_image(which))
            got = watch.call(ctx.color_map_render, _cam(cam), lists[which_list], obs_time)
            want = rc.render(cam, rk.scene_image(which), lists[which_list], obs_time)
            assert got.as_tuple() == tuple(want[name] for name in rk.TOTALS), (call, got.as_tuple(), want)
            assert rk.state_bytes(ctx.color_map_download_rgb()) == rk.state_bytes(rc.map_state()), call
            return got

        for call in range(3):                                              # phase 1: epochs 1, 2, 3 on lists 0, 1, 2
            assert render(call, call).first > 500
        assert watch.read() == (3,)
        _jump(ctx, "epoch")
        assert watch.read() == (0xFFFD,)
        render(3, 3); render(4, 3)                                         # the last two epochs, away from lists 0, 1, 2
        assert watch.read() == (0xFFFF,)
        for call, stale, fresh in ((5, 0, 4), (6, 1, 5), (7, 2, 6)):       # epoch 1 (the wrapping call), 2, 3
            # from the checker alone: the voxels whose marks carry this epoch from phase 1 hold points this call's camera would colour
            probe = rk.RenderChecker(chk)
            probe.state = copy.deepcopy(rc.state)
            cam, which, _, _ = rk.render_call(call % len(rk.RENDERS), visited)
            would = probe.render(cam, rk.scene_image(which), lists[stale], 10.0 + 0.13 * call)
            assert would["first"] + would["updated"] > 500, (call, would)
            render(call, fresh)
            assert watch.read() == (call - 4,)
        assert rk.state_bytes(ctx.color_registered_rgb()) == rk.state_bytes(rc.registered_state())
        watch.done(calls_after=2)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the selection's image cells
def _select(ctx, cam, rows, cols, voxels, opts):
    """ONE call of srl_color_map_select with room for every candidate (the wrapper asks twice: first for the totals, then for the records)"""
    v = np.zeros((0, 3), np.int32) if voxels is None else np.ascontiguousarray(voxels, dtype=np.int32).reshape(-1, 3)
    out = np.zeros(max(len(v), ctx.color_map_size()[2]), dtype=capi.COLOR_SELECTED_DTYPE)
    tot = capi.ColorSelectTotals()
    ctx._chk(ctx.lib.srl_color_map_select(ctx.h, C.byref(_cam(cam)), int(rows), int(cols), capi._ptr(v) if len(v) else None, len(v), C.byref(opts),
                                          capi._ptr(out), len(out), C.byref(tot)), "srl_color_map_select")
    return out[:tot.selected].copy(), tot


def _same_selection(got, want, what):
    rec, tot = got
    assert tot.as_tuple() == sk.totals_tuple(want[1]), (what, tot.as_tuple(), want[1])
    assert rec.tobytes() == want[0].tobytes(), (what, np.flatnonzero(rec != want[0])[:8] if len(rec) == len(want[0]) else (len(rec), len(want[0])))


def _pow2(v):
    p = 1024
    while p < v:
        p <<= 1
    return p


# all-points mode: the camera of a render for either margin, in phase 1 (as select_checker.ALL_POINTS_CAMERAS) and behind the wrap
ALL_POINTS_PHASE_1, ALL_POINTS_PHASE_3 = (0, 1), (4, 3)


@functools.lru_cache(maxsize=None)
def _all_points_want(batches, k, m, s):
    """the checker's all-points selection of the scene after `batches` insertions: camera of render k, margin m, parameter set s"""
    cam, rows, cols, _ = sk.scene_camera(k, sk.MARGINS[m])
    md, skip = sk.PARAMETER_SETS[s]
    return sk.select_sequential(sk.scene_map(batches)[0], cam, rows, cols, None, md, skip, True)


@pytest.mark.parametrize("family", FAMILIES)
def test_select_wrap(family):
    """phase 1: the four parameter sets under both margins, on render 0's list and then on all points (numbers 1 ... 16).  Across the wrap
    minimum_dis goes 40, 0.4, 10 (the mask in use grows to the whole table and shrinks to an eighth of it); behind it the numbers 1 ... 16
    meet the same cell grids under the camera of render 4 (3 for the smaller image).  A further insertion then makes the table and its
    companions grow"""
    ctx, visited = _scene_ctx()
    try:
        smap, chk_visited = sk.scene_map()
        for a, b in zip(visited, chk_visited):
            assert np.array_equal(a, b)
        results = sk.sequence_results()
        watch = _Watch(ctx, ("select_" + family,))
        most_visited = [0]

        def run(cam, rows, cols, voxels, s, use_all, want, what):
            md, skip = sk.PARAMETER_SETS[s]
            o = capi.default_color_select_opts(minimum_dis=md, skip_step=skip, use_all_points=1 if use_all else 0, minimum_depth=sk.MINIMUM_DEPTH,
                                               maximum_depth=sk.MAXIMUM_DEPTH)
            got = watch.call(_select, ctx, cam, rows, cols, voxels, o)
            _same_selection(got, want, what)
            assert got[1].selected > 50
            return got

        def listed(k, s, m):
            cam, rows, cols, lists = sk.scene_camera(k, sk.MARGINS[m])
            got = run(cam, rows, cols, np.concatenate([visited[j] for j in lists]), s, False, results[sk.SEQUENCE.index((k, s, m))], (k, s, m))
            most_visited[0] = max(most_visited[0], got[1].visited)

        def all_points(batches, k, s, m):
            cam, rows, cols, _ = sk.scene_camera(k, sk.MARGINS[m])
            got = run(cam, rows, cols, None, s, True, _all_points_want(batches, k, m, s), ("all", batches, k, s, m))
            most_visited[0] = max(most_visited[0], got[1].visited) if batches == 3 else most_visited[0]
            return got

        sets = [(s, m) for s in range(len(sk.PARAMETER_SETS)) for m in range(len(sk.MARGINS))]
        assert [_all_points_want(3, k, m, 0)[0].tobytes() for m, k in enumerate(ALL_POINTS_PHASE_1)] == [r[0].tobytes() for r in sk.all_points_results(3)]
        for s, m in sets:                                                  # phase 1
            listed(0, s, m)
        for s, m in sets:
            all_points(3, ALL_POINTS_PHASE_1[m], s, m)
        assert watch.read() == (16,)
        _jump(ctx, family)
        assert watch.read() == (LAST[family] - 2,)
        assert [sk.PARAMETER_SETS[s][0] for s in (2, 3, 0)] == [40.0, 0.4, 10.0]
        listed(4, 2, 0)                                                    # minimum_dis 40
        listed(4, 3, 0)                                                    # 0.4: more cells than candidates, the whole table in use
        assert watch.read() == (LAST[family],)
        for s, m in sets:                                                  # 10 on the wrapping call; the numbers 1 ... 8 as in phase 1, another camera
            listed(4, s, m)
            assert watch.read() == (1 + sets.index((s, m)),)
        for s, m in sets:                                                  # 9 ... 16: phase 1's all-points grids from other poses
            all_points(3, ALL_POINTS_PHASE_3[m], s, m)
        assert watch.read() == (16,)
        # a further insertion: at minimum_dis 0.4 there are more cells than candidates, the table holds 2 x the registered points rounded up
        # to a power of two -- more than any call so far asked for: the table and its companions are allocated again
        more = ctx.color_map_insert(sk.extra_batch(), sk.EXTRA_BATCH_TIME, 0.0)[2]
        smap4, visited4 = sk.scene_map(4)
        assert np.array_equal(more, visited4[3])
        grown = all_points(4, 4, 3, 0)
        assert grown[1].visited == ctx.color_map_size()[2] and _pow2(2 * grown[1].visited) > _pow2(2 * most_visited[0])
        cam, rows, cols, _ = sk.scene_camera(0, 0.005)
        run(cam, rows, cols, more, 0, False, sk.select_sequential(smap4, cam, rows, cols, more), "after the growth")
        watch.done(calls_after=16)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the tracker's two tables
TRACK_PHASE_1 = ("narrow", "fill", "track1", "track2", "track3", "wall", "wide")          # the largest tables first: no later call re-allocates them
# two calls on the last numbers: no candidates, no tracked points (both tables still open a call); the wrapping call; then the numbers
# 2 ... 7 of phase 1 under other cameras, with other tracked sets and candidate lists ("among" on fill's cell grid, "both" on track1's with
# the candidates of two selections in a row, "full_negative" on track3's with its candidates reversed and nothing tracked)
TRACK_PHASE_3 = ("size_300_0", "size_0_257", "odd", "among", "both", "budget_more", "full_negative", "among_wide", "size_1_0", "size_0_1",
                 "budget_1", "size_64_257")


@pytest.mark.parametrize("family", FAMILIES)
def test_track_update_wrap(family):
    ctx, _ = _scene_ctx()
    try:
        assert ctx.color_map_size()[0] == len(tk.pool_positions())
        by_name = {c[0]: (c, r) for c, r in zip(tk.cases(), tk.case_results())}
        names = ("track_pool_" + family, "track_cell_" + family)
        watch = _Watch(ctx, names)

        def run(name):
            (_, k, margin, tracked, cand, md, maximum), want = by_name[name]
            cam, rows, cols, _ = sk.scene_camera(k, margin)
            rec, t_out, c_out, tot = watch.call(ctx.color_map_track_update, _cam(cam), rows, cols, tracked, cand,
                                                capi.default_color_track_opts(mini_distance=md, maximum_tracked_points=maximum))
            assert tot.as_tuple() == tk.totals_tuple(want[3]), (name, tot.as_tuple(), want[3])
            assert t_out.tobytes() == want[1].tobytes() and c_out.tobytes() == want[2].tobytes(), name
            assert rec.tobytes() == want[0].tobytes(), name

        # the sets and lists change from call to call, and those next to the wrap are the one-sided ones
        items = [len(by_name[n][0][3]) + len(by_name[n][0][4]) for n in TRACK_PHASE_1 + TRACK_PHASE_3]
        assert items[0] == max(items) and len(by_name["size_300_0"][0][4]) == 0 and len(by_name["size_0_257"][0][3]) == 0
        for name in TRACK_PHASE_1:
            run(name)
        assert watch.read() == (7, 7)
        _jump(ctx, family)
        assert watch.read() == (LAST[family] - 2,) * 2
        for n, name in enumerate(TRACK_PHASE_3):
            run(name)
            assert watch.read() == (((LAST[family] - 1, LAST[family]) + tuple(range(1, 20)))[n],) * 2
        watch.done(calls_after=7)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the insertion's scratch table
def _row_of_voxels(j, n=512):
    """n points in n voxels of their own, far from the scene: 2 n == 1024, the smallest table an insertion uses"""
    i = np.arange(n)
    return np.stack([100.0 + 0.1 * i + 0.05, np.full(n, 50.0 + 1.0 * j + 0.05), np.full(n, 3.05)], 1)


def _insert(ctx, chk, watch, pts, t):
    """one insertion on the device and in the checker: what the call returned, then the whole map through both downloads"""
    outcome, stored, visited, tot = watch.call(ctx.color_map_insert, pts, t, 0.0)
    w_outcome, w_stored, w_visited = chk.insert(pts, t, 0.0)
    assert outcome.tobytes() == w_outcome.tobytes() and stored.tobytes() == w_stored.tobytes() and np.array_equal(visited, w_visited), t
    assert (tot.stored, tot.created, tot.registered, tot.visited) == (len(w_stored), int((w_outcome & 2).astype(bool).sum()),
                                                                       int((w_outcome & 4).astype(bool).sum()), len(w_visited)), t
    assert ctx.color_map_size() == chk.sizes()
    keys, counts, times, xyz, pidx = ctx.color_map_download()
    w = chk.map_arrays()
    assert np.array_equal(keys, w[0]) and np.array_equal(counts, w[1]) and times.tobytes() == w[2].tobytes(), t
    assert xyz.tobytes() == w[3].tobytes() and np.array_equal(pidx, w[4]), t
    reg = ctx.color_registered_download()
    rx, rkeys, rs = chk.registered_arrays()
    assert np.stack([reg["x"], reg["y"], reg["z"]], 1).tobytes() == rx.tobytes() and np.array_equal(reg["slot"].astype(np.int32), rs), t
    assert np.array_equal(np.stack([reg["kx"], reg["ky"], reg["kz"]], 1), rkeys), t
    return tot


@pytest.mark.parametrize("family", FAMILIES)
def test_insert_wrap(family):
    """phase 1: the scene's three batches (a table of 32 768 slots) and a row of 512 voxels in the first 1 024 slots, numbers 1 ... 4.  Across
    the wrap two large batches, then the wrapping call with a row of 512 other voxels in the same 1 024 slots, large batches that create
    voxels on the numbers 2 and 3 and a row again on 4; a second jump crosses the wrap once more"""
    chk = cc.ColorChecker(*rk.OPT)
    ctx = _ctx()
    try:
        watch = _Watch(ctx, ("scratch_" + family,))
        shift = np.array([0.53, 0.31, -0.027])
        batches = [cc.scene_batch(0), cc.scene_batch(1), cc.scene_batch(2), _row_of_voxels(0)]
        across = [sk.extra_batch(), cc.scene_batch(1) + shift, _row_of_voxels(1), cc.scene_batch(2) + shift, cc.scene_batch(0) - 2 * shift, _row_of_voxels(2)]
        again = [_row_of_voxels(3), _row_of_voxels(4)[:200], cc.scene_batch(1)[:3000] - shift, _row_of_voxels(5)]
        assert all(len(b) >= 20 * len(across[2]) for b in batches[:3]) and 2 * len(across[2]) == 1024

        def insert(pts, t):
            return _insert(ctx, chk, watch, pts, t)

        t = 1.0
        for pts in batches:
            insert(pts, t); t += 1.0
        assert watch.read() == (4,)
        _jump(ctx, family)
        assert watch.read() == (LAST[family] - 2,)
        for n, pts in enumerate(across):
            created = insert(pts, t).created; t += 1.0
            assert created > 150                                           # every batch behind the jump creates voxels
            assert watch.read() == ((LAST[family] - 1, LAST[family], 1, 2, 3, 4)[n],)
        _jump(ctx, family, 0)                                              # the next call wraps
        assert watch.read() == (LAST[family],)
        for n, pts in enumerate(again):
            insert(pts, t); t += 1.0
            assert watch.read() == (n + 1,)
        watch.done(crossings=2, calls_after=6)
    finally:
        ctx.close()


def test_insert_epoch_wraps_twice_on_the_smallest_table():
    """An entry of the scratch table that wrongly counts as current does no harm by itself (a probe passes it, a key that equals it finds
    its own slot); harm is a table with no room left.  A table is made for twice its batch, so the entries of ONE earlier call of the same
    epoch cannot fill it: it takes two.  A table of 1 024 slots that is never re-allocated: a row of 512 voxels on epoch 1, single points on
    the epochs between (each takes one slot at most), the wrap and a second row on epoch 1, the wrap again and a third row on epoch 1 --
    without the fill at the wrap there would be more than 1 000 entries of epoch 1 in front of its 512 keys"""
    chk = cc.ColorChecker(*rk.OPT)
    ctx = _ctx()
    try:
        watch = _Watch(ctx, ("scratch_epoch",))
        single = lambda j: np.array([[0.05 + 0.1 * j, -7.05, 1.05]])
        t = 1.0
        for n, pts in enumerate((_row_of_voxels(0), single(0), single(1))):                       # epochs 1, 2, 3
            assert _insert(ctx, chk, watch, pts, t).created == len(pts); t += 1.0
        ctx.set_color_epochs(2, -1)
        for n, pts in enumerate((single(2), single(3), _row_of_voxels(1), single(4))):           # 0xFFFE, 0xFFFF, 1, 2
            assert _insert(ctx, chk, watch, pts, t).created == len(pts); t += 1.0
            assert watch.read() == ((0xFFFE, 0xFFFF, 1, 2)[n],)
        ctx.set_color_epochs(0, -1)
        assert watch.read() == (0xFFFF,)
        for n, pts in enumerate((_row_of_voxels(2), single(5))):                                 # 1, 2
            assert _insert(ctx, chk, watch, pts, t).created == len(pts); t += 1.0
            assert watch.read() == (1 + n,)
        watch.done(crossings=2, calls_after=2)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ all four, as a camera frame uses them
def _positions(smap):
    out = np.zeros((len(smap.pool_of), 3), np.float32)
    for (key, slot), pool in smap.pool_of.items():
        out[pool] = smap.chk.voxels[key].points[slot]
    return out


def _vio_scene(smap, rc, positions, img, cam, points):
    """vio_checker's view of the map: the colour state by pool position"""
    P = len(positions)
    n_rgb = np.zeros(P, np.int16); cov = np.zeros((P, 3), np.float32); rgb = np.zeros((P, 3), np.int16)
    for (key, slot), st in rc.state.items():
        pool = smap.pool_of[(key, slot)]
        n_rgb[pool] = st.n_rgb; cov[pool] = st.cov; rgb[pool] = st.rgb
    return vc.Scene(positions, n_rgb, cov, rgb, img, cam, vc.TIME_TD, vc.r_imu_camera(), points)


def test_all_four_interleaved_across_their_wraps():
    """camera frames as the odometry runs them: insert, select, track update, image upload, render, vio_rows.  Both families jump together
    behind the third frame; a frame asks the selection twice (totals, then records), renders three lists, inserts once, and
    the first frame behind the jump has no tracker update: the render's wrap falls on that frame, the selection's on the next, the
    insertion's on the third and the tracker's on the fourth; three more frames follow"""
    smap = sk.SelectMap(*rk.OPT)
    rc = rk.RenderChecker(smap.chk)
    ctx = _ctx()
    try:
        watches = {"insert": _Watch(ctx, ("scratch_epoch", "scratch_counter")), "select": _Watch(ctx, ("select_epoch", "select_counter")),
                   "track": _Watch(ctx, ("track_pool_epoch", "track_cell_epoch", "track_pool_counter", "track_cell_counter")),
                   "render": _Watch(ctx, ("render_epoch",))}
        wrapped_in = {}
        rng = np.random.default_rng(77)
        tracked = np.zeros(0, tk.TRACK_POINT_DTYPE)
        lists = []
        for frame in range(10):
            if frame == 3:
                ctx.set_color_epochs(2, 2)
            before = {name: w.crossings for name, w in watches.items()}
            pose, which, _, _ = rk.RENDERS[frame % len(rk.RENDERS)]
            cam = rk.scene_camera(rk.POSES[pose], which)
            rows, cols = rk.IMAGE_SIZES[which]
            img = rk.scene_image(which)
            t = 1.0 + frame
            # addPointToColorMap
            pts = cc.scene_batch(frame % 3)[:3000] + frame * np.array([0.37, -0.21, 0.013])
            outcome, stored, visited, _ = watches["insert"].call(ctx.color_map_insert, pts, t, 0.0)
            w_outcome, w_stored, w_visited = smap.insert(pts, t, 0.0)
            assert outcome.tobytes() == w_outcome.tobytes() and stored.tobytes() == w_stored.tobytes() and np.array_equal(visited, w_visited), frame
            lists = (lists + [visited])[-2:]
            # selectPointsForProjection over the voxels of the last two sweeps: totals, then records
            voxels = np.concatenate(lists)
            o = capi.default_color_select_opts(minimum_dis=10.0, skip_step=1, use_all_points=0, minimum_depth=sk.MINIMUM_DEPTH, maximum_depth=sk.MAXIMUM_DEPTH)
            tot = capi.ColorSelectTotals()
            watches["select"].call(lambda: ctx._chk(ctx.lib.srl_color_map_select(ctx.h, C.byref(_cam(cam)), rows, cols, capi._ptr(voxels), len(voxels), C.byref(o),
                                                                                 None, 0, C.byref(tot)), "srl_color_map_select"))
            want = sk.select_sequential(smap, cam, rows, cols, voxels)
            assert tot.as_tuple() == sk.totals_tuple(want[1]), frame
            selected = watches["select"].call(_select, ctx, cam, rows, cols, voxels, o)
            _same_selection(selected, want, frame)
            assert selected[1].selected > 30
            # updateAndAppendTrackPoints
            positions = _positions(smap)
            if frame != 3:
                flow = tk.perturbed(positions, cam, rows, cols, tracked, 500 + frame)
                cand = selected[0]["pool"][rng.permutation(len(selected[0]))].astype(np.int32)
                got = watches["track"].call(ctx.color_map_track_update, _cam(cam), rows, cols, flow, cand,
                                            capi.default_color_track_opts(mini_distance=10.0, maximum_tracked_points=300))
                w = tk.track_update_sequential(positions, cam, rows, cols, flow, cand, 10.0, 300)
                assert got[3].as_tuple() == tk.totals_tuple(w[3]), (frame, got[3].as_tuple(), w[3])
                assert got[1].tobytes() == w[1].tobytes() and got[2].tobytes() == w[2].tobytes() and got[0].tobytes() == w[0].tobytes(), frame
                tracked = got[0]
                assert len(tracked) > 30
            # the image, and three renders: the sweep's voxels, then every second of them twice more (three views: the photometric rows use them)
            ctx.color_image_upload(img)
            for part in (visited, visited[::2], visited[::2]):
                got = watches["render"].call(ctx.color_map_render, _cam(cam), part, 10.0 + 0.1 * frame)
                w = rc.render(cam, img, part, 10.0 + 0.1 * frame)
                assert got.as_tuple() == tuple(w[name] for name in rk.TOTALS), (frame, got.as_tuple(), w)
            assert rk.state_bytes(ctx.color_map_download_rgb()) == rk.state_bytes(rc.map_state()), frame
            # the measurement rows of the tracked points
            points = np.zeros(len(tracked), vc.POINT_DTYPE)
            points["pool"] = tracked["pool"]
            points["match_u"], points["match_v"] = tracked["u"].astype(np.float64) + 0.3, tracked["v"].astype(np.float64) - 0.2
            points["vel_u"], points["vel_v"] = 4.0, -3.0
            mode = vc.PHOTOMETRIC if frame % 2 else vc.REPROJECTION
            sums, v_rows, v_outcome = ctx.color_map_vio_rows(capi.ColorVioArgs(_cam(cam), vc.TIME_TD, (C.c_double * 9)(*vc.r_imu_camera().reshape(9)), mode, 1, 1),
                                                             points)
            w = vc.vio_rows(_vio_scene(smap, rc, positions, img, cam, points), mode)
            assert v_outcome.tobytes() == w.outcome.tobytes() and v_rows.tobytes() == w.rows.tobytes() and sums.counts() == w.counts, frame
            H, r, acc = sums.as_arrays()                                  # the sums: within what reordering a sum of doubles can move it by
            assert (np.abs(np.concatenate([[H[a, b] for a, b in vc.PAIRS], r, [acc]]) - w.sums) <= w.bound()).all() and sums.used > 10, frame
            for name, watch in watches.items():
                if watch.crossings > before[name]:
                    wrapped_in[name] = frame
        assert wrapped_in == {"render": 3, "select": 4, "insert": 5, "track": 6}, wrapped_in
        for watch in watches.values():
            watch.done(calls_after=3)                                      # the numbers 1 ... 3 of the frames in front of the jump, used again
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the render's 16-bit multiplicity
def _small_voxel(chk, cam, rows, cols):
    """the first voxel of the map with at most three points, all of which the camera colours (few points: the checker walks every occurrence)"""
    for key, vox in chk.voxels.items():
        if 1 <= len(vox.points) <= 3 and all(cam.project(tuple(float(c) for c in p), rows, cols)[0] == 0 for p in vox.points):
            return key
    raise AssertionError("no such voxel")


def test_render_multiplicity_at_and_beyond_what_a_mark_word_counts():
    """one voxel 65 535 times is rendered (updateRgb 65 535 times per point: N_rgb, a 16-bit count, ends at -1 without passing 0);
    65 536 times, alone or among other voxels, is refused with nothing changed and zero totals; the render behind a refusal is an
    ordinary one, and a second refusal is seen as the first was"""
    chk, chk_visited = rk.scene_map()
    rc = rk.RenderChecker(chk)
    ctx, visited = _scene_ctx()
    try:
        cam, which, _, _ = rk.render_call(0, visited)
        rows, cols = rk.IMAGE_SIZES[which]
        key = _small_voxel(chk, cam, rows, cols)
        n_points = len(chk.voxels[key].points)
        ctx.color_image_upload(rk.scene_image(which))
        at_limit = np.repeat(np.array([key], np.int32), 65535, 0)
        got = ctx.color_map_render(_cam(cam), at_limit, 10.0)
        want = rc.render(cam, rk.scene_image(which), at_limit, 10.0)
        assert got.as_tuple() == tuple(want[name] for name in rk.TOTALS) and got.first == n_points and got.updated == 65534 * n_points
        state = ctx.color_map_download_rgb()
        assert rk.state_bytes(state) == rk.state_bytes(rc.map_state())
        assert (state[1] == -1).sum() == n_points and (state[1] != 0).sum() == n_points      # N_rgb: 65 535 as an int16
        beyond = np.repeat(np.array([key], np.int32), 65536, 0)
        others = visited[0][:500]
        among = np.concatenate([others[:250], beyond[:40000], others[250:], beyond[40000:]])
        for n, refused in enumerate((beyond, among)):
            for attempt in range(2):
                before = rk.state_bytes(ctx.color_map_download_rgb())
                tot = capi.ColorRenderTotals(7, 7, 7, 7, 7, 7, 7)
                assert ctx.lib.srl_color_map_render(ctx.h, C.byref(_cam(cam)), capi._ptr(refused), len(refused), 11.0 + n, C.byref(tot)) == SRL_ERR_UNSUPPORTED
                assert tot.as_tuple() == (0,) * 7 and rk.state_bytes(ctx.color_map_download_rgb()) == before
                if attempt == 0:                                           # directly behind the refusal: an ordinary render
                    cam_k, which_k, obs_time, voxels = rk.render_call((2, 4)[n], visited)
                    ctx.color_image_upload(rk.scene_image(which_k))
                    got = ctx.color_map_render(_cam(cam_k), voxels, obs_time)
                    want = rc.render(cam_k, rk.scene_image(which_k), voxels, obs_time)
                    assert got.as_tuple() == tuple(want[name] for name in rk.TOTALS) and got.listed > 5000, (n, got.as_tuple(), want)
                    assert rk.state_bytes(ctx.color_map_download_rgb()) == rk.state_bytes(rc.map_state())
        assert rk.state_bytes(ctx.color_registered_rgb()) == rk.state_bytes(rc.registered_state())
    finally:
        ctx.close()
