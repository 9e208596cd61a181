"""The totals of the colour map's counting kernels (k_render_points, k_select_cells, k_cloud_flags: csrc/srl_wg_totals.h) with the
number of workgroups on the edges of the final sum: one wave of the last workgroup adds the rows up, so 64 workgroups give every lane
one row and 65 give lane 0 two.  The scenes of the other tests never put the count there.

The map is a lattice with one point per 0.1-m voxel and per grid cell, so a map of P points holds exactly P stored and P registered
points and the pool position of point n is n.  The render and the all-points selection launch ceil(P / 256) workgroups of 256, the
cloud export ceil(n / 1024) of 1024 for a range of n points.  Totals (and the records that come with them) are compared with the
sequential restatements tests/render_checker.py, tests/select_checker.py and tests/cloud_export_checker.py.  Every call is made twice in
a row and gives the same totals -- the ticket came back to zero -- and where a call can launch fewer workgroups than the one before it
on the same context (selection, cloud export; the pool a render sweeps only grows), the largest shape is followed by the smallest:
rows beyond gridDim.x are not read."""
import ctypes as C
import math

import numpy as np
import pytest

import cloud_export_checker as ck
import render_checker as rk
import select_checker as sk
import sr_livo_amd as srl
from sr_livo_amd import capi

pytestmark = pytest.mark.gpu
SIZES = (1, 256, 257, 64 * 256, 64 * 256 + 1)                   # 1, 1, 2, 64, 65 workgroups of 256
RANGES = (1, 1024, 1025, 64 * 1024, 64 * 1024 + 1)              # 1, 1, 2, 64, 65 workgroups of 1024
CLOUD_POINTS = 65600
UNKNOWN_KEY = (1000, 1000, 1000)
WHICH = 1                                                       # the 375 x 500 image
# (yaw, pitch down, roll, position): inside the lattice, so that points lie behind it, beside its image and in it; NEAR is the same
# camera 1.2 m further along its axis: what it colours first is farther than 1.2 x that distance from FAR and is gated there
FAR = (0.3, 0.3, 0.0, (1.5, 0.2, 0.9))
NEAR = (0.3, 0.3, 0.0, (1.5 + 1.2 * math.cos(0.3) * math.cos(0.3), 0.2 + 1.2 * math.sin(0.3) * math.cos(0.3), 0.9 - 1.2 * math.sin(0.3)))
ABOVE = (0.0, 1.45, 0.0, (2.2, 3.2, 6.0))                        # looks down on the lattice: all of it is in the image
DEPTHS = (0.95, 4.5)                                             # minimum_depth, maximum_depth of the selection: both cut


def _cam(c):
    return capi.ColorCamera((C.c_double * 4)(*c.q), (C.c_double * 3)(*c.t), c.fx, c.fy, c.cx, c.cy, c.fov_margin)


def _ctx():
    """a context with a colour map under the shipped options"""
    o = rk.OPT
    ctx = srl.Context(0)
    ctx.color_map_create(capi.default_color_opts(size_voxel_map=o[0], max_num_points_in_voxel=o[1], min_distance_points=o[2], add_point_step=o[3]))
    return ctx


def _opts(skip=1):
    """the whole registered list, every skip-th candidate, between the two depths"""
    return capi.default_color_select_opts(skip_step=skip, use_all_points=1, minimum_depth=DEPTHS[0], maximum_depth=DEPTHS[1])


def _lattice(lo, hi):
    """points lo ... hi - 1: point n in voxel (n % 64, n / 64 % 64, n / 4096), at its centre"""
    n = np.arange(lo, hi)
    return (np.stack([n % 64, n // 64 % 64, n // 4096], 1) + 0.5) * 0.1


def _voxels_of(points):
    n = np.asarray(points)
    return np.stack([n % 64, n // 64 % 64, n // 4096], 1).astype(np.int32)


def _render_list(P):
    """every point of a small map, every 17th of a larger one and its last (every workgroup's row counts some); the first five voxels
    three times; a key the map does not hold"""
    pts = np.arange(P) if P <= 257 else np.union1d(np.arange(0, P, 17), [P - 1])
    return np.concatenate([_voxels_of(pts), _voxels_of(pts[:5]), _voxels_of(pts[:5]), np.array([UNKNOWN_KEY], np.int32)])


def _render_both(ctx, chk, img, pose, voxels, obs_time):
    cam = rk.scene_camera(pose, WHICH)
    got = ctx.color_map_render(_cam(cam), voxels, obs_time).as_tuple()
    tot = chk.render(cam, img, voxels, obs_time)
    want = tuple(tot[name] for name in rk.TOTALS)
    assert got == want, (pose, got, want)
    return dict(zip(rk.TOTALS, got))


def test_render_and_all_points_selection_at_1_1_2_64_65_workgroups():
    smap = sk.SelectMap(*rk.OPT)
    chk = rk.RenderChecker(smap.chk)
    img = rk.scene_image(WHICH)
    rows, cols = img.shape[:2]
    cam = rk.scene_camera(FAR, WHICH)
    sopts = dict(use_all_points=True, minimum_depth=DEPTHS[0], maximum_depth=DEPTHS[1])
    ctx = _ctx()
    try:
        ctx.color_image_upload(img)
        have = 0
        for P in SIZES:
            pts = _lattice(have, P)
            smap.insert(pts, 1.0 + P, 0.0)
            ctx.color_map_insert(pts, 1.0 + P, 0.0, want_outcome=False, want_stored=False)
            have = P
            assert smap.chk.sizes() == (P, P, P, P)                        # all stored, all registered, one per voxel and per cell
            assert ctx.color_map_size() == (P, P, P, P)
            # the render.  Two calls settle the state (the points NEAR sees get their first colour from close by, the others from FAR);
            # after them a call from FAR changes colours but no count: listed, behind, outside, gated, updated, unknown
            voxels = _render_list(P)
            t = 10.0 + P * 1e-4
            _render_both(ctx, chk, img, NEAR, voxels, t)
            _render_both(ctx, chk, img, FAR, voxels, t + 0.01)
            a = _render_both(ctx, chk, img, FAR, voxels, t + 0.02)
            b = _render_both(ctx, chk, img, FAR, voxels, t + 0.03)
            print("P %d render" % P, a)
            assert a == b and a["first"] == 0
            assert sum(1 for v in a.values() if v) >= 3, a
            if P >= 256:
                assert sum(1 for name in ("behind", "outside", "gated", "updated") if a[name]) >= 3, a
            # the selection over the whole registered list
            want = sk.select_sequential(smap, cam, rows, cols, None, **sopts)
            got = [ctx.color_map_select(_cam(cam), rows, cols, None, _opts()) for _ in range(2)]
            for rec, tot in got:
                assert tot.as_tuple() == sk.totals_tuple(want[1]), (P, tot.as_tuple(), want[1])
                assert rec.tobytes() == want[0].tobytes(), P
            print("P %d select" % P, want[1])
            assert want[1]["candidates"] == want[1]["visited"] == P
            assert sum(1 for v in want[1].values() if v) >= 3, want[1]
            if P >= 256:
                assert sum(1 for name in ("far", "near", "behind", "outside") if want[1][name]) >= 3 and want[1]["selected"] > 0, want[1]
        # 65 workgroups, then one: every P-th candidate of P is the first alone
        for skip in (have, 1, have):
            want = sk.select_sequential(smap, cam, rows, cols, None, skip_step=skip, **sopts)
            rec, tot = ctx.color_map_select(_cam(cam), rows, cols, None, _opts(skip))
            assert tot.as_tuple() == sk.totals_tuple(want[1]) and rec.tobytes() == want[0].tobytes(), skip
            assert tot.visited == (1 if skip == have else have)
    finally:
        ctx.close()


def test_cloud_export_over_ranges_of_1_1_2_64_65_workgroups():
    smap = sk.SelectMap(*rk.OPT)
    chk = rk.RenderChecker(smap.chk)
    img = rk.scene_image(WHICH)
    pts = _lattice(0, CLOUD_POINTS)
    ctx = _ctx()
    try:
        smap.insert(pts, 1.0, 0.0)
        ctx.color_map_insert(pts, 1.0, 0.0, want_outcome=False, want_stored=False)
        assert smap.chk.sizes() == ctx.color_map_size() == (CLOUD_POINTS,) * 4
        # N_rgb 0, 1 and 2 and two observation times in every thousand points
        ctx.color_image_upload(img)
        for step, t in ((23, 10.0), (29, 11.0)):
            _render_both(ctx, chk, img, ABOVE, _voxels_of(np.arange(0, CLOUD_POINTS, step)), t)
        rgb, n_rgb, _, _, time = chk.registered_state()
        reg = ck.Registered(smap.chk.registered_arrays()[0], rgb, n_rgb, time)
        first = 5
        for n in RANGES + (RANGES[0],):                                    # ... and after the largest the smallest
            for reverse, since in ((False, -math.inf), (True, 10.5)):
                want = ck.export(reg, first, n, 1, reverse, since)
                for _ in range(2):
                    rec, idx, tot = ctx.color_map_export_cloud(first, n, capi.default_color_cloud_opts(minimum_views=1, reverse=int(reverse), since=since))
                    assert tot.as_tuple() == ck.totals_tuple(want[2]), (n, reverse, since, tot.as_tuple(), want[2])
                    assert rec.tobytes() == want[0].tobytes() and np.array_equal(idx, want[1]), (n, reverse, since)
                print("n %d reverse %d since %s" % (n, reverse, since), want[2])
                if n >= 1024:
                    assert want[2]["below_views"] > 0 and want[2]["published"] > 0 and (want[2]["stale"] > 0) == (since > 0), (n, want[2])
    finally:
        ctx.close()
