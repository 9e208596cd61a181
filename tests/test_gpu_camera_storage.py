"""The storage transitions of the camera stage that no other test reaches: the flow tracker's point block growing and being used
below its capacity again, its upload blocks arriving before and after a prepared image, a tracker and a preparer destroyed and made again
at another size on one context, and the colour map's image growing through the preparer's hand-over between two uploads.  No checker is
needed: every expected value comes from a fresh context given the same inputs, and every comparison is bytewise."""
import ctypes as C

import numpy as np
import pytest

import color_checker as cc
import render_checker as rk
import sr_livo_amd as srl
from sr_livo_amd import capi

pytestmark = pytest.mark.gpu


def _bgr(rows, cols, seed, shift=0):
    """a seeded BGR texture (coarse blocks, a gradient, noise) moved by (shift, shift) pixels"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(40, 216, size=((rows + 7) // 8 + 1, (cols + 7) // 8 + 1, 3))
    img = np.kron(coarse, np.ones((8, 8, 1), np.int64))[:rows, :cols]
    yy, xx = np.mgrid[0:rows, 0:cols]
    img = img + ((xx + 2 * yy) % 23)[..., None] + rng.integers(-6, 7, size=img.shape)
    return np.roll(np.clip(img, 0, 255).astype(np.uint8), (shift, shift), axis=(0, 1))


def _gray(rows, cols, seed, shift=0):
    return np.ascontiguousarray(_bgr(rows, cols, seed, shift)[..., 1])


def _points(rows, cols, n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-3.0, cols + 3.0, n), rng.uniform(-3.0, rows + 3.0, n)], axis=1).astype(np.float32)


def _prep_opts(rows, cols):
    return capi.default_image_prep_opts(rows=rows, cols=cols, fx=0.9 * cols, fy=0.92 * cols, cx=cols / 2 - 0.37, cy=rows / 2 + 0.21,
                                        dist=[0.2, 0.05, 0.002, -0.003, 0.01])


def _same_track(got, want):
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2]


def _fresh_pair(ctx, first, second, pts):
    """what a new tracker of ctx answers for the pair of images"""
    flow = srl.Flow(ctx)
    try:
        flow.track_image(first, pts)
        return flow.track_image(second, pts)
    finally:
        flow.close()


def test_the_flow_point_block_grows_and_is_used_below_its_capacity_again():
    """64 x 48: two levels.  1 point, then 513 (past the first capacity of 512), 770 (past 513 + 256), 1 again"""
    rows, cols = 48, 64
    counts = (1, 513, 770, 1)
    imgs = [_gray(rows, cols, 3, k) for k in range(len(counts))]
    a, b = srl.Context(0), srl.Context(0)
    try:
        flow = srl.Flow(a)
        for k, n in enumerate(counts):
            pts = _points(rows, cols, n, 50 + k)
            got = flow.track_image(imgs[k], pts)
            assert flow.levels() == 1
            if k == 0:
                assert got[2] == 0 and got[0].tobytes() == pts.tobytes() and not got[1].any()
                continue
            want = _fresh_pair(b, imgs[k - 1], imgs[k], pts)
            _same_track(got, want)
            assert n == 1 or want[2] > n // 4
    finally:
        a.close()
        b.close()


def test_the_flow_upload_blocks_arrive_before_or_after_a_prepared_image():
    rows, cols = 48, 64
    pts = _points(rows, cols, 200, 7)
    frames = [_bgr(rows, cols, 9, k) for k in range(3)]
    ctxs = [srl.Context(0) for _ in range(3)]
    try:
        preps = [srl.ImagePrep(c, _prep_opts(rows, cols)) for c in ctxs[:2]]
        grays = []
        for f in frames:
            preps[0].prepare(f)
            grays.append(preps[0].download(capi.SRL_PREP_GRAY_EQ))
        only_uploads = srl.Flow(ctxs[2])
        want = [only_uploads.track_image(g, pts) for g in grays]
        assert want[1][2] > 50 and want[2][2] > 50
        for c, prep, prepared in ((ctxs[0], preps[0], (True, True, False)), (ctxs[1], preps[1], (False, False, True))):
            flow = srl.Flow(c)
            for k, from_prep in enumerate(prepared):
                if from_prep:
                    prep.prepare(frames[k])
                    got = flow.track_prepared(pts)
                else:
                    got = flow.track_image(grays[k], pts)
                _same_track(got, want[k])
    finally:
        for c in ctxs:
            c.close()


def test_a_tracker_made_again_at_another_size():
    sizes = ((48, 64), (96, 170))
    a, b = srl.Context(0), srl.Context(0)
    try:
        for rows, cols in sizes:
            imgs = [_gray(rows, cols, 13, k) for k in range(2)]
            pts = _points(rows, cols, 120, 17)
            flow = srl.Flow(a)
            try:
                flow.track_image(imgs[0], pts)
                # the set no image has reached yet reads zeros, whatever a tracker before this one left in memory
                for level in range(flow.levels() + 1):
                    img, der = flow.download_level(capi.SRL_FLOW_CUR, level)
                    assert not img.any() and not der.any(), level
                got = flow.track_image(imgs[1], pts)
            finally:
                flow.close()
        want = _fresh_pair(b, imgs[0], imgs[1], pts)              # the second size on a context that never saw the first
        _same_track(got, want)
        assert want[2] > 50
    finally:
        a.close()
        b.close()


def test_a_preparer_made_again_at_another_size():
    sizes = ((37, 53), (96, 170))
    a, b = srl.Context(0), srl.Context(0)
    try:
        for rows, cols in sizes:
            prep = srl.ImagePrep(a, _prep_opts(rows, cols))
            try:
                info = prep.prepare(_bgr(rows, cols, 19))
                got = [prep.download(w) for w in (capi.SRL_PREP_GRAY_EQ, capi.SRL_PREP_BGR_EQ)]
                got += [prep.download_stage(s, info.tiles) for s in (capi.SRL_PREP_STAGE_UNDIST, capi.SRL_PREP_STAGE_YCRCB, capi.SRL_PREP_STAGE_LUT_Y)]
            finally:
                prep.close()
        prep = srl.ImagePrep(b, _prep_opts(rows, cols))
        info_b = prep.prepare(_bgr(rows, cols, 19))
        want = [prep.download(w) for w in (capi.SRL_PREP_GRAY_EQ, capi.SRL_PREP_BGR_EQ)]
        want += [prep.download_stage(s, info_b.tiles) for s in (capi.SRL_PREP_STAGE_UNDIST, capi.SRL_PREP_STAGE_YCRCB, capi.SRL_PREP_STAGE_LUT_Y)]
        assert info.as_tuple() == info_b.as_tuple()
        assert [g.tobytes() for g in got] == [w.tobytes() for w in want] and want[0].any()
    finally:
        a.close()
        b.close()


def _camera(rows, cols):
    """the render scene's overview camera for an image of another size with the same 3 : 4 shape"""
    cam = rk.scene_camera(rk.POSES[0], 0)
    s = cols / rk.IMAGE_SIZES[0][1]
    assert rows * rk.IMAGE_SIZES[0][1] == cols * rk.IMAGE_SIZES[0][0]
    return capi.ColorCamera((C.c_double * 4)(*cam.q), (C.c_double * 3)(*cam.t), cam.fx * s, cam.fy * s, cam.cx * s, cam.cy * s, cam.fov_margin)


def _colour_context():
    ctx = srl.Context(0)
    o = rk.OPT
    ctx.color_map_create(capi.default_color_opts(size_voxel_map=o[0], max_num_points_in_voxel=o[1], min_distance_points=o[2], add_point_step=o[3]))
    visited = ctx.color_map_insert(cc.scene_batch(0), 1.0, 0.0)[2]
    return ctx, visited


def test_the_colour_image_grows_through_an_install_between_two_uploads():
    """upload 48 x 64, the preparer's hand-over at 96 x 128, upload 48 x 64 again.  The three renders list disjoint thirds of the
    voxels, so what a render does to its points does not depend on the renders before it: it is what a fresh context that only saw
    that image does, and the other points stay as they were."""
    small, large = (48, 64), (96, 128)
    a, visited = _colour_context()
    try:
        thirds = np.array_split(visited, 3)
        prep = srl.ImagePrep(a, _prep_opts(*large))
        before = a.color_map_download_rgb()
        for k, third in enumerate(thirds):
            if k == 1:
                assert prep.prepare(_bgr(*large, 31)).installed_color == 1
                image, size = prep.download(capi.SRL_PREP_BGR_EQ), large
            else:
                image, size = _bgr(*small, 29 + k), small
                a.color_image_upload(image)
            tot = a.color_map_render(_camera(*size), third, 5.0 + k)
            after = a.color_map_download_rgb()
            b, visited_b = _colour_context()
            try:
                assert np.array_equal(visited_b, visited)
                b.color_image_upload(image)
                tot_b = b.color_map_render(_camera(*size), third, 5.0 + k)
                want = b.color_map_download_rgb()
            finally:
                b.close()
            assert tot.as_tuple() == tot_b.as_tuple() and tot.first > 10, tot.as_tuple()
            touched = want[1] != 0                                  # n_rgb: the points this render gave a colour
            assert touched.any() and not (before[1] != 0)[touched].any()
            for got_a, want_a, before_a in zip(after, want, before):
                assert got_a[touched].tobytes() == want_a[touched].tobytes()
                assert got_a[~touched].tobytes() == before_a[~touched].tobytes()
            before = after
    finally:
        a.close()
