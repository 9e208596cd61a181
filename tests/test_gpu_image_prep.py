"""The image preparation on the device (srl_image_prepare: undistortion, gray, CLAHE, YCrCb equalisation; include/srlivo_hip.h) against
the independent restatement of tests/imgprep_checker.py -- there is no OpenCV to compare with, and the contract claims none.

Every comparison is BYTEWISE, through the C-ABI: every intermediate stage (undist, gray, Y / CrCb, both sets of look-up tables), both
results and the info record.  No tolerance: integer arithmetic and uncontracted IEEE FP32 / FP64 are exact on both sides.  Images are
seeded and structured (gradients, blocks of 0 and 255 that overflow the clip limit, noise), carry all 216 pixels of {0, 1, 127, 128, 254,
255}^3, and are handed over with row_stride_bytes > 3 cols and poisoned padding."""
import ctypes as C
import functools

import numpy as np
import pytest

import imgprep_checker as ck
import sr_livo_amd as srl
from imgprep_cases import image as _image          # (rows, cols, seed): strided, poisoned padding, read-only
from imgprep_device import check_all as _check_all, same as _same
from sr_livo_amd import capi

pytestmark = pytest.mark.gpu
SRL_OK, SRL_ERR_BAD_ARG, SRL_ERR_UNSUPPORTED, SRL_ERR_NO_MAP, SRL_ERR_NO_SWEEP = 0, -3, -4, -5, -6
MILD = (0.2, 0.05, 0.002, -0.003, 0.01)          # pincushion: the corners come from outside the image
DISTORTIONS = {"zero": (0, 0, 0, 0, 0), "barrel": (-0.3, 0, 0, 0, 0), "pincushion with tangential": (0.3, 0.1, 0.01, -0.01, 0.02)}


def _opts(rows, cols, dist=MILD, tiles=0):
    return capi.default_image_prep_opts(rows=rows, cols=cols, fx=0.9 * cols, fy=0.92 * cols, cx=cols / 2 - 0.37, cy=rows / 2 + 0.21, dist=list(dist),
                                        tiles=tiles)


@functools.lru_cache(maxsize=None)
def _want(rows, cols, seed, dist=MILD, tiles=0):
    """the checker's chain, computed once per case and shared"""
    o = _opts(rows, cols, dist, tiles)
    w = ck.prepare(np.ascontiguousarray(_image(rows, cols, seed)), o.fx, o.fy, o.cx, o.cy, list(o.dist), o.clip_gray, o.clip_color, tiles)
    for v in w.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return w


def _run(rows, cols, seed, dist=MILD, tiles=0):
    ctx = srl.Context(0)
    try:
        prep = srl.ImagePrep(ctx, _opts(rows, cols, dist, tiles))
        info = prep.prepare(_image(rows, cols, seed))
        want = _want(rows, cols, seed, dist, tiles)
        _check_all(prep, info, want)
        return want, info
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("rows,cols,T,tile", [
    (37, 53, 4, (14, 10)),            # both dimensions ragged, odd width
    (96, 160, 8, (20, 12)),           # both divide: no extension
    (96, 170, 8, (22, 13)),           # rows divide, cols do not: rows grow by a whole T
    (250, 330, 16, (21, 16)),
    (480, 640, 32, (20, 15)),
    (1024, 1280, 64, (20, 16)),       # the product shape
])
def test_every_stage_equals_the_checker(rows, cols, T, tile):
    want, info = _run(rows, cols, 11)
    assert (info.tiles, info.tile_w, info.tile_h) == (T,) + tile
    # the case exercises what it is there for: pixels from outside the image, and tiles whose bins were cut
    assert (want["map1"][..., 0] < 0).any() and (want["map1"][..., 0] >= cols - 1).any()
    assert len(np.unique(want["lut_gray"].reshape(-1, 256), axis=0)) > 1


# ------------------------------------------------------------------------------------------------ 2. distortion
@pytest.mark.parametrize("name", list(DISTORTIONS))
def test_distortions(name):
    rows, cols = 96, 170
    want, _ = _run(rows, cols, 12, DISTORTIONS[name])
    if name == "zero":
        assert np.array_equal(want["undist"], _image(rows, cols, 12))      # ... and the device equalled `want` bytewise
    else:
        assert not np.array_equal(want["undist"], _image(rows, cols, 12))


# ------------------------------------------------------------------------------------------------ 3. tiles given
@pytest.mark.parametrize("tiles", [2, 18])               # 18 = min(37, 53) / 2
def test_tiles_given_explicitly(tiles):
    _, info = _run(37, 53, 13, MILD, tiles)
    assert info.tiles == tiles


# ------------------------------------------------------------------------------------------------ 4. repeatability
def test_repeats_a_second_image_and_a_refused_size():
    rows, cols = 96, 170
    ctx = srl.Context(0)
    try:
        prep = srl.ImagePrep(ctx, _opts(rows, cols))
        first = _want(rows, cols, 21)
        prep.prepare(_image(rows, cols, 21))
        a = (prep.download(0).tobytes(), prep.download(1).tobytes())
        info = prep.prepare(_image(rows, cols, 21))
        assert (prep.download(0).tobytes(), prep.download(1).tobytes()) == a      # the same bytes call after call
        _check_all(prep, info, first)
        info = prep.prepare(_image(rows, cols, 22))                                # another image into the same buffers
        _check_all(prep, info, _want(rows, cols, 22))
        assert prep.download(0).tobytes() != a[0]
        # a wrong size is refused, the info zeroed, and the previous results are still there
        other = np.ascontiguousarray(_image(37, 53, 13))
        bad = capi.ImagePrepInfo()
        C.memset(C.byref(bad), 0xFF, C.sizeof(bad))
        assert ctx.lib.srl_image_prepare(ctx.h, capi._ptr(other), 37, 53, 159, C.byref(bad)) == SRL_ERR_BAD_ARG and bad.as_tuple() == (0,) * 8
        img = _image(rows, cols, 22)
        assert ctx.lib.srl_image_prepare(ctx.h, capi._ptr(img), rows, cols, 3 * cols - 1, None) == SRL_ERR_BAD_ARG
        assert ctx.lib.srl_image_prepare(ctx.h, None, rows, cols, 3 * cols, None) == SRL_ERR_BAD_ARG
        _check_all(prep, info, _want(rows, cols, 22))
        # a strided download leaves the padding alone
        out = np.full((rows, cols + 5), 7, np.uint8)
        assert ctx.lib.srl_image_prep_download(ctx.h, 0, capi._ptr(out), cols + 5) == SRL_OK
        assert np.array_equal(out[:, :cols], _want(rows, cols, 22)["gray_eq"]) and (out[:, cols:] == 7).all()
        assert ctx.lib.srl_image_prep_download(ctx.h, 0, capi._ptr(out), cols - 1) == SRL_ERR_BAD_ARG
        assert ctx.lib.srl_image_prep_download(ctx.h, 1, capi._ptr(out), 3 * cols - 1) == SRL_ERR_BAD_ARG
        assert ctx.lib.srl_image_prep_download(ctx.h, 2, capi._ptr(out), 3 * cols) == SRL_ERR_BAD_ARG
        assert ctx.lib.srl_image_prep_download_stage(ctx.h, capi.SRL_PREP_STAGE_GRAY, capi._ptr(out), rows * cols - 1) == SRL_ERR_BAD_ARG
        assert ctx.lib.srl_image_prep_download_stage(ctx.h, 5, capi._ptr(out), out.size) == SRL_ERR_BAD_ARG
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 5. consumers
def test_the_colour_map_renders_the_prepared_image_as_an_uploaded_one():
    import color_checker as cc
    import render_checker as rk
    rows, cols = rk.IMAGE_SIZES[0]
    cam = rk.scene_camera(rk.POSES[0], 0)
    cam = capi.ColorCamera((C.c_double * 4)(*cam.q), (C.c_double * 3)(*cam.t), cam.fx, cam.fy, cam.cx, cam.cy, cam.fov_margin)
    want = _want(rows, cols, 11)
    states = []
    for prepared in (True, False):
        ctx = srl.Context(0)
        try:
            o = rk.OPT
            ctx.color_map_create(capi.default_color_opts(size_voxel_map=o[0], max_num_points_in_voxel=o[1], min_distance_points=o[2], add_point_step=o[3]))
            visited = ctx.color_map_insert(cc.scene_batch(0), 1.0, 0.0)[2]
            if prepared:
                prep = srl.ImagePrep(ctx, _opts(rows, cols))
                info = prep.prepare(_image(rows, cols, 11))      # the first image: the colour state is allocated here
                assert info.installed_color == 1
                _same("bgr_eq", prep.download(capi.SRL_PREP_BGR_EQ), want["bgr_eq"])
            else:
                ctx.color_image_upload(want["bgr_eq"])
            tot = ctx.color_map_render(cam, visited, 5.0)
            assert tot.first > 100
            states.append((tot.as_tuple(),) + tuple(a.tobytes() for a in ctx.color_map_download_rgb()))
        finally:
            ctx.close()
    assert states[0] == states[1]


def _points(rows, cols, n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.1 * cols, 0.9 * cols, n), rng.uniform(0.1 * rows, 0.9 * rows, n)], axis=1).astype(np.float32)


def test_the_flow_tracks_the_prepared_gray_as_an_uploaded_one():
    rows, cols = 96, 170
    pts = _points(rows, cols, 200, 5)
    frames = [_image(rows, cols, 21), np.roll(np.ascontiguousarray(_image(rows, cols, 21)), (1, 2), axis=(0, 1))]      # the content moves by (+2, +1)
    a, b = srl.Context(0), srl.Context(0)
    try:
        prep = srl.ImagePrep(a, _opts(rows, cols))
        fa, fb = srl.Flow(a), srl.Flow(b)
        assert a.lib.srl_flow_track_prepared(a.h, None, 0, None, None, None) == SRL_ERR_NO_SWEEP      # before the first image
        results = []
        for frame in frames:
            prep.prepare(frame)
            got = fa.track_prepared(pts)
            ref = fb.track_image(prep.download(capi.SRL_PREP_GRAY_EQ), pts)
            assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes() and got[2] == ref[2]
            results.append(got)
        assert results[0][2] == 0 and np.array_equal(results[0][0], pts)      # a tracker's first image is only stored
        nxt, status, n = results[1]
        assert n > 100 and np.abs(np.median((nxt - pts)[status == 1], axis=0) - (2.0, 1.0)).max() < 0.5
        # both entries on one tracker: the uploaded image after two prepared ones
        again = fa.track_image(prep.download(capi.SRL_PREP_GRAY_EQ), pts)
        assert again[2] > 100 and np.abs(np.median((again[0] - pts)[again[1] == 1], axis=0)).max() < 0.1
    finally:
        a.close()
        b.close()


def test_the_mirror_tracks_the_prepared_image_as_the_same_gray_from_the_host():
    rows, cols = 96, 170
    n = 60
    rec = np.zeros(n, capi.COLOR_SELECTED_DTYPE)
    rec["pool"] = np.arange(n) * 3 + 1
    xy = _points(rows, cols, n, 6)
    rec["u"], rec["v"] = xy[:, 0], xy[:, 1]
    rec["x"], rec["y"], rec["z"] = 1.0, 2.0, 5.0
    frames = [_image(rows, cols, 21), np.roll(np.ascontiguousarray(_image(rows, cols, 21)), (1, 2), axis=(0, 1))]
    a, b = srl.Context(0), srl.Context(0)
    ofa, ofb = srl.Oft(a), srl.Oft(b)
    try:
        prep = srl.ImagePrep(a, _opts(rows, cols))
        ofa.use_prepared_image(True)
        for o in (ofa, ofb):
            o.set_fundamental_provider(lambda last, cur, status: (status.__setitem__(slice(None), 1), 0)[1])
        prep.prepare(frames[0])
        ofa.init(rec, None, 10.0)
        ofb.init(rec, prep.download(capi.SRL_PREP_GRAY_EQ), 10.0)
        prep.prepare(frames[1])
        na = ofa.track_image(None, 10.1, rows, cols)
        nb = ofb.track_image(prep.download(capi.SRL_PREP_GRAY_EQ), 10.1, rows, cols)
        assert na == nb and na > 30 and ofa.sizes() == ofb.sizes()
        for which in (0, 1):
            assert ofa.pose_map(which).tobytes() == ofb.pose_map(which).tobytes()
        cur = ofa.pose_map(1)
        by_pool = {int(r["pool"]): r for r in rec}
        moved = np.array([[r["u"] - by_pool[int(r["pool"])]["u"], r["v"] - by_pool[int(r["pool"])]["v"]] for r in cur])
        assert np.abs(np.median(moved, axis=0) - (2.0, 1.0)).max() < 0.5       # the device's flow on the prepared image
    finally:
        ofa.close()
        ofb.close()
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ 6. refusals that need a context
def test_refusals_on_a_device():
    rows, cols = 37, 53
    ctx = srl.Context(0)
    try:
        lib = ctx.lib
        img = np.ascontiguousarray(_image(rows, cols, 13))
        out = np.zeros((rows, cols, 3), np.uint8)
        info = capi.ImagePrepInfo()
        pts = _points(rows, cols, 4, 1)
        nxt, st, nt = np.zeros((4, 2), np.float32), np.zeros(4, np.uint8), C.c_int(-1)
        track = lambda: lib.srl_flow_track_prepared(ctx.h, capi._ptr(pts), 4, capi._ptr(nxt), capi._ptr(st), C.byref(nt))      # noqa: E731
        # no preparer
        assert lib.srl_image_prepare(ctx.h, capi._ptr(img), rows, cols, 3 * cols, C.byref(info)) == SRL_ERR_NO_MAP
        assert lib.srl_image_prep_download(ctx.h, 0, capi._ptr(out), cols) == SRL_ERR_NO_MAP
        assert lib.srl_image_prep_download_stage(ctx.h, 0, capi._ptr(out), out.size) == SRL_ERR_NO_MAP
        assert track() == SRL_ERR_NO_MAP                                        # ... and no tracker
        assert lib.srl_image_prep_destroy(ctx.h) == SRL_OK
        flow = srl.Flow(ctx)
        assert track() == SRL_ERR_NO_MAP and nt.value == 0                      # a tracker, still no preparer
        o = _opts(rows, cols)
        bad = _opts(rows, cols, tiles=19)
        assert lib.srl_image_prep_create(ctx.h, C.byref(bad)) == SRL_ERR_BAD_ARG and lib.srl_image_prep_create(ctx.h, None) == SRL_ERR_BAD_ARG
        ctx.comm_set_host_callbacks(2, 0, lambda a: None, lambda v: [v, v])       # more than one rank
        assert lib.srl_image_prep_create(ctx.h, C.byref(o)) == SRL_ERR_UNSUPPORTED
        ctx.comm_set_host_callbacks(1, 0, None, None)
        assert lib.srl_image_prep_create(ctx.h, C.byref(o)) == SRL_OK
        assert lib.srl_image_prep_create(ctx.h, C.byref(o)) == SRL_ERR_BAD_ARG  # a second create
        # before the first image
        assert lib.srl_image_prep_download(ctx.h, 0, capi._ptr(out), cols) == SRL_ERR_NO_SWEEP
        assert lib.srl_image_prep_download_stage(ctx.h, 0, capi._ptr(out), out.size) == SRL_ERR_NO_SWEEP
        assert track() == SRL_ERR_NO_SWEEP
        ctx.comm_set_host_callbacks(2, 0, lambda a: None, lambda v: [v, v])
        assert lib.srl_image_prepare(ctx.h, capi._ptr(img), rows, cols, 3 * cols, C.byref(info)) == SRL_ERR_UNSUPPORTED and info.as_tuple() == (0,) * 8
        ctx.comm_set_host_callbacks(1, 0, None, None)
        assert lib.srl_image_prepare(ctx.h, capi._ptr(img), rows, cols, 3 * cols, C.byref(info)) == SRL_OK and info.installed_color == 0
        assert track() == SRL_OK
        flow.close()
        # a tracker whose first image had another size
        flow = srl.Flow(ctx)
        flow.track_image(np.zeros((40, 60), np.uint8), pts)
        assert track() == SRL_ERR_BAD_ARG
        flow.close()
        assert lib.srl_image_prep_destroy(ctx.h) == SRL_OK and lib.srl_image_prep_destroy(ctx.h) == SRL_OK
        assert lib.srl_image_prep_download(ctx.h, 0, capi._ptr(out), cols) == SRL_ERR_NO_MAP
        assert lib.srl_image_prep_create(ctx.h, C.byref(o)) == SRL_OK           # and a new one may be made
    finally:
        ctx.close()
