"""The resize of the image preparation on the device (srl_image_prepare_resized; include/srlivo_hip.h, stage (r)) against the independent
restatement of tests/resize_checker.py followed by tests/imgprep_checker.py.

Every comparison is BYTEWISE, through the C-ABI: the resized frame (srl_image_prep_download_resized), every later stage
(srl_image_prep_download_stage), both results and the info record.  No tolerance: the resize is integer arithmetic on both sides.  Source
images come from tests/resize_cases.py: row_stride_bytes > 3 cols, poisoned padding, read-only."""
import ctypes as C
import functools

import numpy as np
import pytest

import imgprep_checker as ck
import resize_cases as rc
import resize_checker as rk
import sr_livo_amd as srl
from sr_livo_amd import capi

pytestmark = pytest.mark.gpu
SRL_OK, SRL_ERR_BAD_ARG, SRL_ERR_UNSUPPORTED, SRL_ERR_NO_MAP, SRL_ERR_NO_SWEEP = 0, -3, -4, -5, -6
MILD = (0.2, 0.05, 0.002, -0.003, 0.01)          # pincushion: the corners come from outside the image


def _opts(rows, cols):
    return capi.default_image_prep_opts(rows=rows, cols=cols, fx=0.9 * cols, fy=0.92 * cols, cx=cols / 2 - 0.37, cy=rows / 2 + 0.21, dist=list(MILD))


@functools.lru_cache(maxsize=None)
def _want(src, dst, seed):
    """the checker's resize and chain, computed once per case and shared"""
    o = _opts(*dst)
    resized = rk.resize(np.ascontiguousarray(rc.image(src[0], src[1], seed)), dst[0], dst[1])
    w = ck.prepare(resized, o.fx, o.fy, o.cx, o.cy, list(o.dist), o.clip_gray, o.clip_color, 0)
    w["resized"] = resized
    for v in w.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return w


def _same(name, got, want):
    want = np.ascontiguousarray(want)
    assert got.size == want.size, (name, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, (name, bad.size, bad[:8], got.ravel()[bad[:8]], want.ravel()[bad[:8]])


def _check_all(prep, info, want):
    assert info.as_tuple() == want["info"] + (0,), (info.as_tuple(), want["info"])
    T = info.tiles
    _same("resized", prep.download_resized(), want["resized"])
    _same("undist", prep.download_stage(capi.SRL_PREP_STAGE_UNDIST, T), want["undist"])
    _same("gray", prep.download_stage(capi.SRL_PREP_STAGE_GRAY, T), want["gray"])
    ycrcb = np.concatenate([want["y"].ravel(), np.stack([want["cr"], want["cb"]], axis=-1).ravel()])
    _same("ycrcb", prep.download_stage(capi.SRL_PREP_STAGE_YCRCB, T), ycrcb)
    _same("lut_gray", prep.download_stage(capi.SRL_PREP_STAGE_LUT_GRAY, T), want["lut_gray"])
    _same("lut_y", prep.download_stage(capi.SRL_PREP_STAGE_LUT_Y, T), want["lut_y"])
    _same("gray_eq", prep.download(capi.SRL_PREP_GRAY_EQ), want["gray_eq"])
    _same("bgr_eq", prep.download(capi.SRL_PREP_BGR_EQ), want["bgr_eq"])


def _all_bytes(prep, tiles):
    stages = [prep.download_resized()] + [prep.download_stage(s, tiles) for s in range(5)] + [prep.download(0), prep.download(1)]
    return tuple(a.tobytes() for a in stages)


# ------------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("src,dst,what", rc.SHAPES, ids=[s[2] for s in rc.SHAPES])
def test_every_stage_equals_the_checker(src, dst, what):
    ctx = srl.Context(0)
    try:
        prep = srl.ImagePrep(ctx, _opts(*dst))
        info = prep.prepare_resized(rc.image(src[0], src[1], 31))
        want = _want(src, dst, 31)
        _check_all(prep, info, want)
        # the case exercises what it is there for
        assert rk.is_exact_half(src, *dst) == (what.startswith("exact half") or src == (192, 340))
        if src == (1, 1):
            assert (want["resized"] == np.asarray(rc.image(1, 1, 31))[0, 0]).all()
        else:
            assert len(np.unique(want["resized"].reshape(-1, 3), axis=0)) > 100
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 2. equal sizes
def test_equal_sizes_run_no_resize_and_equal_the_plain_prepare():
    rows, cols = 37, 53
    img = rc.image(rows, cols, 32)
    a, b = srl.Context(0), srl.Context(0)
    try:
        pa, pb = srl.ImagePrep(a, _opts(rows, cols)), srl.ImagePrep(b, _opts(rows, cols))
        ia = pa.prepare_resized(img)
        ib = pb.prepare(img)
        assert ia.as_tuple() == ib.as_tuple()
        assert _all_bytes(pa, ia.tiles) == _all_bytes(pb, ib.tiles)
        _same("resized", pa.download_resized(), np.ascontiguousarray(img))      # the frame as uploaded
        _check_all(pa, ia, _want((rows, cols), (rows, cols), 32))
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ 3. one preparer, several source sizes
def test_a_second_source_size_rebuilds_the_tables_and_calls_repeat():
    dst = (37, 53)
    ctx = srl.Context(0)
    try:
        prep = srl.ImagePrep(ctx, _opts(*dst))
        # general rule, another general rule (larger source: the block grows), the shortcut, the first size again, the plain entry
        for src in ((61, 91), (19, 27), (90, 131), (74, 106), (61, 91)):
            info = prep.prepare_resized(rc.image(src[0], src[1], 33))
            _check_all(prep, info, _want(src, dst, 33))
        first = _all_bytes(prep, info.tiles)
        info = prep.prepare_resized(rc.image(61, 91, 33))
        assert _all_bytes(prep, info.tiles) == first                             # the same bytes call after call
        info = prep.prepare(rc.image(37, 53, 33))
        _check_all(prep, info, _want(dst, dst, 33))
        info = prep.prepare_resized(rc.image(61, 91, 33))                        # ... and the tables are still those of 61 x 91
        assert _all_bytes(prep, info.tiles) == first
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_a_refused_call_leaves_the_prepared_images():
    dst = (37, 53)
    ctx = srl.Context(0)
    try:
        lib = ctx.lib
        src = rc.image(61, 91, 34)
        info = capi.ImagePrepInfo()
        call = lambda img, r, c, stride, inf=None: lib.srl_image_prepare_resized(ctx.h, None if img is None else capi._ptr(img), r, c, stride,      # noqa: E731
                                                                                 None if inf is None else C.byref(inf))
        out = np.zeros(dst + (3,), np.uint8)
        assert call(src, 61, 91, src.strides[0], info) == SRL_ERR_NO_MAP           # no preparer
        assert lib.srl_image_prep_download_resized(ctx.h, capi._ptr(out), out.size) == SRL_ERR_NO_MAP
        prep = srl.ImagePrep(ctx, _opts(*dst))
        assert lib.srl_image_prep_download_resized(ctx.h, capi._ptr(out), out.size) == SRL_ERR_NO_SWEEP      # no image yet
        good = prep.prepare_resized(src)
        before = _all_bytes(prep, good.tiles)
        other = rc.image(19, 27, 34)
        for args in ((other, 19, 27, 3 * 27 - 1), (None, 19, 27, 3 * 27), (other, 0, 27, other.strides[0]), (other, 19, 0, other.strides[0]),
                     (other, -1, 27, other.strides[0]), (other, 16385, 27, other.strides[0]), (other, 19, 16385, 3 * 16385),
                     (other, 8193, 8193, 3 * 8193)):
            C.memset(C.byref(info), 0xFF, C.sizeof(info))
            assert call(*args, info) == SRL_ERR_BAD_ARG and info.as_tuple() == (0,) * 8, args[1:]
        ctx.comm_set_host_callbacks(2, 0, lambda a: None, lambda v: [v, v])       # more than one rank
        assert call(other, 19, 27, other.strides[0], info) == SRL_ERR_UNSUPPORTED and info.as_tuple() == (0,) * 8
        ctx.comm_set_host_callbacks(1, 0, None, None)
        assert lib.srl_image_prep_download_resized(ctx.h, capi._ptr(out), out.size - 1) == SRL_ERR_BAD_ARG
        assert lib.srl_image_prep_download_resized(ctx.h, None, out.size) == SRL_ERR_BAD_ARG
        assert _all_bytes(prep, good.tiles) == before                             # the previous results are still there
        _check_all(prep, good, _want((61, 91), dst, 34))
        info = prep.prepare_resized(other)                                        # and the preparer still works
        _check_all(prep, info, _want((19, 27), dst, 34))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 5. the colour map
def test_the_resized_image_becomes_the_colour_maps():
    import render_checker as rkr
    o = rkr.OPT
    dst = (37, 53)
    ctx = srl.Context(0)
    try:
        ctx.color_map_create(capi.default_color_opts(size_voxel_map=o[0], max_num_points_in_voxel=o[1], min_distance_points=o[2], add_point_step=o[3]))
        prep = srl.ImagePrep(ctx, _opts(*dst))
        info = prep.prepare_resized(rc.image(61, 91, 35))
        assert info.installed_color == 1
        _same("bgr_eq", prep.download(capi.SRL_PREP_BGR_EQ), _want((61, 91), dst, 35)["bgr_eq"])
    finally:
        ctx.close()
