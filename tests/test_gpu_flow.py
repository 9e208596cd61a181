"""The optical flow of the camera stage on the device (srl_flow_track_image: LKOpticalFlowKernel::trackImage, lkpyramid.cpp:755-795)
against the sequential restatement of tests/flow_checker.py and the records of tests/golden/golden_flow.npz (the reference's own compiled
statements, tests/flow_reader.py).  Everything is compared bit for bit: next_xy as raw float bits and status bytewise for ALL points,
failed ones included; every padded level and derivative of both pyramid sets bytewise, borders included."""
import os
import zlib

import numpy as np
import pytest

import flow_checker as fc
import sr_livo_amd as srl
from sr_livo_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRL_ERR_BAD_ARG, SRL_ERR_UNSUPPORTED, SRL_ERR_NO_MAP = -3, -4, -5         # include/srlivo_hip.h: srl_status
COUNTS = (0, 1, 63, 64, 65, 300)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_flow.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def ctx():
    c = srl.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def checked():
    """the checker's answer per scene, computed once"""
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = fc.run_scene(name)
        return memo[name]
    return get


def _same_levels(flow, which, pyr):
    for level in range(pyr.L + 1):
        img, der = flow.download_level(which, level)
        assert img.shape == pyr.image[level].shape and der.shape == pyr.deriv[level].shape
        assert img.tobytes() == pyr.image[level].tobytes(), (which, level, "image")
        assert der.tobytes() == pyr.deriv[level].tobytes(), (which, level, "derivative")


@pytest.mark.parametrize("name", fc.SCENES)
def test_scene_equals_the_checker_and_the_golden_record(ctx, checked, golden, name):
    """sizes 160 x 120 (L = 2), 203 x 157 (odd at every level, L = 2), 233 x 185 (L = 3), 60 x 44 (max_level 3 lowered to 1 and staying
    there); three images in a row where the scene has them: the first call returns 0 with next == prev, the later ones track from the
    stored pyramid and ITS derivatives; the edge-admission scene and every exit class of the crafted scenes"""
    imgs, pts, opts = fc.scene(name)
    want = checked(name)
    flow = srl.Flow(ctx, max_level=opts.max_level, max_count=opts.max_count, epsilon=opts.epsilon, min_eig_threshold=opts.min_eig_threshold)
    try:
        for k, im in enumerate(imgs):
            nxt, status, nt = flow.track_image(im, pts)
            w_next, w_status, w_nt, w_pyr = want[k]
            assert flow.levels() == w_pyr.L == int(golden[f"{name}/L"])
            if k == 0:
                assert nt == 0 and _bits(nxt).tobytes() == _bits(pts).tobytes() and not status.any()
            else:
                bad = np.flatnonzero((_bits(nxt) != _bits(w_next)).any(axis=1) | (status != w_status))
                assert bad.size == 0, (name, k, bad[:8], nxt[bad[:8]], w_next[bad[:8]], status[bad[:8]], w_status[bad[:8]])
                assert nt == w_nt == int(w_status.sum())
                assert np.array_equal(_bits(nxt), golden[f"{name}/next{k}"]) and np.array_equal(status, golden[f"{name}/status{k}"])
            # after the swap: the set called prev holds the image just given, the other one the image before it
            _same_levels(flow, capi.SRL_FLOW_PREV, w_pyr)
            if k:
                _same_levels(flow, capi.SRL_FLOW_CUR, want[k - 1][3])
            ic, dc = w_pyr.crcs()
            assert np.array_equal(ic, golden[f"{name}/image_crc{k}"]) and np.array_equal(dc, golden[f"{name}/deriv_crc{k}"])
    finally:
        flow.close()


@pytest.fixture(scope="module")
def many_points():
    """300 points on the 160 x 120 scene, a tenth of them around the rim and beyond it; points are independent, so the first n of the
    checker's answer are the answer for the first n"""
    imgs, _, opts = fc.scene("shift_160x120")
    pts = fc.grid_points(17, 120 + 60, 160 + 60, 300) - np.float32(30.0)
    pts[::10] = fc.grid_points(18, 120, 160, 30)
    tr = fc.Tracker(opts)
    tr.track_image(imgs[0], pts)
    nxt, status, _ = tr.track_image(imgs[1], pts)
    assert 0 < status.sum() < 300
    return imgs, pts, nxt, status


@pytest.mark.parametrize("n", COUNTS)
def test_point_counts(ctx, many_points, n):
    imgs, pts, w_next, w_status = many_points
    flow = srl.Flow(ctx)
    try:
        flow.track_image(imgs[0], pts[:n])
        nxt, status, nt = flow.track_image(imgs[1], pts[:n])
        assert nxt.shape == (n, 2) and status.shape == (n,)
        assert _bits(nxt).tobytes() == _bits(w_next[:n]).tobytes() and status.tobytes() == w_status[:n].tobytes()
        assert nt == int(w_status[:n].sum())
    finally:
        flow.close()


def test_third_call_uses_the_second_images_derivatives(ctx, checked):
    """after the swap the stored derivatives are the SECOND image's.  The checker run with the third image's derivatives in their place
    gives another answer (asserted), so a device that used the current image's derivatives would fail here."""
    name = "shift_203x157"
    imgs, pts, opts = fc.scene(name)
    want = checked(name)
    right = want[2]
    second, third = want[1][3], want[2][3]
    wrong_prev = fc.Pyramid(imgs[1], opts.max_level)
    wrong_prev.deriv = third.deriv
    with np.errstate(all="ignore"):
        wrong = np.array([fc.track_point(wrong_prev, third, third.L, p, opts)[:2] for p in pts[:16]], dtype=np.float32)
    assert (_bits(wrong) != _bits(right[0][:16])).any()
    flow = srl.Flow(ctx)
    try:
        for im in imgs[:2]:
            flow.track_image(im, pts)
        nxt, status, _ = flow.track_image(imgs[2], pts)
        assert _bits(nxt).tobytes() == _bits(right[0]).tobytes() and status.tobytes() == right[1].tobytes()
        assert flow.download_level(capi.SRL_FLOW_CUR, 0)[1].tobytes() == second.deriv[0].tobytes()
    finally:
        flow.close()


def test_contract_departures(ctx):
    """a coordinate that is not finite or whose window corner is no int32: status 0 and next = prev, the neighbours untouched by it"""
    imgs, pts, opts = fc.scene("shift_160x120")
    pts = pts[:12].copy()
    odd = {1: (np.nan, 40.0), 3: (50.0, np.inf), 5: (-np.inf, np.nan), 7: (1e12, 30.0), 9: (20.0, -1e12), 11: (3e9, 3e9)}
    for i, v in odd.items():
        pts[i] = v
    tr = fc.Tracker(opts)
    tr.track_image(imgs[0], pts)
    w_next, w_status, _ = tr.track_image(imgs[1], pts)
    for i in odd:
        assert w_status[i] == 0 and _bits(w_next[i]).tobytes() == _bits(pts[i]).tobytes()
    assert w_status[[0, 2, 4, 6, 8, 10]].all()
    flow = srl.Flow(ctx)
    try:
        flow.track_image(imgs[0], pts)
        nxt, status, nt = flow.track_image(imgs[1], pts)
        assert _bits(nxt).tobytes() == _bits(w_next).tobytes() and status.tobytes() == w_status.tobytes() and nt == 6
    finally:
        flow.close()


def test_refusals(ctx):
    imgs, pts, _ = fc.scene("shift_160x120")
    with pytest.raises(srl.SrlError) as e:
        capi.Flow(ctx, win=15)
    assert e.value.status == SRL_ERR_UNSUPPORTED
    for kw in (dict(max_level=4), dict(max_level=-1), dict(max_count=101), dict(epsilon=-1.0), dict(epsilon=float("nan")), dict(min_eig_threshold=float("inf"))):
        with pytest.raises(srl.SrlError) as e:
            capi.Flow(ctx, **kw)
        assert e.value.status == SRL_ERR_BAD_ARG, kw
    nt = capi.C.c_int(7)
    assert ctx.lib.srl_flow_track_image(ctx.h, capi._ptr(imgs[0]), 120, 160, 160, None, 0, None, None, capi.C.byref(nt)) == SRL_ERR_NO_MAP and nt.value == 0
    flow = srl.Flow(ctx)
    try:
        with pytest.raises(srl.SrlError) as e:
            capi.Flow(ctx)                         # one tracker per context
        assert e.value.status == SRL_ERR_BAD_ARG
        flow.track_image(imgs[0], pts)
        with pytest.raises(srl.SrlError) as e:     # the size of the first image holds
            flow.track_image(imgs[1][:, :158], pts)
        assert e.value.status == SRL_ERR_BAD_ARG
        with pytest.raises(srl.SrlError) as e:
            flow.track_image(imgs[1][:118], pts)
        assert e.value.status == SRL_ERR_BAD_ARG
        # the refusal changed nothing: the next call tracks from the first image
        tr = fc.Tracker()
        tr.track_image(imgs[0], pts)
        w_next, w_status, _ = tr.track_image(imgs[1], pts)
        nxt, status, _ = flow.track_image(imgs[1], pts)
        assert _bits(nxt).tobytes() == _bits(w_next).tobytes() and status.tobytes() == w_status.tobytes()
    finally:
        flow.close()


def test_strided_rows_and_determinism(ctx, checked):
    """a gray image whose rows are strided gives what the packed image gives; two runs of the same calls are bytewise equal"""
    name = "shift_233x185"
    imgs, pts, _ = fc.scene(name)
    want = checked(name)
    runs = []
    for strided in (False, True):
        flow = srl.Flow(ctx)
        try:
            out = []
            for im in imgs:
                if strided:
                    wide = np.full((im.shape[0], im.shape[1] + 11), 255, np.uint8)
                    wide[:, :im.shape[1]] = im
                    im = wide[:, :im.shape[1]]
                out.append(flow.track_image(im, pts))
            runs.append(out)
        finally:
            flow.close()
    for k in (1, 2):
        assert _bits(runs[0][k][0]).tobytes() == _bits(runs[1][k][0]).tobytes() == _bits(want[k][0]).tobytes()
        assert runs[0][k][1].tobytes() == runs[1][k][1].tobytes() == want[k][1].tobytes()


def test_host_mirror_forwards_to_the_device(ctx, checked):
    """srl_lk_*: the mirror's LKOpticalFlowKernel with the reference's constructor arguments (opticalFlowTracker.cpp:5-8)"""
    name = "shift_160x120"
    imgs, pts, _ = fc.scene(name)
    want = checked(name)
    lib, Cc = ctx.lib, capi.C
    h = Cc.c_void_p()
    assert lib.srl_lk_create(ctx.h, 21, 21, 3, 3, 10, 0.05, 8, 1e-4, Cc.byref(h)) == 0
    try:
        for k, im in enumerate(imgs):
            nxt, status, nt = np.zeros_like(pts), np.zeros(len(pts), np.uint8), Cc.c_int(-1)
            assert lib.srl_lk_track_image(h, capi._ptr(im), im.shape[0], im.shape[1], im.strides[0], capi._ptr(pts), len(pts), capi._ptr(nxt),
                                          capi._ptr(status), Cc.byref(nt)) == 0
            L = Cc.c_int(-1)
            assert lib.srl_lk_get(h, Cc.byref(L), None, None) == 0 and L.value == 2
            if k == 0:
                assert nt.value == 0 and nxt.tobytes() == pts.tobytes()
            else:
                assert _bits(nxt).tobytes() == _bits(want[k][0]).tobytes() and status.tobytes() == want[k][1].tobytes() and nt.value == want[k][2]
    finally:
        lib.srl_lk_destroy(h)
    assert lib.srl_flow_levels(ctx.h, Cc.byref(Cc.c_int())) == SRL_ERR_NO_MAP      # the handle took its tracker with it
