"""One camera frame end to end on the device (srl_lio_image_process: imageProcessing::process of the host mirror, include/srlivo_host.h)
against the same frame driven CALL BY CALL from this file with the handles that existed before it: ImagePrep, Oft with
use_device_consensus / use_prepared_image, Lio.select_points_for_projection, vio_esikf, vio_photometric,
render_points_in_recent_voxel and update_and_append_track_points, in the order of src/imageProcessing.cpp:89-164.

Every step is specified to give the same bytes call after call, so context A (one call per frame) and context B (piecewise) agree
BYTEWISE after every frame on the 31-double camera state, the 121-double covariance, both pose maps with their flags, the render and
track totals, the refreshed candidates and srl_color_registered_rgb.  No tolerance anywhere.

The scene is render_checker's room under its smaller camera (375 x 500); the frames are one smooth texture displaced by (1, 2) pixels
per frame, in three channels of different gain.  The main case asserts ON B ALONE that at least 30 points survive the flow and at
least 10 survive PnP in every frame after the first: a condition of the scene, not a tolerance -- it keeps the comparison from passing
with both camera updates gated off."""
import ctypes as C
import functools

import numpy as np
import pytest

import color_checker as cc
import flow_checker as fc
import render_checker as rk
import sr_livo_amd as srl
from sr_livo_amd import capi

pytestmark = pytest.mark.gpu
ROWS, COLS = rk.IMAGE_SIZES[1]
CAM = rk.scene_camera(rk.POSES[0], 1)
DIST = (0.02, -0.004, 0.0004, -0.0003, 0.0005)
T0, DT = 10.0, 0.1


@functools.lru_cache(maxsize=None)
def _frames(rows, cols, n):
    """n read-only BGR frames of rows x cols, the content moving by (+2, +1) pixels per frame; row stride 3 cols + 13, padding 0xA5"""
    tex = fc.texture(91, rows, cols)
    out = []
    for k in range(n):
        g = fc.crop(tex, rows, cols, -k, -2 * k).astype(np.int64)
        img = np.clip(np.stack([g, (g * 3) // 4 + 30, 255 - (g * 2) // 3], axis=-1), 0, 255).astype(np.uint8)
        stride = 3 * cols + 13
        buf = np.full(rows * stride, 0xA5, np.uint8)
        view = np.lib.stride_tricks.as_strided(buf, shape=(rows, cols, 3), strides=(stride, 3, 1))
        view[...] = img
        view.setflags(write=False)
        buf.setflags(write=False)
        out.append(view)
    return tuple(out)


def _camera(state31, margin):
    s = state31
    return capi.ColorCamera((C.c_double * 4)(*s[17:21]), (C.c_double * 3)(*s[21:24]), s[13], s[14], s[15], s[16], margin)


def _lio(width, height, ratio, window, maximum):
    """a handle with the room's first two sweeps in its colour map (the second with to_rendering), the scene's camera as its camera
    state, and the options of both paths"""
    lio = srl.Lio(0)
    o = rk.OPT
    lio.set_color_map_options(capi.default_color_opts(size_voxel_map=o[0], max_num_points_in_voxel=o[1], min_distance_points=o[2], add_point_step=o[3]))
    for j in range(2):
        lio.add_points_to_map_at(cc.scene_batch(j), rk.BATCH_TIMES[j], to_rendering=(j == 1))
    K = np.array([[CAM.fx, 0, CAM.cx], [0, CAM.fy, CAM.cy], [0, 0, 1.0]])
    lio.vio_set_options(2, True, True, K, np.eye(3), np.zeros(3))
    s = np.zeros(31)
    s[1:10] = np.eye(3).ravel()
    s[13:17] = CAM.fx, CAM.fy, CAM.cx, CAM.cy
    s[17:21], s[21:24] = CAM.q, CAM.t
    s[24:28], s[28:31] = CAM.q, CAM.t
    lio.vio_set_camera_state(s)
    lio.image_set_options(image_width=width, image_height=height, image_resize_ratio=ratio, dist=DIST, track_windows_size=window,
                          maximum_tracked_points=maximum)
    return lio


class Piecewise:
    """imageProcessing::process written out in Python over the handles that existed before srl_lio_image_process"""

    def __init__(self, lio, width, height, ratio, window, maximum):
        self.lio, self.width, self.height, self.ratio, self.window, self.maximum = lio, width, height, ratio, window, maximum
        self.first_data, self.updated_frame_index, self.candidates = True, -1, np.zeros(0, capi.COLOR_SELECTED_DTYPE)
        self.k = [CAM.fx, CAM.fy, CAM.cx, CAM.cy]

    def frame(self, raw, t, frame_id):
        lio, rows, cols = self.lio, raw.shape[0], raw.shape[1]
        if self.first_data:                                                 # :91-111
            self.scale = self.width * self.ratio / cols
            self.k = [v / self.scale for v in self.k]
            self.size = (int(self.height / self.scale), int(self.width / self.scale))
            self.prep = srl.ImagePrep(lio.ctx, capi.default_image_prep_opts(rows=self.size[0], cols=self.size[1], fx=self.k[0], fy=self.k[1], cx=self.k[2],
                                                                            cy=self.k[3], dist=list(DIST)))
            self.oft = srl.Oft(lio.ctx)
            self.oft.use_device_consensus(self.k)
            self.oft.use_prepared_image(True)
            self.oft.set_maximum_tracked_points(self.maximum)
        if abs(self.ratio - 1.0) > 1e-6:                                    # :113-125
            self.prep.prepare_resized(raw)
        else:
            self.prep.prepare(raw)
        if self.first_data:                                                 # :127-135
            sel, _ = lio.select_points_for_projection(_camera(lio.vio_get_camera_state(), 0.005), rows, cols, self.window / self.scale, 1)
            self.oft.init(sel, None, t)
            self.first_data = False
        out = {}
        out["after_flow"] = self.oft.track_image(None, t, rows, cols)     # :137
        out["accepted"] = self.oft.remove_outlier_using_ransac_pnp(1)       # :141
        out["after_pnp"] = self.oft.sizes()[1]
        new_voxels = lio.color_visited(1)[1]
        if out["accepted"]:                                                 # :149-153
            out["esikf"] = lio.vio_esikf(self.oft.tracked_for_vio(), new_voxels)[0::2]
            out["photometric"] = lio.vio_photometric(self.oft.tracked_for_vio(), new_voxels)[0::2]
        state = lio.vio_get_camera_state()
        out["render"] = lio.render_points_in_recent_voxel(_camera(state, 0.005), t).as_tuple()      # :155
        if frame_id != self.updated_frame_index:                            # :157-159
            self.candidates, _ = lio.refresh_points_for_projection(_camera(state, -0.4), rows, cols)
            self.updated_frame_index = frame_id
        out["track"] = self.oft.update_and_append_track_points(_camera(state, 0.005), rows, cols, self.candidates, self.window / self.scale).as_tuple()      # :161
        return out

    def close(self):
        if not self.first_data:
            self.oft.close()
            self.prep.close()


def _rgb_bytes(lio):
    return tuple(a.tobytes() for a in lio.ctx.color_registered_rgb())


def _run(raw_size, width, height, ratio, window, maximum, n_frames, frame_ids=None):
    """both contexts over the frames; returns B's per-frame records and A's results after asserting that they agree bytewise"""
    frames = _frames(raw_size[0], raw_size[1], n_frames)
    a, b = _lio(width, height, ratio, window, maximum), _lio(width, height, ratio, window, maximum)
    piecewise = Piecewise(b, width, height, ratio, window, maximum)
    records = []
    try:
        assert _rgb_bytes(a) == _rgb_bytes(b)
        for k, raw in enumerate(frames):
            t, fid = T0 + DT * k, (frame_ids[k] if frame_ids else k + 1)
            want = piecewise.frame(raw, t, fid)
            r = a.image_process(raw, t, fid)
            print(f"frame {k}: B after flow {want['after_flow']}, after PnP {want['after_pnp']}, accepted {want['accepted']}, "
                  f"updates {want.get('esikf')} {want.get('photometric')}, render {want['render']}, candidates {len(piecewise.candidates)}")
            assert (r.first_data, r.prepared_rows, r.prepared_cols, r.image_scale_factor) == (int(k == 0),) + piecewise.size + (piecewise.scale,)
            assert (r.tracked_after_flow, r.tracked_after_pnp, bool(r.pnp_accepted)) == (want["after_flow"], want["after_pnp"], want["accepted"])
            if want["accepted"]:
                assert (bool(r.esikf_accepted), r.esikf_used) == want["esikf"] and (bool(r.photometric_accepted), r.photometric_used) == want["photometric"]
            else:
                assert (r.esikf_accepted, r.esikf_iterations, r.photometric_accepted, r.photometric_iterations) == (0, 0, 0, 0)
            assert r.render.as_tuple() == want["render"] and r.track.as_tuple() == want["track"]
            assert a.vio_get_camera_state().tobytes() == b.vio_get_camera_state().tobytes()
            assert a.vio_get_cov().tobytes() == b.vio_get_cov().tobytes()
            oa = a.image_oft()
            for which in (0, 1):
                assert oa.pose_map(which).tobytes() == piecewise.oft.pose_map(which).tobytes(), (k, which)
            assert oa.sizes() == piecewise.oft.sizes() and oa.times() == piecewise.oft.times()
            assert a.image_candidates().tobytes() == piecewise.candidates.tobytes() and r.refreshed_candidates == len(piecewise.candidates)
            assert _rgb_bytes(a) == _rgb_bytes(b)
            assert a.image_time_last_process() == t
            # the prepared images are the same, too
            pa = np.zeros(piecewise.size, np.uint8)
            assert a.lib.srl_image_prep_download(a.ctx.h, 0, capi._ptr(pa), pa.strides[0]) == capi.SRL_OK
            assert pa.tobytes() == piecewise.prep.download(capi.SRL_PREP_GRAY_EQ).tobytes()
            records.append((want, r))
        return records
    finally:
        piecewise.close()
        a.close()
        b.close()


def test_four_frames_equal_the_piecewise_sequence_with_both_updates_running():
    records = _run((ROWS, COLS), COLS, ROWS, 1.0, 40.0, 300, 4)
    for k, (want, r) in enumerate(records[1:], 1):
        # the condition on B alone: the flow and PnP leave enough points for both camera updates to run
        assert want["after_flow"] >= 30 and want["after_pnp"] >= 10 and want["accepted"], (k, want)
        assert want["esikf"][0] and want["photometric"][0] and want["esikf"][1] >= 10, (k, want)
        assert r.esikf_iterations >= 1
    # the photometric update uses a point only once it has been rendered often enough: by the last frame it moves the state, too
    assert records[-1][0]["photometric"][1] >= 10 and records[-1][1].photometric_iterations >= 1
    assert records[0][1].render.first > 100 and all(w["track"][1] + w["track"][12] > 30 for w, _ in records)      # colours were written, the set is topped up


def test_a_repeated_frame_id_keeps_the_candidates_on_both_sides():
    _run((ROWS, COLS), COLS, ROWS, 1.0, 40.0, 300, 3, frame_ids=(5, 5, 6))


def test_a_resize_ratio_crosses_the_device_resize_inside_the_loop():
    # image_resize_ratio 0.5 on a frame of half the configured size: image_scale_factor is 1.0, the intrinsics stay the scene's, and the
    # preparer's 375 x 500 is twice the frame that arrives (srl_image_prepare_resized, the general rule: 375 is not 2 x 187)
    records = _run((187, 250), COLS, ROWS, 0.5, 12.0, 300, 3)
    assert all((r.prepared_rows, r.prepared_cols, r.image_scale_factor) == (ROWS, COLS, 1.0) for _, r in records)
    assert any(w["accepted"] and r.esikf_iterations >= 1 for w, r in records[1:])      # a camera update ran behind the resize


def test_a_ratio_of_two_crosses_the_exact_half_shortcut_inside_the_loop():
    # image_resize_ratio 2.0 on a frame of twice the configured size: image_scale_factor 1.0 again, the preparer's 375 x 500 is exactly
    # half the 750 x 1000 that arrives (the 2 x 2 box mean), and the projection tests run on the raw frame's 750 x 1000
    records = _run((2 * ROWS, 2 * COLS), COLS, ROWS, 2.0, 40.0, 300, 3)
    assert all((r.prepared_rows, r.prepared_cols, r.image_scale_factor) == (ROWS, COLS, 1.0) for _, r in records)
    assert any(w["accepted"] and r.esikf_iterations >= 1 for w, r in records[1:])      # a camera update ran behind the resize


def test_only_the_two_consensus_steps_replaced_hold_from_the_first_frame_and_go_back():
    """a step table with nothing but `fundamental` and `pnp` on a device handle: the caller's functions are what the tracker calls on the
    FIRST frame already, behind the default consensus setup (which installs the device's estimators), the device's never run; with the
    table taken away again the device's estimators are back"""
    frames = _frames(ROWS, COLS, 3)
    lio = _lio(COLS, ROWS, 1.0, 40.0, 300)
    calls = {"fundamental": 0, "pnp": 0}

    def fundamental(last, cur, n, status, user):
        calls["fundamental"] += 1
        C.memset(status, 1, n)
        return 0

    def pnp(xyz, uv, n, inliers, n_inliers, user):
        calls["pnp"] += 1
        np.frombuffer((C.c_int32 * n).from_address(inliers), np.int32)[:] = np.arange(n)
        n_inliers[0] = n
        return 0
    steps = capi.ImageProcessSteps()
    steps.fundamental, steps.pnp = capi.OFT_FUNDAMENTAL_PROVIDER_FN(fundamental), capi.OFT_PNP_PROVIDER_FN(pnp)
    try:
        lio.image_set_steps(steps)
        oft = lio.image_oft()
        for k in range(2):
            r = lio.image_process(frames[k], T0 + DT * k, k + 1)
            assert calls == {"fundamental": k + 1, "pnp": k + 1}, (k, calls)
            assert r.tracked_after_flow >= 30 and r.tracked_after_pnp == r.tracked_after_flow and r.pnp_accepted      # all ones, all inliers
            for which in (0, 1):
                assert bytes(oft.last_consensus(which)) == bytes(C.sizeof(capi.ConsensusResult)), (k, which)      # the device's never ran
        lio.image_set_steps(None)
        r = lio.image_process(frames[2], T0 + DT * 2, 3)
        assert calls == {"fundamental": 2, "pnp": 2} and r.tracked_after_flow >= 30 and r.pnp_accepted
        for which in (0, 1):
            assert bytes(oft.last_consensus(which)) != bytes(C.sizeof(capi.ConsensusResult)), which
    finally:
        lio.close()


def test_five_tracked_points_cross_the_gate_of_ten():
    records = _run((ROWS, COLS), COLS, ROWS, 1.0, 170.0, 5, 3)
    for want, r in records:
        assert not want["accepted"] and want["after_pnp"] < 10 and (r.esikf_accepted, r.photometric_accepted) == (0, 0)
        assert r.render.listed > 0 and want["track"][1] + want["track"][12] <= 9      # the render and the top-up still run
