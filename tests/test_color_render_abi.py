"""srl_color_image_upload / srl_color_map_render / srl_color_map_download_rgb / srl_color_registered_rgb and the host handle's
srl_lio_render_points_in_recent_voxel (rgbMapTracker::renderPointsInRecentVoxel, rgbMapTracker.cpp:176-237) on a box without a GPU: the
entry points are declared and exported, the records have one layout on both sides, and the refusals that are decided before a device is
touched are returned without one, with the totals written as 0."""
import ctypes as C
import os
import re

import numpy as np

import render_checker as rk
import sr_livo_amd as srl
from sr_livo_amd import capi

SRL_ERR_BAD_ARG = -3          # include/srlivo_hip.h: srl_status
NEW = ("srl_color_image_upload", "srl_color_map_render", "srl_color_map_download_rgb", "srl_color_registered_rgb",
       "srl_lio_render_points_in_recent_voxel")
CSRC = os.path.join(os.path.dirname(capi.INCLUDE_DIR), "sr_livo_amd", "csrc")


def _camera():
    c = rk.scene_camera(rk.POSES[0], 0)
    return capi.ColorCamera((C.c_double * 4)(*c.q), (C.c_double * 3)(*c.t), c.fx, c.fy, c.cx, c.cy, c.fov_margin)


def test_render_entry_points_are_declared_and_exported():
    lib = srl.load_library()
    for name in NEW:
        assert name in srl.declared_symbols()
        assert hasattr(lib, name)
    hip = open(os.path.join(capi.INCLUDE_DIR, "srlivo_hip.h")).read()
    host = open(os.path.join(capi.INCLUDE_DIR, "srlivo_host.h")).read()
    for name in NEW[:4]:
        assert re.search(r"\bint " + name + r"\(srl_ctx \*ctx", hip), name
    assert re.search(r"\bint srl_lio_render_points_in_recent_voxel\(srl_lio \*lio", host)
    # the signatures of the existing downloads did not change
    assert "int srl_color_map_download(srl_ctx *ctx, int16_t *keys_xyz, int32_t *counts, double *last_visited_time, int max_voxels," in hip
    assert "int srl_color_registered_download(srl_ctx *ctx, int64_t first, int count, srl_color_stored *out);" in hip


def test_records_have_one_layout_on_both_sides():
    hip = open(os.path.join(capi.INCLUDE_DIR, "srlivo_hip.h")).read()
    assert C.sizeof(capi.ColorCamera) == 12 * 8 and C.sizeof(capi.ColorRenderTotals) == 7 * 8
    m = re.search(r"typedef struct srl_color_camera \{(.*?)\} srl_color_camera;", hip, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = re.findall(r"\b([a-z_]+)(?:\[\d\])?\s*[,;]", body)
    assert tuple(names) == tuple(f for f, _ in capi.ColorCamera._fields_)
    m = re.search(r"typedef struct srl_color_render_totals \{(.*?)\} srl_color_render_totals;", hip, re.S)
    names = re.findall(r"\b([a-z_]+)\s*[,;]", m.group(1))
    assert tuple(names) == tuple(f for f, _ in capi.ColorRenderTotals._fields_) == rk.TOTALS
    # the state record: a NEW array parallel to the point pool, 40 bytes per stored point; the existing layouts are as they were
    layout = open(os.path.join(CSRC, "srl_color_map.h")).read()
    assert "struct SrlColorState { double observe_distance; double last_observe_time; float cov_rgb[3]; short rgb[3]; short n_rgb; };" in layout
    assert "static_assert(sizeof(SrlColorState) == 40" in layout
    assert "struct SrlColorPoint { float x, y, z; int voxel; int slot; int reg; };" in layout
    assert "sizeof(SrlColorVoxel) == 24 && sizeof(SrlColorPoint) == 24 && sizeof(SrlColorSlot) == 16 && sizeof(SrlGridCell) == 16" in \
        open(os.path.join(CSRC, "srl_color_kernels.hip")).read()
    state = np.dtype([("observe_distance", "<f8"), ("last_observe_time", "<f8"), ("cov_rgb", "<f4", 3), ("rgb", "<i2", 3), ("n_rgb", "<i2")], align=True)
    assert state.itemsize == 40
    # the render kernels are compiled without contraction like the rest of the library
    assert "-ffp-contract=off" in open(os.path.join(CSRC, "Makefile")).read()


def test_refusals_without_a_device_zero_the_totals():
    lib = srl.load_library()
    cam = _camera()
    voxels = np.zeros((2, 3), np.int32)
    tot = capi.ColorRenderTotals(7, 7, 7, 7, 7, 7, 7)
    assert lib.srl_color_map_render(None, C.byref(cam), capi._ptr(voxels), 2, 1.0, C.byref(tot)) == SRL_ERR_BAD_ARG
    assert tot.as_tuple() == (0,) * 7
    assert lib.srl_color_map_render(None, None, None, 0, 1.0, None) == SRL_ERR_BAD_ARG
    img = rk.scene_image(1)
    assert lib.srl_color_image_upload(None, capi._ptr(img), img.shape[0], img.shape[1], img.strides[0]) == SRL_ERR_BAD_ARG
    rgb = np.full((2, 3), 9, np.int16)
    assert lib.srl_color_map_download_rgb(None, capi._ptr(rgb), None, None, None, None, 2) == SRL_ERR_BAD_ARG
    assert lib.srl_color_registered_rgb(None, 0, 2, capi._ptr(rgb), None, None, None, None) == SRL_ERR_BAD_ARG
    assert (rgb == 9).all()
    tot = capi.ColorRenderTotals(7, 7, 7, 7, 7, 7, 7)
    assert lib.srl_lio_render_points_in_recent_voxel(None, C.byref(cam), 1.0, C.byref(tot)) == SRL_ERR_BAD_ARG and tot.as_tuple() == (0,) * 7


def test_host_only_handle_has_no_render():
    lib = srl.load_library()
    h = C.c_void_p()
    assert lib.srl_lio_create(-1, C.byref(h)) == capi.SRL_OK        # host-only object: no device behind it
    try:
        cam = _camera()
        tot = capi.ColorRenderTotals(7, 7, 7, 7, 7, 7, 7)
        assert lib.srl_lio_render_points_in_recent_voxel(h, C.byref(cam), 1.0, C.byref(tot)) == capi.SRL_ERR_NO_DEVICE      # an error, never a host-side loop
        assert tot.as_tuple() == (0,) * 7
        assert lib.srl_lio_render_points_in_recent_voxel(h, None, 1.0, None) == SRL_ERR_BAD_ARG
        assert not lib.srl_lio_ctx(h)
    finally:
        lib.srl_lio_destroy(h)


def test_the_wrappers_hold_no_arithmetic_of_the_path():
    """the camera goes to the library as the caller gave it: pose inversion, bounds and rounding live behind the C-ABI"""
    c = rk.scene_camera(rk.POSES[3], 1)
    cam = capi.ColorCamera((C.c_double * 4)(*c.q), (C.c_double * 3)(*c.t), c.fx, c.fy, c.cx, c.cy, c.fov_margin)
    assert tuple(cam.q_world_camera) == c.q and tuple(cam.t_world_camera) == c.t and cam.fov_margin == 0.005
