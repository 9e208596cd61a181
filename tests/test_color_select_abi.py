"""srl_color_map_select and the host handle's srl_lio_select_points_for_projection (rgbMapTracker::selectPointsForProjection,
rgbMapTracker.cpp:45-152) on a box without a GPU: the entry points are declared and exported, the records have one layout on both sides,
the defaults are the reference's, and the refusals that can be reached without a context are returned with the totals written as 0.  (The
refusals that need a context -- options, image size, camera, no map, more than one rank -- are decided before a device is touched too;
a context exists only on a device: tests/test_gpu_color_select.py::test_refusals_leave_the_totals_zero.)"""
import ctypes as C
import os
import re

import numpy as np

import render_checker as rk
import select_checker as sk
import sr_livo_amd as srl
from sr_livo_amd import capi

SRL_ERR_BAD_ARG = -3          # include/srlivo_hip.h: srl_status
NEW = ("srl_color_map_select", "srl_color_select_opts_default", "srl_lio_select_points_for_projection")
CSRC = os.path.join(os.path.dirname(capi.INCLUDE_DIR), "sr_livo_amd", "csrc")


def _camera():
    c = rk.scene_camera(rk.POSES[0], 0)
    return capi.ColorCamera((C.c_double * 4)(*c.q), (C.c_double * 3)(*c.t), c.fx, c.fy, c.cx, c.cy, c.fov_margin)


def test_select_entry_points_are_declared_and_exported():
    lib = srl.load_library()
    for name in NEW:
        assert name in srl.declared_symbols()
        assert hasattr(lib, name)
    hip = open(os.path.join(capi.INCLUDE_DIR, "srlivo_hip.h")).read()
    host = open(os.path.join(capi.INCLUDE_DIR, "srlivo_host.h")).read()
    assert re.search(r"\bint srl_color_map_select\(srl_ctx \*ctx, const srl_color_camera \*cam, int image_rows, int image_cols,", hip)
    assert re.search(r"\bint srl_lio_select_points_for_projection\(srl_lio \*lio", host)
    # the function is no longer named as the caller's
    assert "vioPhotometric, selectPointsForProjection" not in hip
    # the signatures of the render did not change
    assert "int srl_color_map_render(srl_ctx *ctx, const srl_color_camera *cam, const int32_t *voxels_xyz, int n_voxels, double obs_time," in hip


def _fields(header, struct):
    m = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", header, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return tuple(re.findall(r"\b([a-z_]+)\s*[,;]", body))


def test_records_have_one_layout_on_both_sides():
    hip = open(os.path.join(capi.INCLUDE_DIR, "srlivo_hip.h")).read()
    assert C.sizeof(capi.ColorSelectOpts) == 32 and C.sizeof(capi.ColorSelectTotals) == 64 and capi.COLOR_SELECTED_DTYPE.itemsize == 32
    assert _fields(hip, "srl_color_select_opts") == tuple(f for f, _ in capi.ColorSelectOpts._fields_)
    assert _fields(hip, "srl_color_select_totals") == tuple(f for f, _ in capi.ColorSelectTotals._fields_) == sk.TOTALS
    assert _fields(hip, "srl_color_selected") == capi.COLOR_SELECTED_DTYPE.names == sk.SELECTED_DTYPE.names
    assert capi.COLOR_SELECTED_DTYPE == sk.SELECTED_DTYPE
    assert "static_assert(sizeof(srl_color_selected) == 32" in open(os.path.join(CSRC, "srl_color_select.hip")).read()
    # the map's layouts are as they were: the tail array and the cell table are the selection's own
    layout = open(os.path.join(CSRC, "srl_color_map.h")).read()
    assert "struct SrlColorVoxel { unsigned long long key; double last_visited_time; unsigned count; unsigned pad; };" in layout
    assert "struct SrlColorPoint { float x, y, z; int voxel; int slot; int reg; };" in layout
    # one projection for the render and the selection
    shared = open(os.path.join(CSRC, "srl_color_project.h")).read()
    assert "srl_color_project(" in shared and "zc < 0.001" in shared
    for name in ("srl_color_render.hip", "srl_color_select.hip"):
        text = open(os.path.join(CSRC, name)).read()
        assert "srl_color_project(" in text and "zc < 0.001" not in text, name


def test_the_defaults_are_the_references():
    o = capi.default_color_select_opts()
    assert (o.minimum_dis, o.skip_step, o.use_all_points, o.minimum_depth, o.maximum_depth) == (10.0, 1, 0, 0.1, 200.0)
    assert (sk.MINIMUM_DEPTH, sk.MAXIMUM_DEPTH) == (0.1, 200.0)
    srl.load_library().srl_color_select_opts_default(None)                 # a NULL is ignored
    assert "double minimum_depth_for_projection = 0.1;" in open(os.path.join(CSRC, "host", "lioOptimization.h")).read()
    assert "double maximum_depth_for_projection = 200;" in open(os.path.join(CSRC, "host", "lioOptimization.h")).read()


def test_refusals_without_a_context_zero_the_totals():
    lib = srl.load_library()
    cam, o = _camera(), capi.default_color_select_opts()
    voxels = np.zeros((2, 3), np.int32)
    out = np.full(4, 9, capi.COLOR_SELECTED_DTYPE)
    tot = capi.ColorSelectTotals(7, 7, 7, 7, 7, 7, 7, 7)
    assert lib.srl_color_map_select(None, C.byref(cam), 480, 640, capi._ptr(voxels), 2, C.byref(o), capi._ptr(out), 4, C.byref(tot)) == SRL_ERR_BAD_ARG
    assert tot.as_tuple() == (0,) * 8 and (out["index"] == 9).all()
    assert lib.srl_color_map_select(None, None, 480, 640, None, 0, None, None, 0, None) == SRL_ERR_BAD_ARG
    n = C.c_int(5)
    tot = capi.ColorSelectTotals(7, 7, 7, 7, 7, 7, 7, 7)
    assert lib.srl_lio_select_points_for_projection(None, C.byref(cam), 480, 640, 10.0, 1, 0, 0, None, 0, C.byref(n), C.byref(tot)) == SRL_ERR_BAD_ARG
    assert n.value == 0 and tot.as_tuple() == (0,) * 8


def test_host_only_handle_has_no_selection():
    lib = srl.load_library()
    h = C.c_void_p()
    assert lib.srl_lio_create(-1, C.byref(h)) == capi.SRL_OK        # host-only object: no device behind it
    try:
        cam = _camera()
        n = C.c_int(5)
        tot = capi.ColorSelectTotals(7, 7, 7, 7, 7, 7, 7, 7)
        for refresh in (0, 1):
            assert lib.srl_lio_select_points_for_projection(h, C.byref(cam), 480, 640, 10.0, 1, 0, refresh, None, 0, C.byref(n), C.byref(tot)) == \
                capi.SRL_ERR_NO_DEVICE                                      # an error, never a host-side loop
            assert n.value == 0 and tot.as_tuple() == (0,) * 8
        assert lib.srl_lio_select_points_for_projection(h, None, 480, 640, 10.0, 1, 0, 0, None, 0, C.byref(n), None) == SRL_ERR_BAD_ARG
        assert lib.srl_lio_select_points_for_projection(h, C.byref(cam), 480, 640, 10.0, 1, 0, 0, None, 0, None, None) == SRL_ERR_BAD_ARG
        assert lib.srl_lio_select_points_for_projection(h, C.byref(cam), 480, 640, 10.0, 1, 0, 0, None, 3, C.byref(n), None) == SRL_ERR_BAD_ARG
    finally:
        lib.srl_lio_destroy(h)
