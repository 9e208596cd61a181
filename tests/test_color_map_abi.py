"""srl_color_map_* / srl_lio_*color* (addPointToColorMap, lioOptimization.cpp:448-518) on a box without a GPU: the entry points are declared
and exported, the option defaults are the effective yaml values, the records have the same layout on both sides, NULL and bad arguments
are refused before anything touches a device with the counts written as 0, and a host-only handle has no colour map and no host-side
insertion."""
import ctypes as C
import os
import re

import numpy as np

import color_checker as cc
import sr_livo_amd as srl
from sr_livo_amd import capi

SRL_ERR_BAD_ARG = -3          # include/srlivo_hip.h: srl_status
NEW = ("srl_color_opts_default", "srl_color_map_create", "srl_color_map_destroy", "srl_color_map_insert", "srl_color_map_size",
       "srl_color_map_download", "srl_color_registered_download", "srl_debug_color_map_rebuilds", "srl_lio_set_color_map_options",
       "srl_lio_set_color_times", "srl_lio_add_points_to_map_at", "srl_lio_color_visited", "srl_lio_color_stored")


def test_colour_entry_points_are_declared_and_exported():
    lib = srl.load_library()
    for name in NEW:
        assert name in srl.declared_symbols()
        assert hasattr(lib, name)


def test_option_defaults_are_the_effective_yaml_values():
    o = capi.default_color_opts()
    assert (o.size_voxel_map, o.max_num_points_in_voxel, o.min_distance_points, o.add_point_step) == (0.1, 50, 0.01, 1)
    assert cc.OPTION_SETS[0] == (0.1, 50, 0.01, 1)
    srl.load_library().srl_color_opts_default(None)          # tolerated


def test_records_have_one_layout_on_both_sides():
    assert capi.COLOR_STORED_DTYPE.itemsize == 28 and capi.COLOR_STORED_DTYPE == cc.STORED_DTYPE
    assert C.sizeof(capi.ColorTotals) == 16 and C.sizeof(capi.ColorOpts) == 32
    text = open(os.path.join(capi.INCLUDE_DIR, "srlivo_hip.h")).read()
    m = re.search(r"typedef struct srl_color_stored \{(.*?)\} srl_color_stored;", text, re.S)
    names = re.findall(r"\b([a-z_]+)\s*[,;]", m.group(1))
    assert tuple(names) == capi.COLOR_STORED_DTYPE.names
    src = open(os.path.join(os.path.dirname(capi.INCLUDE_DIR), "sr_livo_amd", "csrc", "srl_color_kernels.hip")).read()
    assert "static_assert(sizeof(srl_color_stored) == 28" in src
    # bytes per voxel / stored point / table slot do not depend on the cap
    assert "sizeof(SrlColorVoxel) == 24 && sizeof(SrlColorPoint) == 24 && sizeof(SrlColorSlot) == 16 && sizeof(SrlGridCell) == 16" in src
    limit = int(re.search(r"#define SRL_COLOR_MAP_INSERT_MAX_POINTS (\d+)", text).group(1))
    assert limit == 1_048_576


def test_null_arguments_are_refused_without_a_device_and_zero_the_counts():
    lib = srl.load_library()
    pts = np.zeros((4, 3))
    outcome = np.full(4, 9, np.uint8)
    stored = np.zeros(4, capi.COLOR_STORED_DTYPE)
    visited = np.full((4, 3), 9, np.int32)
    tot = capi.ColorTotals(7, 7, 7, 7)
    assert lib.srl_color_map_insert(None, capi._ptr(pts), 4, 1.0, 0.0, capi._ptr(outcome), capi._ptr(stored), 4, capi._ptr(visited), 4, C.byref(tot)) == SRL_ERR_BAD_ARG
    assert (tot.stored, tot.created, tot.registered, tot.visited) == (0, 0, 0, 0)
    assert lib.srl_color_map_insert(None, None, 0, 1.0, 0.0, None, None, 0, None, 0, None) == SRL_ERR_BAD_ARG
    assert (outcome == 9).all() and (visited == 9).all()
    assert lib.srl_color_map_create(None, C.byref(capi.default_color_opts())) == SRL_ERR_BAD_ARG
    assert lib.srl_color_map_create(None, None) == SRL_ERR_BAD_ARG
    assert lib.srl_color_map_destroy(None) == SRL_ERR_BAD_ARG
    a, b, c, d = C.c_int64(7), C.c_int32(7), C.c_int64(7), C.c_int64(7)
    assert lib.srl_color_map_size(None, C.byref(a), C.byref(b), C.byref(c), C.byref(d)) == SRL_ERR_BAD_ARG
    assert (a.value, b.value, c.value, d.value) == (0, 0, 0, 0)
    assert lib.srl_color_map_download(None, None, None, None, 0, None, None, 0) == SRL_ERR_BAD_ARG
    assert lib.srl_color_registered_download(None, 0, 0, None) == SRL_ERR_BAD_ARG
    assert lib.srl_debug_color_map_rebuilds(None, None, None) == SRL_ERR_BAD_ARG
    n, new = C.c_int(7), C.c_int(7)
    assert lib.srl_lio_color_visited(None, 0, None, 0, C.byref(n), C.byref(new)) == SRL_ERR_BAD_ARG and (n.value, new.value) == (0, 0)
    n.value = 7
    assert lib.srl_lio_color_stored(None, None, 0, C.byref(n)) == SRL_ERR_BAD_ARG and n.value == 0
    assert lib.srl_lio_set_color_map_options(None, None) == SRL_ERR_BAD_ARG
    assert lib.srl_lio_set_color_times(None, 0.0, 0.0, 0) == SRL_ERR_BAD_ARG
    assert lib.srl_lio_add_points_to_map_at(None, capi._ptr(pts), 4, 1.0, 20, 0.1, 0, 1.0, 0) == SRL_ERR_BAD_ARG


def test_host_only_handle_has_no_colour_map_and_no_host_side_insert():
    lib = srl.load_library()
    h = C.c_void_p()
    assert lib.srl_lio_create(-1, C.byref(h)) == capi.SRL_OK        # host-only object: no device behind it
    try:
        assert lib.srl_lio_set_color_map_options(h, None) == capi.SRL_ERR_NO_DEVICE
        assert lib.srl_lio_set_color_map_options(h, C.byref(capi.default_color_opts())) == capi.SRL_ERR_NO_DEVICE
        assert lib.srl_lio_set_color_times(h, 0.0, 1.0, 1) == capi.SRL_OK
        pts = np.array([[0.1, 0.1, 0.1], [0.4, 0.1, 0.1]])
        assert lib.srl_lio_add_points_to_map_at(h, capi._ptr(pts), 2, 1.0, 20, 0.1, 0, 1.0, 1) != capi.SRL_OK      # an error, never a host-side insert
        n, new = C.c_int(7), C.c_int(7)
        out = np.zeros((2, 3), np.int32)
        assert lib.srl_lio_color_visited(h, 0, capi._ptr(out), 2, C.byref(n), C.byref(new)) == capi.SRL_ERR_NO_DEVICE and n.value == 0
        rec = np.zeros(2, capi.COLOR_STORED_DTYPE)
        n.value = 7
        assert lib.srl_lio_color_stored(h, capi._ptr(rec), 2, C.byref(n)) == capi.SRL_ERR_NO_DEVICE and n.value == 0
        assert lib.srl_lio_color_visited(h, 2, None, 0, C.byref(n), None) == SRL_ERR_BAD_ARG
    finally:
        lib.srl_lio_destroy(h)
