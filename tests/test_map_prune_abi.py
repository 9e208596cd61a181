"""srl_map_remove_far / srl_lio_remove_points_far_from_location (removePointsFarFromLocation, lioOptimization.cpp:556-572) on a box
without a GPU: both entry points are exported, and a NULL context, handle or location is refused before anything touches a device."""
import ctypes as C

import numpy as np

import sr_livo_amd as srl
from sr_livo_amd import capi

SRL_ERR_BAD_ARG = -3          # include/srlivo_hip.h: srl_status


def test_prune_entry_points_are_declared_and_exported():
    lib = srl.load_library()
    for name in ("srl_map_remove_far", "srl_lio_remove_points_far_from_location"):
        assert name in srl.declared_symbols()
        assert hasattr(lib, name)


def test_null_arguments_are_refused_without_a_device():
    lib = srl.load_library()
    loc = np.zeros(3)
    dloc = loc.ctypes.data_as(C.POINTER(C.c_double))
    nv, npnt = C.c_int32(7), C.c_int64(7)
    assert lib.srl_map_remove_far(None, dloc, 1.0, C.byref(nv), C.byref(npnt)) == SRL_ERR_BAD_ARG
    assert (nv.value, npnt.value) == (0, 0)                     # the counts are written before the check
    assert lib.srl_map_remove_far(None, None, 1.0, None, None) == SRL_ERR_BAD_ARG
    # a non-NULL context with a NULL location: refused before the context is looked at (any non-NULL pointer will do here)
    dummy = (C.c_char * 64)()
    assert lib.srl_map_remove_far(C.cast(dummy, C.c_void_p), None, 1.0, None, None) == SRL_ERR_BAD_ARG
    assert lib.srl_lio_remove_points_far_from_location(None, dloc, 1.0) == SRL_ERR_BAD_ARG
    assert lib.srl_lio_remove_points_far_from_location(None, None, 1.0) == SRL_ERR_BAD_ARG


def test_host_only_handle_refuses_null_location_and_has_no_fallback():
    lib = srl.load_library()
    h = C.c_void_p()
    assert lib.srl_lio_create(-1, C.byref(h)) == capi.SRL_OK        # host-only object: no device map behind it
    try:
        assert lib.srl_lio_remove_points_far_from_location(h, None, 1.0) == SRL_ERR_BAD_ARG
        loc = np.zeros(3)
        rc = lib.srl_lio_remove_points_far_from_location(h, loc.ctypes.data_as(C.POINTER(C.c_double)), 1.0)
        assert rc != capi.SRL_OK                                   # no device map: an error, never a host-side prune
    finally:
        lib.srl_lio_destroy(h)
