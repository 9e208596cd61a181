"""srl_frame_subsample / srl_frame_take_subsampled / srl_lio_set_device_subsample (buildFrame's subSampleFrame on the device) on a box
without a GPU: the entry points are exported and declared, and bad arguments are refused before anything touches a device."""
import ctypes as C

import numpy as np

import sr_livo_amd as srl
from sr_livo_amd import capi

SRL_ERR_BAD_ARG = -3          # include/srlivo_hip.h: srl_status


def test_subsample_entry_points_are_declared_and_exported():
    lib = srl.load_library()
    for name in ("srl_frame_subsample", "srl_frame_take_subsampled", "srl_lio_set_device_subsample"):
        assert name in srl.declared_symbols()
        assert hasattr(lib, name)


def test_bad_arguments_are_refused_without_a_device():
    lib = srl.load_library()
    order = np.arange(4, dtype=np.int32)
    optr = order.ctypes.data_as(C.c_void_p)
    kept = C.c_int(7)
    # a NULL context
    assert lib.srl_frame_subsample(None, optr, 4, 0.1, C.byref(kept)) == SRL_ERR_BAD_ARG
    assert kept.value == 0                                       # the count is written before the check
    assert lib.srl_frame_take_subsampled(None, None, 0, None, None, None) == SRL_ERR_BAD_ARG
    # the rest with a non-NULL context: refused before the context is looked at (any non-NULL pointer will do here)
    dummy = C.cast((C.c_char * 4096)(), C.c_void_p)
    assert lib.srl_frame_subsample(dummy, None, 4, 0.1, C.byref(kept)) == SRL_ERR_BAD_ARG          # NULL visit order, n > 0
    assert lib.srl_frame_subsample(dummy, optr, -1, 0.1, C.byref(kept)) == SRL_ERR_BAD_ARG         # n < 0
    for size in (0.0, -0.1, float("nan")):                                                          # !(sample_size > 0)
        assert lib.srl_frame_subsample(dummy, optr, 4, size, C.byref(kept)) == SRL_ERR_BAD_ARG
    assert lib.srl_frame_subsample(dummy, optr, 4, 0.1, None) == SRL_ERR_BAD_ARG                   # NULL num_kept
    assert lib.srl_frame_take_subsampled(dummy, None, -1, None, None, None) == SRL_ERR_BAD_ARG      # m < 0
    assert lib.srl_lio_set_device_subsample(None, 1) == SRL_ERR_BAD_ARG


def test_host_only_handle_takes_the_switch():
    lib = srl.load_library()
    h = C.c_void_p()
    assert lib.srl_lio_create(-1, C.byref(h)) == capi.SRL_OK        # host-only object: no device behind it
    try:
        assert lib.srl_lio_set_device_subsample(h, 0) == capi.SRL_OK
        assert lib.srl_lio_set_device_subsample(h, 1) == capi.SRL_OK
    finally:
        lib.srl_lio_destroy(h)
