"""The C-ABI of the one-call camera frame (srl_lio_image_*, include/srlivo_host.h) without a device, in the manner of
tests/test_image_prep_abi.py: the symbols are declared and exported, the three structures agree between the header and the ctypes
layer, the defaults are the reference's constructor values (imageProcessing.cpp:11-18), and every refusal that is made before a step
runs is made."""
import ctypes as C
import os
import re

import numpy as np

import sr_livo_amd as srl
from sr_livo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRL_OK, SRL_ERR_NO_DEVICE, SRL_ERR_BAD_ARG = 0, -1, -3
POINTER = C.sizeof(C.c_void_p)
SIZES = {"double": 8, "int32_t": 4, "srl_color_render_totals": C.sizeof(capi.ColorRenderTotals), "srl_color_track_totals": C.sizeof(capi.ColorTrackTotals)}
NEW = ("srl_image_process_opts_default", "srl_lio_image_set_options", "srl_lio_image_set_steps", "srl_lio_image_process", "srl_lio_image_oft",
       "srl_lio_image_candidates", "srl_lio_image_time_last_process", "srl_lio_run_measurement_image", "srl_lio_set_g_norm")


def _body(name):
    text = open(os.path.join(ROOT, "include", "srlivo_host.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    return re.sub(r"/\*.*?\*/", "", body, flags=re.S)


def _plain_fields(name):
    fields = []
    for decl in _body(name).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for nm in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", nm)
            fields.append((m.group(1), SIZES[ctype] * int(m.group(2) or 1)))
    return fields


def test_symbols_are_declared_and_exported():
    declared, exported = srl.declared_symbols(), srl.library_symbols()
    for s in NEW:
        assert s in declared and s in exported, s


def test_structs_agree_with_the_header():
    for name, cls, size in (("srl_image_process_opts", capi.ImageProcessOpts, 88), ("srl_image_process_result", capi.ImageProcessResult, 232)):
        fields = _plain_fields(name)
        assert [f for f, _ in fields] == [f for f, _ in cls._fields_], name
        assert [s for _, s in fields] == [C.sizeof(t) for _, t in cls._fields_], name
        assert sum(s for _, s in fields) == C.sizeof(cls) == size, name
    # the step table: a user pointer and ten function pointers, in the header's order
    members = re.findall(r"\(\*(\w+)\)\s*\(|\b(?:void \*|srl_\w+_provider )(\w+);", _body("srl_image_process_steps"))
    names = [a or b for a, b in members]
    assert names == [f for f, _ in capi.ImageProcessSteps._fields_], names
    assert C.sizeof(capi.ImageProcessSteps) == 11 * POINTER
    assert capi.ImageProcessResult.render.offset == 64 and capi.ImageProcessResult.track.offset == 120 and capi.ImageProcessResult.image_scale_factor.offset == 56


def test_defaults_are_the_references_constructor_values():
    o = capi.ImageProcessOpts()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    lib = srl.load_library()
    lib.srl_image_process_opts_default(C.byref(o))
    assert (o.image_width, o.image_height, o.image_resize_ratio, list(o.dist)) == (0, 0, 1.0, [0.0] * 5)
    assert (o.track_windows_size, o.maximum_tracked_points, o.reserved, o.tracker_minimum_depth, o.tracker_maximum_depth) == (40.0, 300, 0, 0.1, 200.0)
    lib.srl_image_process_opts_default(None)             # tolerated


def test_refusals_that_need_no_device():
    lib = srl.load_library()
    img = np.zeros((48, 64, 3), np.uint8)
    res = capi.ImageProcessResult()
    o = capi.ImageProcessOpts()
    lib.srl_image_process_opts_default(C.byref(o))
    n = C.c_int(7)
    t = C.c_double(7.0)
    # a NULL handle
    assert lib.srl_lio_image_set_options(None, C.byref(o)) == SRL_ERR_BAD_ARG and lib.srl_lio_image_set_steps(None, None) == SRL_ERR_BAD_ARG
    C.memset(C.byref(res), 0xFF, C.sizeof(res))
    assert lib.srl_lio_image_process(None, capi._ptr(img), 48, 64, 192, 1.0, 1, C.byref(res)) == SRL_ERR_BAD_ARG and bytes(res) == bytes(C.sizeof(res))
    assert lib.srl_lio_image_oft(None) is None
    assert lib.srl_lio_image_candidates(None, None, 0, C.byref(n)) == SRL_ERR_BAD_ARG and n.value == 0
    assert lib.srl_lio_image_time_last_process(None, C.byref(t)) == SRL_ERR_BAD_ARG
    lio = srl.Lio(-1)
    try:
        h = lio.h
        # options: a size, a positive ratio and a positive window are needed (the defaults carry no size)
        assert lib.srl_lio_image_set_options(h, None) == SRL_ERR_BAD_ARG and lib.srl_lio_image_set_options(h, C.byref(o)) == SRL_ERR_BAD_ARG
        call = lambda: lib.srl_lio_image_process(h, capi._ptr(img), 48, 64, 192, 1.0, 1, C.byref(res))      # noqa: E731
        assert call() == SRL_ERR_BAD_ARG                 # no options yet
        for kw in (dict(image_width=0), dict(image_height=-1), dict(image_resize_ratio=0.0), dict(image_resize_ratio=float("nan")),
                   dict(track_windows_size=0.0), dict(track_windows_size=float("nan"))):
            bad = capi.ImageProcessOpts.from_buffer_copy(o)
            bad.image_width, bad.image_height = 64, 48
            for k, v in kw.items():
                setattr(bad, k, v)
            assert lib.srl_lio_image_set_options(h, C.byref(bad)) == SRL_ERR_BAD_ARG, kw
        assert call() == SRL_ERR_BAD_ARG                 # a refused set leaves none
        o.image_width, o.image_height = 64, 48
        assert lib.srl_lio_image_set_options(h, C.byref(o)) == SRL_OK
        # the frame
        for args in ((None, 48, 64, 192), (capi._ptr(img), 0, 64, 192), (capi._ptr(img), 48, 0, 192), (capi._ptr(img), 48, 64, 191)):
            C.memset(C.byref(res), 0xFF, C.sizeof(res))
            assert lib.srl_lio_image_process(h, *args, 1.0, 1, C.byref(res)) == SRL_ERR_BAD_ARG and bytes(res) == bytes(C.sizeof(res)), args[1:]
        # a host-only handle with its steps at their defaults: no device, never a host loop
        assert call() == SRL_ERR_NO_DEVICE and lib.srl_lio_image_process(h, capi._ptr(img), 48, 64, 192, 1.0, 1, None) == SRL_ERR_NO_DEVICE
        assert b"host-only" in lib.srl_lio_last_error(h)
        # the read-backs before any frame
        assert lib.srl_lio_image_candidates(h, None, 0, C.byref(n)) == SRL_OK and n.value == 0
        assert lib.srl_lio_image_candidates(h, None, 0, None) == SRL_ERR_BAD_ARG and lib.srl_lio_image_candidates(h, None, 4, C.byref(n)) == SRL_ERR_BAD_ARG
        assert lib.srl_lio_image_time_last_process(h, C.byref(t)) == SRL_OK and t.value == -1e5
        assert lib.srl_lio_image_time_last_process(h, None) == SRL_ERR_BAD_ARG
        oft = lio.image_oft()
        assert oft.h.value and oft.sizes() == (0, 0, 0, 0) and lib.srl_lio_image_oft(h) == oft.h.value      # one tracker, the handle's
        # a measurement with an image: the image's arguments are checked before the sweep is touched; a host-only handle has no device
        rmi = lambda image, r, c, stride: lib.srl_lio_run_measurement_image(h, 0.0, None, None, None, 0, None, None, 0, 0.0, 0.1, image, r, c, stride, None, None)      # noqa: E731
        assert rmi(capi._ptr(img), 0, 64, 192) == SRL_ERR_BAD_ARG and rmi(capi._ptr(img), 48, 64, 191) == SRL_ERR_BAD_ARG
        assert rmi(capi._ptr(img), 48, 64, 192) == SRL_ERR_NO_DEVICE
        assert lib.srl_lio_run_measurement_image(None, 0.0, None, None, None, 0, None, None, 0, 0.0, 0.1, capi._ptr(img), 48, 64, 192, None, None) == SRL_ERR_BAD_ARG
        # G_norm: finite and positive
        for bad in (0.0, -9.81, float("nan"), float("inf")):
            assert lib.srl_lio_set_g_norm(h, bad) == SRL_ERR_BAD_ARG, bad
        assert lib.srl_lio_set_g_norm(None, 9.81) == SRL_ERR_BAD_ARG and lib.srl_lio_set_g_norm(h, 9.81) == SRL_OK
    finally:
        lio.close()
