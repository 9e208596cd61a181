"""The C-ABI of the image preparation without a device (CPU), in the manner of tests/test_color_track_abi.py: the symbols are declared
and exported, the two structures agree between include/srlivo_hip.h and the ctypes layer, the defaults are the reference's, every refusal
that is made before a device is touched is made (the rules on the options through srl_image_prep_build_map, which shares them with
srl_image_prep_create; the rest on a NULL context), and srl_image_prep_build_map equals the checker's map bytewise."""
import ctypes as C
import os
import re

import numpy as np

import imgprep_checker as ck
import sr_livo_amd as srl
from sr_livo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRL_OK, SRL_ERR_NO_DEVICE, SRL_ERR_BAD_ARG = 0, -1, -3
SIZES = {"double": 8, "int32_t": 4}
NEW = ("srl_image_prep_opts_default", "srl_image_prep_build_map", "srl_image_prep_create", "srl_image_prep_destroy", "srl_image_prepare",
       "srl_image_prep_download", "srl_flow_track_prepared", "srl_image_prep_download_stage", "srl_oft_use_prepared_image")


def _header_fields(name):
    text = open(os.path.join(ROOT, "include", "srlivo_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
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
    for name, cls, size in (("srl_image_prep_opts", capi.ImagePrepOpts, 104), ("srl_image_prep_info", capi.ImagePrepInfo, 32)):
        fields = _header_fields(name)
        assert [f for f, _ in fields] == [f for f, _ in cls._fields_], name
        assert [s for _, s in fields] == [C.sizeof(t) for _, t in cls._fields_], name
        assert sum(s for _, s in fields) == C.sizeof(cls) == size, name
    text = open(os.path.join(ROOT, "include", "srlivo_hip_debug.h")).read()
    stages = re.search(r"enum \{ SRL_PREP_STAGE_UNDIST = 0, SRL_PREP_STAGE_GRAY = 1, SRL_PREP_STAGE_YCRCB = 2, SRL_PREP_STAGE_LUT_GRAY = 3, SRL_PREP_STAGE_LUT_Y = 4 \}", text)
    assert stages and (capi.SRL_PREP_STAGE_UNDIST, capi.SRL_PREP_STAGE_GRAY, capi.SRL_PREP_STAGE_YCRCB, capi.SRL_PREP_STAGE_LUT_GRAY,
                       capi.SRL_PREP_STAGE_LUT_Y) == (0, 1, 2, 3, 4)


def test_defaults():
    o = capi.ImagePrepOpts()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    srl.load_library().srl_image_prep_opts_default(C.byref(o))
    assert (o.clip_gray, o.clip_color, o.tiles, o.reserved, o.rows, o.cols) == (3.0, 1.0, 0, 0, 0, 0)
    assert (o.fx, o.fy, o.cx, o.cy) == (0.0, 0.0, 0.0, 0.0) and list(o.dist) == [0.0] * 5
    srl.load_library().srl_image_prep_opts_default(None)           # tolerated
    o = capi.default_image_prep_opts(rows=20, cols=30, dist=[1, 2, 3, 4, 5])
    assert (o.rows, o.cols, list(o.dist), o.clip_gray) == (20, 30, [1.0, 2.0, 3.0, 4.0, 5.0], 3.0)


def _opts(**kw):
    base = dict(rows=48, cols=64, fx=60.0, fy=61.0, cx=31.5, cy=23.5)
    base.update(kw)
    return capi.default_image_prep_opts(**base)


def _build_rc(o, map1=True, map2=True):
    n = max(o.rows, 1) * max(o.cols, 1) if 0 < o.rows <= 16384 and 0 < o.cols <= 16384 else 1
    m1 = np.full((n, 2), 7, np.int16)
    m2 = np.full(n, 7, np.uint16)
    rc = srl.load_library().srl_image_prep_build_map(C.byref(o), capi._ptr(m1) if map1 else None, capi._ptr(m2) if map2 else None)
    return rc, m1, m2


def test_every_refusal_on_the_options_leaves_the_maps_alone():
    nan, inf = float("nan"), float("inf")
    bad = [dict(rows=15), dict(cols=15), dict(rows=0), dict(cols=-4), dict(rows=16385, cols=64), dict(rows=64, cols=16385),
           dict(rows=8193, cols=8193),                             # rows * cols > SRL_COLOR_IMAGE_MAX_PIXELS
           dict(rows=16, cols=400),                                # T = 20 >= rows: the reflection would leave the image
           dict(rows=20, cols=400),                                # rows == T
           dict(tiles=-1), dict(tiles=1), dict(tiles=25),          # above min(rows, cols) / 2 = 24
           dict(fx=0.0), dict(fy=0.0), dict(fx=nan), dict(fy=inf), dict(cx=nan), dict(cy=-inf),
           dict(clip_gray=0.0), dict(clip_gray=-1.0), dict(clip_gray=nan), dict(clip_gray=inf),
           dict(clip_color=0.0), dict(clip_color=-3.0), dict(clip_color=nan), dict(clip_color=inf)]
    bad += [dict(dist=[0.0] * k + [v] + [0.0] * (4 - k)) for k in range(5) for v in (nan, inf)]
    for kw in bad:
        rc, m1, m2 = _build_rc(_opts(**kw))
        assert rc == SRL_ERR_BAD_ARG and (m1 == 7).all() and (m2 == 7).all(), kw
    o = _opts()
    assert _build_rc(o, map1=False)[0] == SRL_ERR_BAD_ARG and _build_rc(o, map2=False)[0] == SRL_ERR_BAD_ARG
    assert srl.load_library().srl_image_prep_build_map(None, None, None) == SRL_ERR_BAD_ARG
    # the edges that are allowed
    for kw in (dict(rows=16, cols=16), dict(tiles=2), dict(tiles=24), dict(rows=21, cols=400), dict(rows=17, cols=16384, tiles=2)):
        assert _build_rc(_opts(**kw))[0] == SRL_OK, kw


def test_every_entry_refuses_a_null_context_or_argument_and_zeroes_the_info():
    lib = srl.load_library()
    o = _opts()
    img = np.zeros((48, 64, 3), np.uint8)
    out = np.full((48, 64, 3), 7, np.uint8)
    info = capi.ImagePrepInfo()
    C.memset(C.byref(info), 0xFF, C.sizeof(info))
    assert lib.srl_image_prep_create(None, C.byref(o)) == SRL_ERR_BAD_ARG
    assert lib.srl_image_prep_create(None, None) == SRL_ERR_BAD_ARG
    assert lib.srl_image_prep_destroy(None) == SRL_ERR_BAD_ARG
    assert lib.srl_image_prepare(None, capi._ptr(img), 48, 64, 192, C.byref(info)) == SRL_ERR_BAD_ARG
    assert bytes(info) == bytes(C.sizeof(info))
    assert lib.srl_image_prepare(None, None, 48, 64, 192, None) == SRL_ERR_BAD_ARG
    for which in (0, 1, 2, -1):
        assert lib.srl_image_prep_download(None, which, capi._ptr(out), 192) == SRL_ERR_BAD_ARG
    for stage in (0, 4, 5, -1):
        assert lib.srl_image_prep_download_stage(None, stage, capi._ptr(out), out.size) == SRL_ERR_BAD_ARG
    assert (out == 7).all()
    prev = np.ones((4, 2), np.float32)
    nxt = np.full((4, 2), 7, np.float32)
    st = np.full(4, 7, np.uint8)
    nt = C.c_int(-5)
    assert lib.srl_flow_track_prepared(None, capi._ptr(prev), 4, capi._ptr(nxt), capi._ptr(st), C.byref(nt)) == SRL_ERR_BAD_ARG
    assert nt.value == 0 and (nxt == 7).all() and (st == 7).all()


def test_the_mirror_refuses_the_prepared_image_without_a_context_and_then_behaves_as_before():
    lib = srl.load_library()
    assert lib.srl_oft_use_prepared_image(None, 1) == SRL_ERR_BAD_ARG
    oft = srl.Oft(None)
    try:
        try:
            oft.use_prepared_image(True)
            raise AssertionError("opted in on a handle without a context")
        except srl.SrlError as e:
            assert e.status == SRL_ERR_NO_DEVICE
        # ... and a NULL gray is still the reference's empty image: only the time moves
        assert oft.track_image(None, 1.5, 48, 64) == 0 and oft.times()[1] == 1.5
    finally:
        oft.close()


CASES = {
    "zero distortion": dict(dist=[0, 0, 0, 0, 0]),
    "barrel": dict(dist=[-0.3, 0, 0, 0, 0]),
    "pincushion, border pixels map outside": dict(dist=[0.3, 0.1, 0, 0, 0]),
    "tangential with k3": dict(dist=[-0.12, 0.05, 0.01, -0.01, 0.02]),
    "tangential with k3, signs swapped": dict(dist=[0.08, -0.03, -0.01, 0.01, -0.015]),
    "non-finite at the corners": dict(fx=1e-150, fy=1e-150, cx=48.0, cy=32.0, dist=[1e300, 0, 0, 0, 0]),
    "beyond int32 and beyond int16": dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0, dist=[1e4, 0, 0, 0, 0]),
}


def test_build_map_equals_the_checker_bytewise():
    for name, kw in CASES.items():
        for rows, cols in ((64, 96), (37, 53)):
            base = dict(rows=rows, cols=cols, fx=0.9 * cols, fy=0.92 * cols, cx=cols / 2 - 0.37, cy=rows / 2 + 0.21)
            base.update(kw)
            o = capi.default_image_prep_opts(**base)
            map1, map2 = capi.image_prep_build_map(o)
            c1, c2 = ck.build_map(rows, cols, o.fx, o.fy, o.cx, o.cy, list(o.dist))
            assert map1.dtype == c1.dtype and map2.dtype == c2.dtype
            assert map1.tobytes() == c1.tobytes() and map2.tobytes() == c2.tobytes(), (name, rows, cols)
    # what the cases are there for
    o = capi.default_image_prep_opts(rows=64, cols=96, fx=86.4, fy=88.32, cx=47.63, cy=32.21, dist=[0.3, 0.1, 0, 0, 0])
    map1, _ = capi.image_prep_build_map(o)
    assert map1[0, 0, 0] < 0 and map1[0, 0, 1] < 0 and map1[63, 95, 0] > 95 and map1[63, 95, 1] > 63
    o = capi.default_image_prep_opts(rows=64, cols=96, **{k: v for k, v in CASES["non-finite at the corners"].items()})
    map1, map2 = capi.image_prep_build_map(o)
    assert (map1[0, 0] == -32768).all() and map2[0, 0] == 0 and tuple(map1[32, 48]) == (48, 32)
    o = capi.default_image_prep_opts(rows=64, cols=96, **{k: v for k, v in CASES["beyond int32 and beyond int16"].items()})
    map1, _ = capi.image_prep_build_map(o)
    assert (map1[63, 95] == -32768).all() and tuple(map1[2, 1]) == (32767, 32767) and tuple(map1[0, 1]) == (10001, 0)
