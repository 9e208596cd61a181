"""The ABI of the PointCloud2 decode (srl_pc2_decode, srl_pc2_yaw_angles and the mirror's two entry points): struct sizes and offsets
against ctypes and the header's text, the exported symbols, the refusals that need no device, and the pure host helper against
math.atan2 bit for bit on a layout where nothing is aligned."""
import ctypes as C
import math
import os
import re

import numpy as np

import pc2_cases as pc
import pc2_checker as pk
import sr_livo_amd as srl
from sr_livo_amd import capi

NEW_SYMBOLS = ("srl_pc2_decode", "srl_pc2_yaw_angles", "srl_lio_set_pc2_options", "srl_lio_feed_pointcloud2")


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(capi.INCLUDE_DIR, name)).read(), flags=re.S)


def test_struct_sizes_and_offsets():
    assert C.sizeof(capi.Pc2Layout) == 40 and C.sizeof(capi.Pc2Opts) == 32 and C.sizeof(capi.Pc2Report) == 40
    assert [getattr(capi.Pc2Layout, f).offset for f in ("width", "height", "point_step", "row_step", "off_x", "off_y", "off_z", "off_time", "off_ring",
                                                        "is_bigendian")] == list(range(0, 40, 4))
    assert [getattr(capi.Pc2Opts, f).offset for f in ("lidar_type", "n_scans", "scan_rate", "point_filter_num", "time_unit_scale", "blind")] == [0, 4, 8, 12, 16, 24]
    assert [getattr(capi.Pc2Report, f).offset for f in ("points", "given_offset_time", "picked", "appended", "last_end_time", "first_timestamp",
                                                        "last_timestamp")] == [0, 4, 8, 12, 16, 24, 32]
    # the header says the same, member by member and in this order (the library's own static_asserts hold the sizes at build time)
    text = _header("srlivo_hip.h")
    for struct, cls in (("srl_pc2_layout", capi.Pc2Layout), ("srl_pc2_opts", capi.Pc2Opts), ("srl_pc2_report", capi.Pc2Report)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
        members = [m for decl in body.split(";") for m in re.sub(r"^\s*(uint32_t|int32_t|double)\s+", "", decl.strip()).replace(" ", "").split(",") if m]
        assert members == [f[0] for f in cls._fields_], struct
    assert (capi.LIDAR_LIVOX, capi.LIDAR_VELO, capi.LIDAR_OUST, capi.LIDAR_ROBO) == (pk.LIVOX, pk.VELO, pk.OUST, pk.ROBO) == (1, 2, 3, 4)
    for lt in (pk.VELO, pk.OUST, pk.ROBO):
        assert capi.PC2_POINT_DTYPES[lt]["time"] == np.dtype(pk.TIME_DTYPE[lt]) and capi.PC2_POINT_DTYPES[lt]["ring"] == np.dtype(pk.RING_DTYPE[lt])


def test_every_new_symbol_is_declared_and_exported():
    declared = srl.declared_symbols()
    lib = srl.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name), name
    assert "srl_pc2_decode" in _header("srlivo_hip.h") and "srl_lio_feed_pointcloud2" in _header("srlivo_host.h")


def test_refusals_that_need_no_device():
    lib = srl.load_library()
    p = pc.make_points(pc.VELO, 8, 1)
    data, lay = srl.pc2_message(p, pc.VELO)
    ptr = data.ctypes.data_as(C.c_void_p)
    r = capi.Pc2Report()
    o = srl.pc2_opts(pc.VELO)

    def rc(ctx=None, ptr=ptr, nbytes=data.nbytes, lay=lay, stamp=1.0, last_end=-1.0, o=o):
        r.points = r.appended = 7
        r.last_end_time = 1.0
        code = lib.srl_pc2_decode(ctx, ptr, nbytes, C.byref(lay) if lay is not None else None, stamp, last_end, C.byref(o) if o is not None else None, C.byref(r))
        assert (r.points, r.given_offset_time, r.picked, r.appended) == (0, 0, 0, 0) and np.isnan(r.last_end_time) and np.isnan(r.first_timestamp)
        return code

    assert rc() == capi.SRL_ERR_BAD_ARG                                              # a null context
    # everything below is refused before the context is looked at; a context that is no context makes sure of it
    fake = C.c_void_p(1)
    assert rc(ctx=fake, ptr=None) == rc(ctx=fake, lay=None) == rc(ctx=fake, o=None) == capi.SRL_ERR_BAD_ARG
    bad = capi.Pc2Layout.from_buffer_copy(lay); bad.is_bigendian = 1
    assert rc(ctx=fake, lay=bad) == capi.SRL_ERR_BAD_ARG
    for name, size in (("off_x", 4), ("off_y", 4), ("off_z", 4), ("off_time", 4), ("off_ring", 2)):
        bad = capi.Pc2Layout.from_buffer_copy(lay); setattr(bad, name, lay.point_step - size + 1)
        assert rc(ctx=fake, lay=bad) == capi.SRL_ERR_BAD_ARG, name                   # a field past point_step
        bad = capi.Pc2Layout.from_buffer_copy(lay); setattr(bad, name, -1)
        assert rc(ctx=fake, lay=bad) == capi.SRL_ERR_BAD_ARG, name
    bad = capi.Pc2Layout.from_buffer_copy(lay); bad.point_step = 0
    assert rc(ctx=fake, lay=bad) == capi.SRL_ERR_BAD_ARG
    assert rc(ctx=fake, nbytes=data.nbytes - 1) == rc(ctx=fake, nbytes=0) == capi.SRL_ERR_BAD_ARG          # short of the last point
    robo = srl.pc2_opts(pc.ROBO)
    assert rc(ctx=fake, o=robo) == capi.SRL_ERR_BAD_ARG                              # the double at 18 does not fit into a 22-byte point
    for lt in (capi.LIDAR_LIVOX, 0, 5, -2):
        assert rc(ctx=fake, o=srl.pc2_opts(lt)) == capi.SRL_ERR_BAD_ARG, lt
    assert rc(ctx=fake, o=srl.pc2_opts(pc.VELO, point_filter_num=0)) == rc(ctx=fake, o=srl.pc2_opts(pc.VELO, point_filter_num=-1)) == capi.SRL_ERR_BAD_ARG
    for v in (0.0, -1.0, float("inf"), float("nan")):
        assert rc(ctx=fake, o=srl.pc2_opts(pc.VELO, time_unit_scale_value=v)) == capi.SRL_ERR_BAD_ARG, v
    assert rc(ctx=fake, o=srl.pc2_opts(pc.VELO, blind=float("nan"))) == rc(ctx=fake, stamp=float("nan")) == rc(ctx=fake, last_end=float("nan")) == capi.SRL_ERR_BAD_ARG
    # the mirror
    assert lib.srl_lio_set_pc2_options(None, C.byref(o)) == capi.SRL_ERR_BAD_ARG
    assert lib.srl_lio_feed_pointcloud2(None, ptr, data.nbytes, C.byref(lay), 1.0, C.byref(r)) == capi.SRL_ERR_BAD_ARG
    assert r.points == 0 and np.isnan(r.last_end_time)


def test_the_yaw_helper_equals_libm_bitwise_on_an_unaligned_layout():
    rng = np.random.default_rng(3)
    n = 3 * 41
    p = np.zeros(n, dtype=capi.PC2_POINT_DTYPES[pc.ROBO])
    p["x"], p["y"] = rng.normal(0, 20, n).astype(np.float32), rng.normal(0, 20, n).astype(np.float32)
    p["x"][:8] = [0.0, -0.0, 0.0, -0.0, 1.0, -1.0, np.inf, np.nan]
    p["y"][:8] = [0.0, 0.0, -0.0, -0.0, 0.0, -0.0, -np.inf, 1.0]
    data, lay = srl.pc2_message(p, pc.ROBO, point_step=27, offsets=dict(x=1, y=6, z=11, ring=15, time=19), height=3, row_pad=3)
    block = np.empty(data.nbytes + 1, dtype=np.uint8)
    block[1:] = data                                                                 # the buffer itself starts at an odd address
    yaw = srl.pc2_yaw_angles(block[1:], lay)
    want = np.array([math.atan2(float(b), float(a)) * 57.2957 for a, b in zip(p["x"], p["y"])])
    # (index 7 has a NaN coordinate: NaN from both, but math.atan2 answers a NaN argument itself, with a NaN of its own making)
    assert np.isnan(yaw[7]) and np.isnan(want[7])
    yaw[7] = want[7] = 0.0
    assert yaw.tobytes() == want.tobytes()
    assert np.delete(yaw, 7).tobytes() == np.delete(np.array(pk.yaw_angles(p["x"], p["y"])), 7).tobytes()
    lib = srl.load_library()
    out = np.zeros(n)
    # (the last row's padding is not needed: the last point's end is what counts)
    assert lib.srl_pc2_yaw_angles(data.ctypes.data_as(C.c_void_p), data.nbytes - 3, C.byref(lay), capi._dptr(out)) == capi.SRL_OK
    out[:] = 0.0
    assert lib.srl_pc2_yaw_angles(data.ctypes.data_as(C.c_void_p), data.nbytes - 4, C.byref(lay), capi._dptr(out)) == capi.SRL_ERR_BAD_ARG
    assert lib.srl_pc2_yaw_angles(None, data.nbytes, C.byref(lay), capi._dptr(out)) == capi.SRL_ERR_BAD_ARG and not out.any()
    assert lib.srl_pc2_yaw_angles(data.ctypes.data_as(C.c_void_p), data.nbytes, None, capi._dptr(out)) == capi.SRL_ERR_BAD_ARG
