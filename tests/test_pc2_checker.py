"""The independent checker of the PointCloud2 decode (tests/pc2_checker.py) on cases small enough to work out by hand, and the message
builder (sr_livo_amd.capi.pc2_message) against the checker's own field reader.  No device, no library call except the pure host helper
behind the builder's layouts."""
import math

import numpy as np
import pytest

import pc2_cases as pc
import pc2_checker as pk
from sr_livo_amd import capi

F32 = np.float32


def _points(lidar_type, rows):
    """rows of (x, y, z, time, ring)"""
    p = np.zeros(len(rows), dtype=capi.PC2_POINT_DTYPES[lidar_type])
    for i, r in enumerate(rows):
        p[i] = tuple(r)
    return p


def _decode(lidar_type, p, stamp=100.0, last_end=-1.0, n_scans=4, scan_rate=10, scale=1.0, blind=0.5, pfn=1, **layout):
    data, lay = capi.pc2_message(p, lidar_type, **layout)
    return pk.decode(data, lay, lidar_type, stamp, last_end, n_scans, scan_rate, scale, blind, pfn)


def test_the_builder_and_the_field_reader_agree_on_every_layout():
    for lt in (pc.VELO, pc.OUST, pc.ROBO):
        p = pc.make_points(lt, 24, 5)
        step0, off0 = capi.PC2_DRIVER_LAYOUTS[lt]
        for kw in (dict(), dict(point_step=step0 + 9), dict(height=4, row_pad=3), dict(point_step=64, offsets=dict(x=33, y=1, z=7, time=50, ring=61), height=2, row_pad=1)):
            data, lay = capi.pc2_message(p, lt, **kw)
            L = pk.layout_dict(lay)
            assert L["row_step"] == L["width"] * L["point_step"] + kw.get("row_pad", 0) and L["width"] * L["height"] == 24
            assert data.nbytes == L["height"] * L["row_step"]
            assert pk.layout_ok(L, lt, data.nbytes) and not pk.layout_ok(L, lt, data.nbytes - kw.get("row_pad", 0) - 1)
            for name, key, dt in (("x", "off_x", "<f4"), ("y", "off_y", "<f4"), ("z", "off_z", "<f4"), ("time", "off_time", pk.TIME_DTYPE[lt]), ("ring", "off_ring", pk.RING_DTYPE[lt])):
                assert pk.field(data, L, L[key], dt).tobytes() == np.ascontiguousarray(p[name]).tobytes(), (lt, kw, name)
            # every byte that is no field is the fill
            covered = sum(np.dtype(d).itemsize for d in ("<f4", "<f4", "<f4", pk.TIME_DTYPE[lt], pk.RING_DTYPE[lt]))
            assert int(np.count_nonzero(data == 0xA5)) >= data.nbytes - 24 * covered
    with pytest.raises(ValueError):
        capi.pc2_message(pc.make_points(pc.ROBO, 4, 1), pc.ROBO, point_step=24)          # the double at 18 does not fit into 24 bytes


def test_velodyne_given_times_by_hand():
    # times in ms (scale 1): sorted order is index 2 (-2), 0 (1), 3 (3), 1 (4); the last message record is positive
    p = _points(pc.VELO, [(1, 0, 0, 1.0, 0), (2, 0, 0, 4.0, 1), (3, 0, 0, -2.0, 2), (0.25, 0, 0, 3.0, 3)])
    w = _decode(pc.VELO, p)
    assert (w["status"], w["given"], w["points"], w["picked"], w["appended"], w["has_ties"]) == ("ok", 1, 4, 4, 3, False)
    assert w["records"].tolist() == [[3.0, 0, 0, -2.0, 100.0 - 0.002], [1.0, 0, 0, 1.0, 100.001], [2.0, 0, 0, 4.0, 100.004]]      # x = 0.25 is inside blind
    assert w["last_end_time"] == 100.0 + 4.0 / 1000.0 and w["first_timestamp"] == 100.0 - 0.002 and w["last_timestamp"] == 100.004
    # the pick is on the sorted position, before the blind test: positions 0 and 2 -> message indices 2 and 3; 3 is blind
    w = _decode(pc.VELO, p, pfn=2)
    assert (w["picked"], w["appended"]) == (2, 1) and w["records"][0, 0] == 3.0
    # the last_end_time test is strict
    w = _decode(pc.VELO, p, last_end=100.001)
    assert w["records"][:, 0].tolist() == [2.0] and not w["all_pass"]
    # a point exactly at blind is dropped, the next float is kept
    q = _points(pc.VELO, [(1.5, 0, 0, 1.0, 0), (np.nextafter(F32(1.5), F32(2)), 0, 0, 2.0, 0)])
    assert _decode(pc.VELO, q, blind=1.5)["records"][:, 3].tolist() == [2.0]


def test_ties_keep_message_order_and_signed_zeros_tie():
    p = _points(pc.VELO, [(1, 0, 0, 0.0, 0), (2, 0, 0, -0.0, 0), (3, 0, 0, 0.0, 0), (4, 0, 0, -1.0, 0), (5, 0, 0, 7.0, 0)])
    w = _decode(pc.VELO, p)
    assert w["has_ties"] and w["records"][:, 0].tolist() == [4.0, 1.0, 2.0, 3.0, 5.0]
    assert [math.copysign(1.0, v) for v in w["records"][1:4, 3]] == [1.0, -1.0, 1.0]            # relative_time keeps the zero's own sign
    p = _points(pc.OUST, [(1, 0, 0, 50, 0), (2, 0, 0, 20, 1), (3, 0, 0, 50, 2), (4, 0, 0, 20, 3)])
    w = _decode(pc.OUST, p, scale=2.0)
    assert w["has_ties"] and w["records"][:, 0].tolist() == [2.0, 4.0, 1.0, 3.0] and w["records"][:, 3].tolist() == [40.0, 40.0, 100.0, 100.0]


def test_ouster_top_bit_and_the_branch_from_the_last_record():
    p = _points(pc.OUST, [(1, 0, 0, 0xFFFFFFFF, 0), (2, 0, 0, 0x80000000, 0), (3, 0, 0, 5, 0)])
    w = _decode(pc.OUST, p, scale=float(F32(1e-6)))
    assert w["given"] == 1 and w["records"][:, 0].tolist() == [3.0, 2.0, 1.0]
    assert w["records"][2, 3] == 4294967295.0 * float(F32(1e-6))
    p["time"][2] = 0                                           # the last record alone decides: the yaw branch, whatever the others hold
    assert _decode(pc.OUST, p)["given"] == 0


def test_robosense_relative_to_the_sorted_front_and_the_absolute_last():
    t0 = 1.7e9
    p = _points(pc.ROBO, [(1, 0, 0, t0 + 0.5, 0), (2, 0, 0, t0 + 0.25, 0), (3, 0, 0, t0 + 0.75, 0)])
    w = _decode(pc.ROBO, p, stamp=t0, scale=1000.0)
    assert w["records"][:, 0].tolist() == [2.0, 1.0, 3.0]
    assert w["records"][:, 3].tolist() == [0.0, ((t0 + 0.5) - (t0 + 0.25)) * 1000.0, ((t0 + 0.75) - (t0 + 0.25)) * 1000.0]
    assert w["last_end_time"] == t0 + ((t0 + 0.75) * 1000.0) / 1000.0                           # the reference's quirk: not the difference


def test_yaw_branch_by_hand():
    # one ring, scan_rate 10: omega = 3.61 degrees per ms.  The first point at 90 degrees; the others at 0, 180 (above the first: + 360) and 45
    p = _points(pc.VELO, [(0, 2, 0, 0, 0), (2, 0, 0, 0, 0), (-2, 0, 0, 0, 0), (2, 2, 0, 0, 0)])
    w = _decode(pc.VELO, p, blind=100.0)                       # no blind test in this branch
    omega = 0.361 * 10
    y = [math.atan2(a, b) * 57.2957 for a, b in ((2.0, 0.0), (0.0, 2.0), (0.0, -2.0), (2.0, 2.0))]
    want = [0.0, (y[0] - y[1]) / omega, (y[0] - y[2] + 360.0) / omega, (y[0] - y[3]) / omega]
    assert w["given"] == 0 and w["appended"] == 4 and not w["has_ties"]
    assert w["records"][:, 3].tolist() == sorted(want) and w["records"][:, 0].tolist() == [0.0, 2.0, 2.0, -2.0]
    assert w["records"][0, 4] == 0.0 and w["records"][1, 4] == want[3] / 1000.0 + 100.0          # the ring's first point: timestamp 0.0
    assert w["last_end_time"] == 100.0 + max(want) / 1000.0
    # ... which passes only while last_end_time is negative
    w = _decode(pc.VELO, p, last_end=0.0)
    assert w["appended"] == 3 and w["records"][:, 0].tolist() == [2.0, 2.0, -2.0] and not w["all_pass"]
    # two rings: both first points tie at 0 and keep message order; a duplicate of a first point ties with it at +0.0
    p = _points(pc.VELO, [(0, 2, 0, 0, 1), (2, 0, 0, 0, 0), (0, 2, 0, 0, 1), (2, 2, 0, 0, 0)])
    w = _decode(pc.VELO, p)
    assert w["has_ties"] and w["records"][:, 3].tolist()[:3] == [0.0, 0.0, 0.0] and w["records"][:, 4].tolist()[:3] == [0.0, 0.0, 100.0]
    assert w["records"][:, 0].tolist() == [0.0, 2.0, 0.0, 2.0]


def test_what_is_refused():
    p = pc.make_points(pc.VELO, 8, 3)
    ok = _decode(pc.VELO, p)
    assert ok["status"] == "ok"
    assert _decode(pc.VELO, p, pfn=0)["status"] == _decode(pc.VELO, p, scale=0.0)["status"] == _decode(pc.VELO, p, scale=float("inf"))["status"] == "refused"
    assert _decode(pc.VELO, p, blind=float("nan"))["status"] == _decode(pc.VELO, p, stamp=float("nan"))["status"] == "refused"
    assert _decode(pc.VELO, p, last_end=float("nan"))["status"] == "refused"
    data, lay = capi.pc2_message(p, pc.VELO)
    assert pk.decode(data, lay, 1, 100.0, -1.0, 4, 10, 1.0, 0.5, 1)["status"] == "refused"        # LIVOX is not a PointCloud2 LiDAR
    assert pk.decode(data[:-1], lay, pc.VELO, 100.0, -1.0, 4, 10, 1.0, 0.5, 1)["status"] == "refused"
    lay.is_bigendian = 1
    assert pk.decode(data, lay, pc.VELO, 100.0, -1.0, 4, 10, 1.0, 0.5, 1)["status"] == "refused"
    q = p.copy(); q["time"][2] = np.nan
    assert _decode(pc.VELO, q)["status"] == "refused"
    q = p.copy(); q["time"][-1] = np.nan                       # the yaw branch: a NaN time is not looked at there
    assert _decode(pc.VELO, q, n_scans=16)["status"] == "ok" and _decode(pc.VELO, q, n_scans=16)["given"] == 0
    q["time"] = 0
    assert _decode(pc.VELO, q, n_scans=16)["status"] == "ok"
    assert _decode(pc.VELO, q, n_scans=int(q["ring"].max()))["status"] == "refused"               # a ring == n_scans
    assert _decode(pc.VELO, q, n_scans=16, scan_rate=0)["status"] == _decode(pc.VELO, q, n_scans=0)["status"] == "refused"
    q["ring"] = [0, 0, 0, 0, 0, 0, 0, 3]
    q["y"][7] = np.nan                                         # the only point of its ring: relative_time 0.0, whatever its yaw -- accepted, as upstream
    assert _decode(pc.VELO, q, n_scans=16)["status"] == "ok"
    q["y"][5] = np.nan
    assert _decode(pc.VELO, q, n_scans=16)["status"] == "refused"                                 # a NaN relative_time
    for c in pc.refused_cases():
        assert [w["status"] for w in pk.decode_case(c)] == ["refused"], c["name"]


def test_an_empty_message_and_the_carried_time():
    w = _decode(pc.OUST, pc.make_points(pc.OUST, 0, 1))
    assert w["status"] == "ok" and w["points"] == 0 and w["appended"] == 0 and math.isnan(w["last_end_time"])
    c = pc.case_by_name("velo_overlap")
    ws = pk.decode_case(c)
    assert [w["points"] for w in ws] == [200, 200, 0, 200]
    assert 0 < ws[1]["appended"] < ws[0]["appended"] and not ws[1]["all_pass"]                    # the overlap drops a prefix
    assert ws[1]["records"][0, 4] > ws[0]["last_end_time"]
    assert ws[3]["appended"] > 0 and ws[3]["records"][0, 4] > ws[1]["last_end_time"]              # the empty message left last_end_time alone


def test_the_flags_of_every_case_are_what_its_name_says():
    names = [c["name"] for c in pc.all_cases() + pc.refused_cases()]
    assert len(set(names)) == len(names)
    for c in pc.all_cases():
        ws = pk.decode_case(c)
        assert all(w["status"] == "ok" for w in ws), c["name"]
        assert any(w["has_ties"] for w in ws) == c["ties"] == (c["name"] in pc.TIE_CASES), c["name"]
        assert ws[0]["given"] == (0 if c["name"].startswith("yaw_") else 1), c["name"]
