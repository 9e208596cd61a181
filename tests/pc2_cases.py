"""PointCloud2 messages for the tests of srl_pc2_decode (csrc/srl_pc2.hip) and srl_lio_feed_pointcloud2.

A case is a dict: name, lidar_type (2 VELO, 3 OUST, 4 ROBO), msgs -- a list of dict(data (uint8), layout (Pc2Layout), stamp, points) fed in
turn to ONE decoder, so that last_end_time carries from message to message as it does in the node (it starts at -1) --, n_scans, scan_rate,
unit (0 s, 1 ms, 2 us, 3 ns), blind, pfn (point_filter_num) and ties: True where two points of one message share a sort key.  Those are
the cases whose order the reference's std::sort does not define; TIE_CASES names them.  MULTISET_CASES are the tie cases that can still
be held against the reference as a multiset (point_filter_num 1 and every point passing the last_end_time test).  REFUSED names the cases
srl_pc2_decode refuses on the device; the reference has no defined behaviour for them and is never called on them.
Sizes are the smallest at which the code can go wrong: 1 and 2, around a wave (63-65), around a scan / radix tile (1023-1025), more than
two tiles (2049), and one message beyond the one-launch bound of the scan and the radix pass (131 073).
"""
import numpy as np

from sr_livo_amd import capi

VELO, OUST, ROBO = capi.LIDAR_VELO, capi.LIDAR_OUST, capi.LIDAR_ROBO
N_SCANS = 16
F32 = np.float32
STAMP = {VELO: 1000.25, OUST: 1000.25, ROBO: 1.7e9 + 0.125}
UNIT = {VELO: 0, OUST: 3, ROBO: 0}           # velodyne: seconds as float; ouster: nanoseconds; robosense: absolute seconds as double
ROBO_BASE = 1.7e9 + 0.125


def up(v):
    return np.nextafter(F32(v), F32(np.inf))


def down(v):
    return np.nextafter(F32(v), F32(-np.inf))


def make_points(lidar_type, n, seed, order="shuffled"):
    """n points with DISTINCT positive times inside 90 ms (shuffled: the sort has work to do), coordinates well outside the default blind
    range, rings below N_SCANS"""
    rng = np.random.default_rng(seed)
    p = np.zeros(n, dtype=capi.PC2_POINT_DTYPES[lidar_type])
    r = 2.0 + 40.0 * rng.random(n)
    a = 2.0 * np.pi * rng.random(n)
    p["x"], p["y"], p["z"] = (r * np.cos(a)).astype(F32), (r * np.sin(a)).astype(F32), (-3.0 + 6.0 * rng.random(n)).astype(F32)
    p["ring"] = rng.integers(0, N_SCANS, n)
    k = np.arange(n, dtype=np.int64)
    if order == "shuffled":
        k = rng.permutation(n).astype(np.int64)
    elif order == "descending":
        k = k[::-1].copy()
    if lidar_type == VELO:
        p["time"] = ((k + 1) * (0.09 / max(n, 1))).astype(F32)
    elif lidar_type == OUST:
        p["time"] = ((k + 1) * (90_000_000 // max(n, 1))).astype(np.uint32)
    else:
        p["time"] = ROBO_BASE + (k + 1) * (0.09 / max(n, 1))
    assert len(np.unique(p["time"])) == n
    return p


def make_ring_sweep(n, seed, rings=1, start_deg=30.0, span_deg=300.0):
    """a Velodyne message without per-point time (time = 0: the yaw branch): n points whose yaw angle DEcreases from start_deg over span_deg
    (the reference's rule gives increasing relative_time for decreasing yaw), dealt to `rings` rings in turn, at distinct angles"""
    rng = np.random.default_rng(seed)
    p = np.zeros(n, dtype=capi.PC2_POINT_DTYPES[VELO])
    ang = np.deg2rad(start_deg - span_deg * (np.arange(n) + rng.random(n) * 0.5) / max(n, 1))
    r = 3.0 + 20.0 * rng.random(n)
    p["x"], p["y"], p["z"] = (r * np.cos(ang)).astype(F32), (r * np.sin(ang)).astype(F32), (-2.0 + 4.0 * rng.random(n)).astype(F32)
    p["ring"] = np.arange(n) % rings
    perm = np.concatenate([[0], 1 + rng.permutation(n - 1)]) if n > 1 else np.array([0])     # message order is not angle order
    return p[perm]


def message(lidar_type, points, stamp=None, **layout):
    data, lay = capi.pc2_message(points, lidar_type, **layout)
    data.setflags(write=False)
    return dict(data=data, layout=lay, stamp=float(STAMP[lidar_type] if stamp is None else stamp), points=points)


def _case(name, lidar_type, msgs, n_scans=N_SCANS, scan_rate=10, unit=None, blind=0.5, pfn=1, ties=False):
    return dict(name=name, lidar_type=lidar_type, msgs=list(msgs), n_scans=int(n_scans), scan_rate=int(scan_rate),
                unit=int(UNIT[lidar_type] if unit is None else unit), blind=float(blind), pfn=int(pfn), ties=bool(ties))


VELO_ALIGNED = dict(point_step=32, offsets=dict(x=0, y=4, z=8, ring=16, time=20))        # every field on its natural alignment
ROBO_ALIGNED = dict(point_step=32, offsets=dict(x=0, y=4, z=8, ring=16, time=24))
VELO_ODD = dict(point_step=23, offsets=dict(x=1, y=5, z=9, time=13, ring=17))            # nothing aligned, not even the points


def _sizes():
    out = []
    for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049):
        for lt, tag in ((VELO, "velo"), (OUST, "oust"), (ROBO, "robo")):
            out.append(_case(f"{tag}_size_{n}", lt, [message(lt, make_points(lt, n, 100 * lt + n))]))
    # the two-launch scan and radix path, through the two-round 64-bit sort
    out.append(_case("robo_size_131073", ROBO, [message(ROBO, make_points(ROBO, 131073, 7))], pfn=3))
    return out


def _filter_counts():
    out = []
    for n in (30, 31, 32):
        out.append(_case(f"velo_pfn3_n{n}", VELO, [message(VELO, make_points(VELO, n, 500 + n))], pfn=3))
    for n in (40, 41, 43):
        out.append(_case(f"oust_pfn4_n{n}", OUST, [message(OUST, make_points(OUST, n, 600 + n))], pfn=4))
    out.append(_case("robo_pfn_beyond_n", ROBO, [message(ROBO, make_points(ROBO, 5, 700))], pfn=7))
    return out


def _per_type():
    out = []
    # VELO: negative times and -0.0f in front of a positive last one (no +0.0f: that would tie with -0.0f)
    p = make_points(VELO, 90, 31)
    p["time"][:40] = -p["time"][:40]
    p["time"][40] = F32(-0.0)
    assert p["time"][-1] > 0
    out.append(_case("velo_negative_times", VELO, [message(VELO, p)]))
    # ... and both zeros, three of each: equal keys, message order
    p = make_points(VELO, 90, 32)
    p["time"][:30] = -p["time"][:30]
    p["time"][[31, 50, 33]] = F32(-0.0)
    p["time"][[32, 34, 49]] = F32(0.0)
    out.append(_case("velo_signed_zeros", VELO, [message(VELO, p)], ties=True))
    p = make_points(VELO, 90, 33)
    p["time"][[31, 50, 33]] = F32(-0.0)
    p["time"][[32, 34, 49]] = F32(0.0)
    out.append(_case("velo_signed_zeros_pfn3", VELO, [message(VELO, p)], pfn=3, ties=True))
    # OUST: t with the top bit set, up to 2^32 - 1
    p = make_points(OUST, 300, 34)
    p["time"] = (np.uint64(2 ** 32 - 1) - np.random.default_rng(34).permutation(300).astype(np.uint64) * np.uint64(7_000_003)).astype(np.uint32)
    assert int(p["time"].min()) >= 2 ** 31 and int(p["time"].max()) == 2 ** 32 - 1 and len(np.unique(p["time"])) == 300
    out.append(_case("oust_top_bit", OUST, [message(OUST, p)], pfn=3))
    # OUST: 64 columns of 16 rings, one t per column, staggered as the driver staggers them
    p = make_points(OUST, 1024, 35)
    col = np.arange(1024) // 16
    p["time"] = ((np.random.default_rng(35).permutation(64)[col] + 1) * 1_400_000).astype(np.uint32)
    p["ring"] = np.arange(1024) % 16
    out.append(_case("oust_columns", OUST, [message(OUST, p)], ties=True))
    out.append(_case("oust_columns_pfn3", OUST, [message(OUST, p)], pfn=3, ties=True))
    # ROBO: stamps 100 ns apart near 1.7e9: one high word, the order is all in the low word
    p = make_points(ROBO, 500, 36)
    p["time"] = ROBO_BASE + np.random.default_rng(36).permutation(500) * 2.0 ** -22
    hi = np.ascontiguousarray(p["time"]).view(np.uint64) >> np.uint64(32)
    assert len(np.unique(hi)) == 1 and len(np.unique(p["time"])) == 500
    out.append(_case("robo_low_word", ROBO, [message(ROBO, p)]))
    # ... and stamps that need both words (negative, small and large ones), relative to a front that is not the message's first point
    p = make_points(ROBO, 64, 37)
    p["time"] = np.random.default_rng(37).permutation(np.concatenate([-np.logspace(-3, 9, 20), [-0.0], np.logspace(-300, 9.3, 43)]))
    p["time"][-1] = 5.0
    assert len(np.unique(p["time"])) == 64
    out.append(_case("robo_both_words", ROBO, [message(ROBO, p)], unit=1))
    # the dt_last_point quirk: last_end_time = stamp + ABSOLUTE last stamp, so a second message 0.1 s later lies wholly before it
    out.append(_case("robo_dt_last_point_quirk", ROBO, [message(ROBO, make_points(ROBO, 40, 38)), message(ROBO, make_points(ROBO, 40, 39), stamp=STAMP[ROBO] + 0.1)]))
    return out


def _layouts():
    out = []
    out.append(_case("velo_step32_aligned", VELO, [message(VELO, make_points(VELO, 130, 41), **VELO_ALIGNED)]))
    out.append(_case("velo_step23_odd_offsets", VELO, [message(VELO, make_points(VELO, 130, 42), **VELO_ODD)]))
    out.append(_case("robo_step32_aligned", ROBO, [message(ROBO, make_points(ROBO, 130, 43), **ROBO_ALIGNED)]))
    out.append(_case("robo_step48", ROBO, [message(ROBO, make_points(ROBO, 130, 44), point_step=48, offsets=dict(x=4, y=8, z=12, ring=22, time=30))]))
    out.append(_case("oust_rows_padded", OUST, [message(OUST, make_points(OUST, 16 * 70, 45), height=16, row_pad=7)], pfn=3))
    out.append(_case("velo_rows_padded", VELO, [message(VELO, make_points(VELO, 4 * 33, 46), height=4, row_pad=64)]))
    out.append(_case("robo_rows_padded", ROBO, [message(ROBO, make_points(ROBO, 3 * 50, 47), height=3, row_pad=5)]))
    return out


def _blind():
    # ranges at and around blind (1.5: exact in float and double, so is its square)
    rows = [(1.5, 0.0, 0.0), (up(1.5), 0.0, 0.0), (down(1.5), 0.0, 0.0), (0.9, 1.2, 0.0), (0.9, up(1.2), 0.0), (0.9, 0.0, 1.2), (0.9, 0.0, down(1.2)),
            (1.0, 1.0, 0.5), (1.0, up(1.0), 0.5), (0.0, 0.0, 0.0), (-1.5, 0.0, 0.0), (0.0, down(-1.5), 0.0), (np.nan, 3.0, 3.0), (3.0, 3.0, np.inf)]
    p = make_points(VELO, len(rows), 51)
    for i, r in enumerate(rows):
        p[i]["x"], p[i]["y"], p[i]["z"] = F32(r[0]), F32(r[1]), F32(r[2])
    return [_case("blind_edges", VELO, [message(VELO, p)], blind=1.5),
            _case("blind_negative", OUST, [message(OUST, make_points(OUST, 50, 52))], blind=-2.0)]


def _overlap():
    # the second message starts before the first one's end: the last_end_time test drops its prefix
    a, b = make_points(VELO, 200, 61), make_points(VELO, 200, 62)
    c, d = make_points(OUST, 200, 63), make_points(OUST, 200, 64)
    return [_case("velo_overlap", VELO, [message(VELO, a), message(VELO, b, stamp=STAMP[VELO] + 0.06), message(VELO, b[:0], stamp=STAMP[VELO] + 0.07),
                                         message(VELO, a, stamp=STAMP[VELO] + 0.1)], pfn=3),
            _case("oust_overlap", OUST, [message(OUST, c), message(OUST, d, stamp=STAMP[OUST] + 0.03)])]


def _yaw():
    out = []
    # single ring: no two points share a relative_time (only the first has 0), so the reference's order is defined
    for n in (1, 2, 65, 1025):
        out.append(_case(f"yaw_single_ring_{n}", VELO, [message(VELO, make_ring_sweep(n, 800 + n))]))
    out.append(_case("yaw_single_ring_pfn4", VELO, [message(VELO, make_ring_sweep(203, 71))], pfn=4))
    # the last time decides alone: everything else is positive here, the last one 0, negative, NaN
    for tag, last in (("zero", 0.0), ("negative", -1.0), ("nan", np.nan)):
        p = make_ring_sweep(120, 72)
        p["time"] = make_points(VELO, 120, 72)["time"]
        p["time"][-1] = F32(last)
        out.append(_case(f"yaw_velo_last_{tag}", VELO, [message(VELO, p)]))
    # Ouster and RoboSense messages without time: the same branch through their own field types (uint8 ring; the double at offset 18)
    p = np.zeros(150, dtype=capi.PC2_POINT_DTYPES[OUST]); q = make_ring_sweep(150, 73)
    for f in ("x", "y", "z", "ring"):
        p[f] = q[f]
    out.append(_case("yaw_oust_single_ring", OUST, [message(OUST, p)]))
    p = np.zeros(150, dtype=capi.PC2_POINT_DTYPES[ROBO]); q = make_ring_sweep(150, 74)
    for f in ("x", "y", "z", "ring"):
        p[f] = q[f]
    p["time"][:-1] = ROBO_BASE                                                   # only the last one counts
    out.append(_case("yaw_robo_single_ring", ROBO, [message(ROBO, p)]))
    # a wrap through +-180 degrees: the first point at 170, the sweep runs down through 0 and -180 to 175
    out.append(_case("yaw_wrap_180", VELO, [message(VELO, make_ring_sweep(300, 75, start_deg=170.0, span_deg=354.0))]))
    # the other sense of rotation: every yaw is above the first one, the + 360.0 branch
    p = make_ring_sweep(100, 76, start_deg=-100.0, span_deg=-200.0)
    out.append(_case("yaw_increasing", VELO, [message(VELO, p)]))
    # the ring-first quirk: timestamp 0.0 passes only while last_end_time is still -1
    out.append(_case("yaw_first_point_quirk", VELO, [message(VELO, make_ring_sweep(90, 77)), message(VELO, make_ring_sweep(90, 78), stamp=STAMP[VELO] + 0.1)]))
    # 16 rings: sixteen points tie at relative_time 0
    out.append(_case("yaw_16_rings", VELO, [message(VELO, make_ring_sweep(16 * 40, 79, rings=16))], ties=True))
    out.append(_case("yaw_16_rings_pfn3", VELO, [message(VELO, make_ring_sweep(16 * 40, 80, rings=16))], pfn=3, ties=True))
    out.append(_case("yaw_16_rings_two_messages", VELO, [message(VELO, make_ring_sweep(16 * 20, 81, rings=16)),
                                                          message(VELO, make_ring_sweep(16 * 20, 82, rings=16), stamp=STAMP[VELO] + 0.1)], ties=True))
    # a duplicate of the ring's first point: yaw == yaw_first, relative_time +0.0 beside the first point's 0.0
    p = make_ring_sweep(60, 83)
    p[[7, 31]] = p[0]
    out.append(_case("yaw_duplicate_of_first", VELO, [message(VELO, p)], ties=True))
    return out


def _refused():
    out = []
    p = make_ring_sweep(200, 91, rings=16)
    p["ring"][150] = N_SCANS
    out.append(_case("refused_ring_eq_n_scans", VELO, [message(VELO, p)]))
    p = make_ring_sweep(200, 92, rings=16)
    p["x"][170] = np.nan
    out.append(_case("refused_yaw_nan_coordinate", VELO, [message(VELO, p)]))
    p = make_points(VELO, 1100, 93)
    p["time"][1050] = np.nan
    out.append(_case("refused_velo_nan_time", VELO, [message(VELO, p)]))
    p = make_points(ROBO, 70, 94)
    p["time"][3] = -np.nan
    out.append(_case("refused_robo_nan_time", ROBO, [message(ROBO, p)]))
    return out


_CASES = None
_REFUSED = None


def all_cases():
    """the cases srl_pc2_decode accepts; built once; nobody changes a case's arrays"""
    global _CASES
    if _CASES is None:
        _CASES = _sizes() + _filter_counts() + _per_type() + _layouts() + _blind() + _overlap() + _yaw()
    return _CASES


def refused_cases():
    global _REFUSED
    if _REFUSED is None:
        _REFUSED = _refused()
    return _REFUSED


TIE_CASES = ("velo_signed_zeros", "velo_signed_zeros_pfn3", "oust_columns", "oust_columns_pfn3", "yaw_16_rings", "yaw_16_rings_pfn3",
             "yaw_16_rings_two_messages", "yaw_duplicate_of_first")
# of those: point_filter_num 1 and every point of every message passes the last_end_time test -- equal to the reference as a multiset
MULTISET_CASES = ("velo_signed_zeros", "oust_columns", "yaw_16_rings", "yaw_duplicate_of_first")


def exact_cases():
    """what is compared with the reference record by record, in order: everything but the named tie cases"""
    return [c for c in all_cases() if c["name"] not in TIE_CASES]


def multiset_cases():
    return [c for c in all_cases() if c["name"] in MULTISET_CASES]


def case_by_name(name):
    for c in all_cases() + refused_cases():
        if c["name"] == name:
            return c
    raise KeyError(name)
