"""Independent restatement, in NumPy and plain Python, of the PointCloud2 side of cloudProcessing for the tests of csrc/srl_pc2.hip:

  decode   cloudProcessing::process (cloudProcessing.cpp:100-123) with velodyneHandler (:325-433), ousterHandler (:216-323) and
           robosenseHandler (:435-542), plus this library's specification where the reference has none: ties keep message order, and the
           inputs the reference has no defined behaviour for are refused.

Nothing here calls the library.  Fields are read from the message's bytes at the layout's offsets, whatever their alignment.  The yaw
angle is math.atan2 per point (the platform's libm, what the reference calls), NOT np.arctan2: NumPy may dispatch to a SIMD
implementation with other last bits.  The tie order is a specification of this project, not a property of the reference: std::sort is not
stable.  It weighs more here than for Livox: every Ouster column shares one t, and in the yaw branch every ring's first point has
relative_time 0.
"""
import math

import numpy as np

LIVOX, VELO, OUST, ROBO = 1, 2, 3, 4
TIME_DTYPE = {VELO: "<f4", OUST: "<u4", ROBO: "<f8"}
RING_DTYPE = {VELO: "<u2", OUST: "u1", ROBO: "<u2"}


def time_unit_scale(unit):
    """cloudProcessing::setTimeUnit: a FLOAT literal assigned to a double member"""
    return float(np.float32({0: 1.e3, 1: 1.0, 2: 1.e-3, 3: 1.e-6}.get(int(unit), 1.0)))


def layout_dict(layout):
    """a ctypes srl_pc2_layout or a dict -> dict"""
    names = ("width", "height", "point_step", "row_step", "off_x", "off_y", "off_z", "off_time", "off_ring", "is_bigendian")
    return {k: int(layout[k] if isinstance(layout, dict) else getattr(layout, k)) for k in names}


def layout_ok(lay, lidar_type, data_bytes):
    """what srl_pc2_decode demands of a layout before it reads a byte"""
    if lidar_type not in TIME_DTYPE or lay["is_bigendian"] != 0:
        return False
    sizes = dict(off_x=4, off_y=4, off_z=4, off_time=np.dtype(TIME_DTYPE[lidar_type]).itemsize, off_ring=np.dtype(RING_DTYPE[lidar_type]).itemsize)
    for k, size in sizes.items():
        if lay[k] < 0 or lay[k] + size > lay["point_step"]:
            return False
    n = lay["width"] * lay["height"]
    if n > 0 and data_bytes < (lay["height"] - 1) * lay["row_step"] + (lay["width"] - 1) * lay["point_step"] + lay["point_step"]:
        return False
    return True


def field(data, lay, offset, dtype):
    """the field at byte `offset` of every point, gathered byte by byte (no alignment assumed)"""
    dt = np.dtype(dtype)
    n = lay["width"] * lay["height"]
    i = np.arange(n, dtype=np.int64)
    start = (i // max(lay["width"], 1)) * lay["row_step"] + (i % max(lay["width"], 1)) * lay["point_step"] + offset
    idx = start[:, None] + np.arange(dt.itemsize, dtype=np.int64)[None, :]
    return np.ascontiguousarray(np.asarray(data, dtype=np.uint8)[idx]).view(dt).reshape(n)


def yaw_angles(x, y):
    """cloudProcessing.cpp:263 / :372 / :482 per point: atan2(double(y), double(x)) * 57.2957 with libm"""
    return [math.atan2(float(b), float(a)) * 57.2957 for a, b in zip(x, y)]


def _refused():
    nan = float("nan")
    return dict(status="refused", records=np.empty((0, 5)), points=0, given=0, picked=0, appended=0, last_end_time=nan, first_timestamp=nan,
                last_timestamp=nan, has_ties=False, all_pass=False)


def decode(data, layout, lidar_type, header_stamp, last_end_time, n_scans, scan_rate, scale, blind, point_filter_num):
    """-> dict(status 'ok' | 'refused', records (k, 5): x y z relative_time timestamp of the appended points in queue order, points, given,
    picked, appended, last_end_time (NaN for an empty message), first_timestamp, last_timestamp, has_ties (two points share a sort key),
    all_pass (every point of the message passes the last_end_time test))"""
    lay = layout_dict(layout)
    data = np.asarray(data, dtype=np.uint8)
    stamp, last_end, scale, pfn = float(header_stamp), float(last_end_time), float(scale), int(point_filter_num)
    if not layout_ok(lay, lidar_type, data.nbytes) or pfn < 1 or not (scale > 0.0) or math.isinf(scale) or math.isnan(float(blind)) or \
            math.isnan(stamp) or math.isnan(last_end):
        return _refused()
    n = lay["width"] * lay["height"]
    nan = float("nan")
    if n == 0:
        return dict(status="ok", records=np.empty((0, 5)), points=0, given=0, picked=0, appended=0, last_end_time=nan, first_timestamp=nan,
                    last_timestamp=nan, has_ties=False, all_pass=True)
    x = field(data, lay, lay["off_x"], "<f4").astype(np.float64)
    y = field(data, lay, lay["off_y"], "<f4").astype(np.float64)
    z = field(data, lay, lay["off_z"], "<f4").astype(np.float64)
    t = field(data, lay, lay["off_time"], TIME_DTYPE[lidar_type])
    ring = field(data, lay, lay["off_ring"], RING_DTYPE[lidar_type]).astype(np.int64)
    given = bool(t[n - 1] > 0)                                 # the last record in message order, before any sort; NaN > 0 is false
    rows = []
    if given:
        if lidar_type != OUST and np.any(np.isnan(t)):
            return _refused()                                  # std::sort under < has no order with a NaN
        order = np.argsort(t, kind="stable")                   # ties (-0.0 and +0.0 among them) keep message order
        ts_sorted = t[order]
        has_ties = bool(n > 1 and np.any(ts_sorted[1:] == ts_sorted[:-1]))
        tl = [float(v) for v in ts_sorted]                     # double(float), double(uint32), the double
        front = tl[0]
        rel = [(v - front) * scale for v in tl] if lidar_type == ROBO else [v * scale for v in tl]
        ts = [r / 1000.0 + stamp for r in rel]
        dt_last_point = tl[-1] * scale                         # ROBO: the ABSOLUTE timestamp (:456), not the difference
        b2 = float(blind) * float(blind)
        for j in range(0, n, pfn):
            i = order[j]
            xi, yi, zi = float(x[i]), float(y[i]), float(z[i])
            if xi * xi + yi * yi + zi * zi > b2 and ts[j] > last_end:
                rows.append((xi, yi, zi, rel[j], ts[j]))
        all_pass = all(v > last_end for v in ts)
    else:
        if int(scan_rate) <= 0 or int(n_scans) < 1 or np.any(ring >= int(n_scans)):
            return _refused()                                  # yaw_first_point[layer] out of bounds upstream
        omega = 0.361 * int(scan_rate)
        yaw = yaw_angles(x, y)
        first = {}
        rel, ts = [0.0] * n, [0.0] * n
        for i in range(n):
            layer = int(ring[i])
            if layer not in first:
                first[layer] = yaw[i]                          # relative_time = 0.0; timestamp stays what point3D() gave it: 0.0
                continue
            if yaw[i] <= first[layer]:
                rel[i] = (first[layer] - yaw[i]) / omega
            else:
                rel[i] = (first[layer] - yaw[i] + 360.0) / omega
            ts[i] = rel[i] / 1000.0 + stamp
        if any(math.isnan(v) for v in rel):
            return _refused()
        order = sorted(range(n), key=lambda i: rel[i])         # sorted() is stable
        rs = [rel[i] for i in order]
        has_ties = any(rs[k] == rs[k + 1] for k in range(n - 1))
        dt_last_point = rs[-1]
        for j in range(0, n, pfn):                             # no blind test in this branch
            i = order[j]
            if ts[i] > last_end:
                rows.append((float(x[i]), float(y[i]), float(z[i]), rel[i], ts[i]))
        all_pass = all(v > last_end for v in ts)
    rec = np.array(rows, dtype=np.float64).reshape(-1, 5)
    return dict(status="ok", records=rec, points=n, given=int(given), picked=len(range(0, n, pfn)), appended=len(rec),
                last_end_time=stamp + dt_last_point / 1000.0, first_timestamp=rec[0, 4] if len(rec) else nan,
                last_timestamp=rec[-1, 4] if len(rec) else nan, has_ties=has_ties, all_pass=bool(all_pass))


def decode_case(case):
    """every message of a case (tests/pc2_cases.py) in turn, last_end_time carried as the node carries it -> list of decode() results"""
    out, last_end = [], -1.0
    for m in case["msgs"]:
        w = decode(m["data"], m["layout"], case["lidar_type"], m["stamp"], last_end, case["n_scans"], case["scan_rate"], time_unit_scale(case["unit"]),
                   case["blind"], case["pfn"])
        out.append(w)
        if w["status"] == "ok" and w["points"] > 0:
            last_end = w["last_end_time"]
    return out
