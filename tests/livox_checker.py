"""Independent restatement of the point side of the node, in NumPy and plain Python, for the tests of csrc/srl_points.hip:

  decode        cloudProcessing::livoxHandler (cloudProcessing.cpp:125-214) with the library's STABLE tie order
  PointQueue    std::queue<point3D> point_buffer with the prefix cut of getMeasurements (lioOptimization.cpp:719-723, :759-763)
  rewrite_times lioOptimization::makePointTimestamp (:786-819)
  interval_walk the loop of distortFrameByImu (utility.cpp:247-305), as a loop
  interval_rule the closed form srl_frame_undistort_cut evaluates per point on the device

Nothing here calls the library.  The tie order is a specification of this project, not a property of the reference: std::sort is not
stable, so wherever two valid points share an offset_time the reference's order is its standard library's own.
"""
import numpy as np

POINT_DTYPE = np.dtype([("offset_time", "<u4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("reflectivity", "u1"), ("tag", "u1"),
                        ("line", "u1"), ("pad", "u1")])
assert POINT_DTYPE.itemsize == 20


def time_unit_scale(unit):
    """cloudProcessing::setTimeUnit: a FLOAT literal assigned to a double member"""
    return float(np.float32({0: 1.e3, 1: 1.0, 2: 1.e-3, 3: 1.e-6}.get(int(unit), 1.0)))


def valid_mask(pts, n_scans):
    """cloudProcessing.cpp:136-150 for every message index (index 0 is never looked at)"""
    n = len(pts)
    ok = np.zeros(n, dtype=bool)
    if n < 2:
        return ok
    x, y, z = pts["x"], pts["y"], pts["z"]
    with np.errstate(invalid="ignore", over="ignore"):
        xd, yd, zd = x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)
        m = pts["line"].astype(np.int64) < int(n_scans)
        m &= ~(np.abs(x).astype(np.float64) > 1e8) & ~(np.abs(y).astype(np.float64) > 1e8) & ~(np.abs(z).astype(np.float64) > 1e8)
        m &= xd > 0.7
        tagged = ((pts["tag"] & 0x03) != 0) | ((pts["tag"] & 0x0C) != 0)
        m &= ~((xd > 2.0) & tagged)
        # float subtraction against the previous MESSAGE point, magnitude compared as double
        dx = np.abs((x[1:] - x[:-1]).astype(np.float32)).astype(np.float64)
        dy = np.abs((y[1:] - y[:-1]).astype(np.float32)).astype(np.float64)
        dz = np.abs((z[1:] - z[:-1]).astype(np.float32)).astype(np.float64)
        moved = (dx > 1e-7) | (dy > 1e-7) | (dz > 1e-7)
    ok[1:] = m[1:] & moved
    return ok


def decode(pts, header_stamp, n_scans, scale, blind, point_filter_num):
    """-> dict(records (k, 5): x y z relative_time timestamp of the appended points in queue order, valid, picked, appended,
    last_end_time (NaN without a valid point), first_timestamp, last_timestamp, has_ties (two valid points share an offset))"""
    pts = np.asarray(pts, dtype=POINT_DTYPE)
    idx = np.flatnonzero(valid_mask(pts, n_scans))
    off = pts["offset_time"][idx]
    order = np.argsort(off, kind="stable")                     # ties keep message order
    idx, off = idx[order], off[order]
    rel = off.astype(np.float64) * float(scale)
    ts = rel / 1000.0 + float(header_stamp)
    rows = []
    picked = 0
    b2 = float(blind) * float(blind)
    num_valid = 0
    for j in range(len(idx)):                                  # cloudProcessing.cpp:186-197, as written
        num_valid += 1
        if num_valid % int(point_filter_num) != 0:
            continue
        picked += 1
        p = pts[idx[j]]
        x, y, z = float(p["x"]), float(p["y"]), float(p["z"])
        if x * x + y * y + z * z > b2:
            rows.append((x, y, z, rel[j], ts[j]))
    rec = np.array(rows, dtype=np.float64).reshape(-1, 5)
    nan = float("nan")
    return dict(records=rec, valid=len(idx), picked=picked, appended=len(rec),
                last_end_time=float(header_stamp) + rel[-1] / 1000.0 if len(idx) else nan,
                first_timestamp=rec[0, 4] if len(rec) else nan, last_timestamp=rec[-1, 4] if len(rec) else nan,
                has_ties=bool(len(off) > 1 and np.any(off[1:] == off[:-1])))


class PointQueue:
    """point_buffer: records (x y z relative_time timestamp) in arrival order"""

    def __init__(self):
        self.rec = np.empty((0, 5))

    def push(self, records):
        self.rec = np.vstack([self.rec, np.asarray(records, dtype=np.float64).reshape(-1, 5)])

    def info(self):
        if len(self.rec) == 0:
            return 0, float("nan"), float("nan")
        return len(self.rec), float(self.rec[0, 4]), float(self.rec[-1, 4])

    def clear(self):
        self.rec = np.empty((0, 5))

    def cut(self, t):
        """while (front().timestamp < t) pop -- defined on an empty queue too: everything is cut"""
        c = 0
        while c < len(self.rec) and self.rec[c, 4] < t:
            c += 1
        out, self.rec = self.rec[:c].copy(), self.rec[c:].copy()
        return out


def rewrite_times(timestamp, time_begin, time_end, point_time_enable):
    """makePointTimestamp -> (kept indices, relative_time ms, alpha_time)"""
    ts = np.asarray(timestamp, dtype=np.float64)
    delta_t = float(time_end) - float(time_begin)
    keep, rel, alpha = [], [], []
    for i in range(len(ts)):
        if not point_time_enable and (ts[i] > time_end or ts[i] < time_begin):
            continue
        r = ts[i] - float(time_begin)
        with np.errstate(divide="ignore", invalid="ignore"):
            a = np.float64(r) / np.float64(delta_t)
        r = r * 1000.0
        if point_time_enable and a > 1.0:
            a = 1.0 - 1e-5
        keep.append(i); rel.append(r); alpha.append(float(a))
    return np.array(keep, dtype=np.int64), np.array(rel, dtype=np.float64), np.array(alpha, dtype=np.float64)


def interval_walk(relative_time_ms, stamps, time_frame_begin):
    """distortFrameByImu's loop: -> interval per point, -1 = never reached"""
    return np.array(walk_list(np.asarray(relative_time_ms, dtype=np.float64).tolist(), np.asarray(stamps, dtype=np.float64).tolist(),
                              float(time_frame_begin)), dtype=np.int32)


def walk_list(rel, stamps, tfb):
    """the walk on Python floats (IEEE doubles, one rounding per operation)"""
    n = len(rel)
    seg = [-1] * n
    it = 0
    for k in range(len(stamps) - 1):
        tb, te = stamps[k], stamps[k + 1]
        while it != n:
            t = tfb + rel[it] / 1000.0
            if t > tb - 1e-6 and t < te + 1e-6:
                seg[it] = k
                it += 1
            else:
                break
    return seg


def rule_list(rel, stamps, tfb):
    n = len(rel)
    seg = [-1] * n
    for i in range(n):
        t = tfb + rel[i] / 1000.0
        for k in range(len(stamps) - 1):
            if t < stamps[k + 1] + 1e-6:
                if t > stamps[k] - 1e-6:
                    seg[i] = k
                break
        if seg[i] < 0:
            break                                              # this point and every point behind it: -1
    return seg


def interval_rule(relative_time_ms, stamps, time_frame_begin):
    """k(i) = the smallest k with t_i < stamp[k + 1] + 1e-6, accepted iff t_i > stamp[k] - 1e-6; the first point without an accepted interval
    and every point behind it get -1.  Equal to interval_walk where the times and the stamps are non-decreasing."""
    return np.array(rule_list(np.asarray(relative_time_ms, dtype=np.float64).tolist(), np.asarray(stamps, dtype=np.float64).tolist(),
                              float(time_frame_begin)), dtype=np.int32)


def preconditions_hold(relative_time_ms, stamps):
    rel = np.asarray(relative_time_ms, dtype=np.float64)
    stamps = np.asarray(stamps, dtype=np.float64)
    return bool(np.all(rel[:-1] <= rel[1:])) and bool(np.all(stamps[:-1] <= stamps[1:]))
