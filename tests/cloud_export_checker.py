"""Sequential restatement of the three loops that build the reference's coloured cloud -- lioOptimization::pubColorPoints
(src/lioOptimization.cpp:1210-1241), threadPubColorPoints (:1243-1344) and saveColorPoints (:1386-1426) -- over the registered state of a
tests/render_checker.py RenderChecker, one point after the other, and of threadPubColorPoints' topic schedule.  What the device export
(srl_color_map_export_cloud) and the records of tests/golden/golden_color_cloud.npz are compared with;
tests/test_cloud_export_checker_reference.py pins the loops to the reference's own rgbPoint (constructor, updateRgb, getPosition, getRgb).

A record is what the loops assign to a pcl::PointXYZRGB: x, y, z = (float) getPosition()[k] -- the stored float again --, r = getRgb()[2],
g = getRgb()[1], b = getRgb()[0] converted to a byte, and a = 255 as PCL's constructor leaves it; 16 bytes with the colour word holding
b, g, r, a from the low byte.  The byte is defined as the low 8 bits of the int16 colour: the reference's double -> uint8_t for 0 ... 255,
where updateRgb keeps the colours of the scenes (asserted in the tests).

The loops' index arithmetic cannot be asked of the reference (the functions need ROS and PCL): `for (i = 0; i < size; i++)` (:1217,
:1275), `for (i = size - 1; i > 0; i--)` (:1398) and the schedule (:1262-1342) are restated here by hand, line by line.
"""
import functools
import math

import numpy as np

import render_checker as rk

CLOUD_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1")])
TOTALS = ("scanned", "published", "below_views", "stale")
MINIMUM_VIEWS = (-1, 0, 1, 2, 3, 9)
PUB, THREAD_PUB, SAVE = 0, 1, 2


class Registered:
    """rgb_points_vec as the loops read it: per registered point the stored position, rgb, N_rgb and last_observe_time"""

    def __init__(self, xyz, rgb, n_rgb, time):
        self.xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        self.rgb = np.ascontiguousarray(rgb, np.int16).reshape(-1, 3)
        self.n_rgb = np.ascontiguousarray(n_rgb, np.int16)
        self.time = np.ascontiguousarray(time, np.float64)
        assert len(self.xyz) == len(self.rgb) == len(self.n_rgb) == len(self.time)

    def __len__(self):
        return len(self.n_rgb)


def byte_of(v):
    """the low 8 bits of the int16"""
    return int(v) & 0xFF


def _walk(reg, indices, minimum_views, since=-math.inf):
    """the body the three loops share: (records, registered index of every record, totals)"""
    idx, colour = [], []
    tot = dict.fromkeys(TOTALS, 0)
    rgb, n_rgb, time = reg.rgb.tolist(), reg.n_rgb.tolist(), reg.time.tolist()      # Python ints and floats: the values, not their arrays
    for i in indices:
        tot["scanned"] += 1
        if n_rgb[i] < minimum_views:                                       # :1221, :1281, :1404
            tot["below_views"] += 1
            continue
        if time[i] < since:                                                # the export's own option; never true at -inf
            tot["stale"] += 1
            continue
        c = rgb[i]
        colour.append((byte_of(c[0]), byte_of(c[1]), byte_of(c[2]), 255))   # .b = getRgb()[0], .g = getRgb()[1], .r = getRgb()[2] (:1228-1230)
        idx.append(i)
        tot["published"] += 1
    idx = np.array(idx, dtype=np.int32).reshape(-1)
    rec = np.zeros(len(idx), dtype=CLOUD_DTYPE)
    rec["x"], rec["y"], rec["z"] = reg.xyz[idx, 0], reg.xyz[idx, 1], reg.xyz[idx, 2]      # the stored floats, as they are
    colour = np.array(colour, dtype=np.uint8).reshape(-1, 4)
    rec["b"], rec["g"], rec["r"], rec["a"] = colour[:, 0], colour[:, 1], colour[:, 2], colour[:, 3]
    return rec, idx, tot


def pub_color_points(reg, minimum_views, since=-math.inf):
    """:1217  for (int i = 0; i < rgb_points_vec.size(); i++)"""
    return _walk(reg, range(0, len(reg)), minimum_views, since)


def save_color_points(reg, minimum_views, since=-math.inf):
    """:1398  for (long i = point_size - 1; i > 0; i--): index 0 is never saved"""
    indices = []
    i = len(reg) - 1
    while i > 0:
        indices.append(i)
        i -= 1
    return _walk(reg, indices, minimum_views, since)


class TopicSchedule:
    """the two ints threadPubColorPoints carries from round to round (:1246-1247)"""

    def __init__(self):
        self.sleep_time_after_pub = 10
        self.number_of_points_per_topic = 1000

    def round(self, published):
        """one pass of the while loop for `published` kept points: the sizes of the topics sent, in order (:1262-1342)"""
        sizes = []
        pub_index_size = 0
        cur_topic_index = 0
        for _ in range(published):
            pub_index_size += 1                                             # :1295
            if pub_index_size == self.number_of_points_per_topic:          # :1297
                sizes.append(pub_index_size)                                # the cloud still has number_of_points_per_topic points
                pub_index_size = 0
                cur_topic_index += 1
        sizes.append(pub_index_size)                                        # :1319 resize(pub_index_size), :1334 publish -- always
        cur_topic_index += 1
        if cur_topic_index >= 45:                                           # :1338
            self.number_of_points_per_topic = int(self.number_of_points_per_topic * 1.5)      # int *= 1.5: the double product, truncated
            self.sleep_time_after_pub = int(self.sleep_time_after_pub * 1.5)
        assert cur_topic_index == len(sizes)
        return sizes


def thread_pub_color_points(reg, minimum_views, schedule):
    """:1275  for (int i = 0; i < points_size; i++), the kept points filling one topic after the other: (records, indices, totals, topic
    sizes).  The topics are consecutive slices of pubColorPoints' cloud."""
    rec, idx, tot = _walk(reg, range(0, len(reg)), minimum_views)
    return rec, idx, tot, schedule.round(len(rec))


def export(reg, first=0, count=-1, minimum_views=1, reverse=False, since=-math.inf):
    """srl_color_map_export_cloud's range and order in the loops' terms"""
    size = len(reg)
    if count < 0:
        count = size - first
    assert 0 <= first and first + count <= size
    indices = range(first, first + count)
    return _walk(reg, reversed(indices) if reverse else indices, minimum_views, since)


def totals_tuple(tot):
    return tuple(int(tot[name]) for name in TOTALS)


# ------------------------------------------------------------------------------------------------ the scene: render_checker's
@functools.lru_cache(maxsize=None)
def scene_registered():
    """the registered state after each of the render scene's six renders"""
    rc, _, _, reg_states = rk.scene_sequence()
    xyz = rc.map.registered_arrays()[0]
    return tuple(Registered(xyz, rgb, n_rgb, time) for (rgb, n_rgb, _, _, time) in reg_states)


def never_rendered():
    """the scene's map before any render: rgbPoint::reset() everywhere"""
    chk, _ = rk.scene_map()
    xyz = chk.registered_arrays()[0]
    n = len(xyz)
    return Registered(xyz, np.zeros((n, 3), np.int16), np.zeros(n, np.int16), np.zeros(n))


@functools.lru_cache(maxsize=None)
def scene_export(k, minimum_views, reverse, since=-math.inf, first=0, count=-1):
    return export(scene_registered()[k], first, count, minimum_views, reverse, since)


class _RecordingState(rk.RgbState):
    """an RgbState that keeps the arguments of every updateRgb it was given"""
    __slots__ = ("log",)

    def __init__(self):
        super().__init__()
        self.log = []

    def update_rgb(self, colour, observe_distance, observe_time):
        self.log.append((float(colour[0]), float(colour[1]), float(colour[2]), float(observe_distance), float(observe_time)))
        return super().update_rgb(colour, observe_distance, observe_time)


@functools.lru_cache(maxsize=None)
def scene_observations():
    """the scene's sequence once more with recording states: per render k, per registered point, how many of its observations (the
    arguments of its updateRgb calls, refused ones included) had been made after render k, and the observations themselves.  Returns
    (counts (renders, n) int64, observations: one (m, 5) array per registered point)."""
    chk, visited = rk.scene_map()
    rc = rk.RenderChecker(chk)
    keep = rk.RgbState
    rk.RgbState = _RecordingState
    try:
        items = [(r[3], r[4]) for r in chk.registered]
        counts = np.zeros((len(rk.RENDERS), len(items)), np.int64)
        for k in range(len(rk.RENDERS)):
            cam, which, obs_time, voxels = rk.render_call(k, visited)
            rc.render(cam, rk.scene_image(which), voxels, obs_time)
            counts[k] = [len(rc.state[it].log) if it in rc.state else 0 for it in items]
    finally:
        rk.RgbState = keep
    obs = [np.array(rc.state[it].log, np.float64).reshape(-1, 5) if it in rc.state else np.zeros((0, 5)) for it in items]
    # the recording changed nothing
    assert rk.state_bytes(rc.registered_state()) == rk.state_bytes(rk.scene_sequence()[3][-1])
    return counts, obs


# ------------------------------------------------------------------------------------------------ the golden file's layout
# (render, minimum_views, reverse, since, first): an early render ascending, the last one as saveColorPoints walks it, and the time cut
GOLDEN_CALLS = ((1, 1, False, -math.inf, 0), (5, 3, True, -math.inf, 1), (5, 0, False, 10.3, 0))


def golden_pack():
    out = {"calls": np.array([[c[0], c[1], int(c[2]), c[4]] for c in GOLDEN_CALLS], np.int64), "since": np.array([c[3] for c in GOLDEN_CALLS])}
    for n, (k, mv, reverse, since, first) in enumerate(GOLDEN_CALLS):
        rec, idx, tot = scene_export(k, mv, reverse, since, first)
        out["g%d_records" % n] = rec
        out["g%d_index" % n] = idx
        out["g%d_totals" % n] = np.array(totals_tuple(tot), np.int64)
    return out
