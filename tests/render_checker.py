"""Sequential restatement of rgbMapTracker::renderPointsInRecentVoxel / threadRenderPointsInVoxel (src/rgbMapTracker.cpp:176-237) on top of
tests/color_checker.py's map: for every point of every listed voxel cloudFrame::project3dPointInThisImage (src/lioOptimization.cpp:142-199,
if2dPointsAvailable :48-60, refreshPoseForProjection :201-205), the sub-pixel colour getSubPixel<cv::Vec3b> (:71-97) and rgbPoint::updateRgb
(src/cloudMap.cpp:59-100).  One point after the other, Python floats (IEEE doubles) with explicit np.float32 steps where the reference
holds floats, sums of three as (a0 + a1) + a2.  What the device pass (srl_color_map_render) and the recorded golden file are compared
with; tests/test_render_checker_reference.py pins updateRgb and the projection to the reference's own translation units bit for bit.

OpenCV's Vec3b arithmetic decides the colour's bits and OpenCV is not part of the reference tree:
  double * Vec3b  is a Vec3b whose channels are saturate_cast<uchar>(w * pixel): cvRound (lrint: to nearest, ties to even), clamped 0 ... 255
  Vec3b + Vec3b   is a saturating 8-bit add, applied left to right over the four terms
so the colour is a sum of four individually rounded bytes, not a rounded bilinear value.

Also the scene of the tests: color_checker.scene_batch frames in a map (option set 0), synthetic BGR images (a gradient plus seeded noise
plus a few 255-valued patches) at two sizes, and a sequence of renders at different times and poses.
"""
import functools
import math

import numpy as np

import color_checker as cc

F32 = np.float32
IMAGE_OBS_COV = 15.0              # rgbMapTracker.cpp:176
PROCESS_NOISE_SIGMA = 0.1         # cloudMap.cpp:57
TOTALS = ("listed", "behind", "outside", "gated", "first", "updated", "unknown")


# ------------------------------------------------------------------------------------------------ OpenCV's byte arithmetic
def sat8(w, pixel):
    """saturate_cast<uchar>(w * pixel): Python's round() is round-half-even on the exact double, as lrint is"""
    r = round(w * float(pixel))
    return 0 if r < 0 else (255 if r > 255 else r)


def add8(a, b):
    s = a + b
    return 255 if s > 255 else s


def sub_pixel(img, row, col):
    """getSubPixel<cv::Vec3b>(mat, row, col, 0) (:71-97).  Returns (three ints, did any 8-bit add saturate).  The one neighbour the
    field-of-view test lets lie past the row or the image has weight exactly 0 and contributes 0 whatever it holds: it is read from the
    last column / row."""
    rows, cols = img.shape[0], img.shape[1]
    floor_row, floor_col = math.floor(row), math.floor(col)
    frac_row, frac_col = row - floor_row, col - floor_col
    ceil_row, ceil_col = floor_row + 1, floor_col + 1
    if ceil_row >= rows:
        assert frac_row == 0.0
        ceil_row = rows - 1
    if ceil_col >= cols:
        assert frac_col == 0.0
        ceil_col = cols - 1
    w = ((1.0 - frac_row) * (1.0 - frac_col), frac_row * (1.0 - frac_col), (1.0 - frac_row) * frac_col, frac_row * frac_col)
    px = (img[floor_row, floor_col], img[ceil_row, floor_col], img[floor_row, ceil_col], img[ceil_row, ceil_col])
    out, saturated = [], False
    for ch in range(3):
        terms = [sat8(w[k], int(px[k][ch])) for k in range(4)]
        saturated = saturated or (terms[0] + terms[1] > 255) or (add8(terms[0], terms[1]) + terms[2] > 255) or \
            (add8(add8(terms[0], terms[1]), terms[2]) + terms[3] > 255)
        out.append(add8(add8(add8(terms[0], terms[1]), terms[2]), terms[3]))
    return out, saturated


# ------------------------------------------------------------------------------------------------ updateRgb
def to_short(x):
    """(short) of a double as the reference's x86-64 build does it: cvttsd2si to 32 bits ("integer indefinite" outside), low 16 bits"""
    t = int(x) if (x == x and -2147483649.0 < x < 2147483648.0) else -2147483648
    return (t + 32768) % 65536 - 32768


class RgbState:
    """the fields of rgbPoint that updateRgb reads and writes (include/cloudMap.h:51-66); a fresh one is rgbPoint::reset()"""
    __slots__ = ("rgb", "cov", "observe_distance", "last_observe_time", "n_rgb")

    def __init__(self):
        self.rgb = [0, 0, 0]
        self.cov = [F32(0), F32(0), F32(0)]
        self.observe_distance = 0.0
        self.last_observe_time = 0.0
        self.n_rgb = 0

    def update_rgb(self, colour, observe_distance, observe_time):
        """rgbPoint::updateRgb(colour, distance, (15, 15, 15), time) (cloudMap.cpp:59-100); returns 0 / 1 as it does, and -1 where the
        distance gate returned its 0 (the caller tells the two zeros apart)"""
        if self.observe_distance != 0 and observe_distance > self.observe_distance * 1.2:
            return -1
        if self.n_rgb == 0:
            self.last_observe_time = observe_time
            self.observe_distance = observe_distance
            for i in range(3):
                self.rgb[i] = to_short(float(round(colour[i])))
                self.cov[i] = F32(IMAGE_OBS_COV)
            self.n_rgb = 1
            return 0
        for i in range(3):
            cov = F32(float(self.cov[i]) + PROCESS_NOISE_SIGMA * (observe_time - self.last_observe_time))
            old_sigma = float(cov)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                sq = float(cov * cov)                                    # an FP32 product
                inv = np.float64(1.0) / np.float64(sq) + 1.0 / (IMAGE_OBS_COV * IMAGE_OBS_COV)
                cov = F32(math.sqrt(float(np.float64(1.0) / inv)))
                self.cov[i] = cov
                value = np.float64(float(cov * cov)) * (np.float64(self.rgb[i]) / np.float64(old_sigma * old_sigma) + colour[i] / (IMAGE_OBS_COV * IMAGE_OBS_COV))
            self.rgb[i] = to_short(float(value))
        if observe_distance < self.observe_distance:
            self.observe_distance = observe_distance
        self.last_observe_time = observe_time
        self.n_rgb = (self.n_rgb + 1 + 32768) % 65536 - 32768            # an int16 as in the reference
        return 1


# ------------------------------------------------------------------------------------------------ camera
class Camera:
    """what project3dPointInThisImage reads from the frame's state: q_world_camera (w, x, y, z), t_world_camera, fx, fy, cx, cy, fov_margin"""

    def __init__(self, q, t, fx, fy, cx, cy, fov_margin=0.005):
        self.q = tuple(float(v) for v in q)
        self.t = tuple(float(v) for v in t)
        self.fx, self.fy, self.cx, self.cy, self.fov_margin = float(fx), float(fy), float(cx), float(cy), float(fov_margin)
        self.refresh_pose_for_projection()

    def refresh_pose_for_projection(self):
        """q_camera_world = q.inverse(); t_camera_world = -q_camera_world.toRotationMatrix() * t (:201-205); Eigen's quaternion
        semantics as csrc/host/srl_la.h restates them"""
        w, x, y, z = self.q
        n2 = ((x * x + y * y) + z * z) + w * w
        w, x, y, z = (w / n2, -x / n2, -y / n2, -z / n2) if n2 > 0.0 else (0.0, 0.0, 0.0, 0.0)
        tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
        twx, twy, twz = tx * w, ty * w, tz * w
        txx, txy, txz = tx * x, ty * x, tz * x
        tyy, tyz, tzz = ty * y, tz * y, tz * z
        self.R = ((1.0 - (tyy + tzz), txy - twz, txz + twy), (txy + twz, 1.0 - (txx + tzz), tyz - twx), (txz - twy, tyz + twx, 1.0 - (txx + tyy)))
        t = self.t
        self.t_cw = tuple(((-r[0]) * t[0] + (-r[1]) * t[1]) + (-r[2]) * t[2] for r in self.R)

    def project(self, p, rows, cols):
        """project3dPointInThisImage(p, u, v, nullptr, 1.0): (outcome, u, v); outcome 0 accepted, 1 behind the camera, 2 ... 5 the first
        field-of-view bound that fails (u low, u high, v low, v high)"""
        R, t = self.R, self.t_cw
        xc = ((R[0][0] * p[0] + R[0][1] * p[1]) + R[0][2] * p[2]) + t[0]
        yc = ((R[1][0] * p[0] + R[1][1] * p[1]) + R[1][2] * p[2]) + t[1]
        zc = ((R[2][0] * p[0] + R[2][1] * p[1]) + R[2][2] * p[2]) + t[2]
        if zc < 0.001:
            return 1, 0.0, 0.0
        u = (xc * self.fx / zc + self.cx) * 1.0
        v = (yc * self.fy / zc + self.cy) * 1.0
        m = self.fov_margin
        if not (u >= m * cols + 1):
            return 2, u, v
        if not (math.ceil(u) < (1 - m) * cols):
            return 3, u, v
        if not (v >= m * rows + 1):
            return 4, u, v
        if not (math.ceil(v) < (1 - m) * rows):
            return 5, u, v
        return 0, u, v

    def distance(self, p):
        dx, dy, dz = p[0] - self.t[0], p[1] - self.t[1], p[2] - self.t[2]
        return math.sqrt((dx * dx + dy * dy) + dz * dz)


# ------------------------------------------------------------------------------------------------ the loop
class RenderChecker:
    """the colour state of every stored point of a ColorChecker's map, keyed by (voxel key, slot)"""

    def __init__(self, color_checker):
        self.map = color_checker
        self.state = {}
        # outcomes over the checker's life, per point and occurrence (the preconditions of the tests)
        self.seen = dict(behind=0, u_low=0, u_high=0, v_low=0, v_high=0, gated=0, first=0, updated=0, updated_n3=0, saturated=0,
                         repeated_voxels=0, coloured=0, not_coloured=0, listed=0)

    def render(self, camera, img, voxels_xyz, obs_time):
        """threadRenderPointsInVoxel over the list, entry by entry.  Returns the totals as a dict (TOTALS)."""
        rows, cols = img.shape[0], img.shape[1]
        tot = dict.fromkeys(TOTALS, 0)
        seen = self.seen
        names = (None, "behind", "u_low", "u_high", "v_low", "v_high")
        listed_before = set()
        for entry in np.asarray(voxels_xyz, dtype=np.int64).reshape(-1, 3):
            key = (int(entry[0]), int(entry[1]), int(entry[2]))
            vox = self.map.voxels.get(key)
            if vox is None:
                tot["unknown"] += 1
                continue
            if key in listed_before:
                seen["repeated_voxels"] += 1
            listed_before.add(key)
            for slot, p32 in enumerate(vox.points):
                tot["listed"] += 1
                seen["listed"] += 1
                p = (float(p32[0]), float(p32[1]), float(p32[2]))          # getPosition(): position.cast<double>()
                outcome, u, v = camera.project(p, rows, cols)
                if outcome:
                    tot["behind" if outcome == 1 else "outside"] += 1
                    seen[names[outcome]] += 1
                    seen["not_coloured"] += 1
                    continue
                d = camera.distance(p)
                colour, saturated = sub_pixel(img, v, u)                    # getRgb(u, v, 0): getSubPixel(rgb_image, v, u, 0)
                seen["saturated"] += 1 if saturated else 0
                st = self.state.get((key, slot))
                if st is None:
                    st = self.state[(key, slot)] = RgbState()
                r = st.update_rgb([float(c) for c in colour], d, obs_time)
                if r == -1:
                    tot["gated"] += 1
                    seen["gated"] += 1
                    seen["not_coloured"] += 1
                elif r == 0:
                    tot["first"] += 1
                    seen["first"] += 1
                    seen["coloured"] += 1
                else:
                    tot["updated"] += 1
                    seen["updated"] += 1
                    seen["coloured"] += 1
                    seen["updated_n3"] += 1 if st.n_rgb >= 3 else 0
        return tot

    def _arrays(self, items):
        n = len(items)
        rgb = np.zeros((n, 3), np.int16); n_rgb = np.zeros(n, np.int16); cov = np.zeros((n, 3), np.float32)
        dist = np.zeros(n); time = np.zeros(n)
        for i, ks in enumerate(items):
            st = self.state.get(ks)
            if st is not None:
                rgb[i] = st.rgb; n_rgb[i] = st.n_rgb; cov[i] = st.cov; dist[i] = st.observe_distance; time[i] = st.last_observe_time
        return rgb, n_rgb, cov, dist, time

    def map_state(self):
        """(rgb, N_rgb, cov_rgb, observe_distance, last_observe_time) voxel after voxel in slot order: srl_color_map_download_rgb"""
        return self._arrays([(v.key, s) for v in self.map.voxels.values() for s in range(len(v.points))])

    def registered_state(self):
        """... of rgb_points_vec in order: srl_color_registered_rgb"""
        return self._arrays([(r[3], r[4]) for r in self.map.registered])


def state_bytes(arrays):
    """one bytes object per state: what a bitwise comparison compares"""
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


# ------------------------------------------------------------------------------------------------ the scene
OPT = cc.OPTION_SETS[0]
IMAGE_SIZES = ((480, 640), (375, 500))                # rows, cols; 500 is no multiple of 64
BATCH_TIMES = (1.0, 2.0, 4.0)


def scene_image(which):
    """a BGR gradient plus seeded noise (neighbouring pixels differ, so the rounding of every weighted byte matters) and a few 255-valued
    patches (the 8-bit adds saturate there)"""
    rows, cols = IMAGE_SIZES[which]
    rng = np.random.default_rng(7700 + which)
    r, c = np.mgrid[0:rows, 0:cols]
    img = np.stack([(r * 200) // rows + 20, (c * 200) // cols + 30, ((r + c) * 180) // (rows + cols) + 40], 2) + rng.integers(-20, 21, (rows, cols, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    for (fr, fc) in ((0.55, 0.3), (0.7, 0.6), (0.6, 0.8), (0.8, 0.45)):
        r0, c0 = int(fr * rows), int(fc * cols)
        img[r0:r0 + rows // 12, c0:c0 + cols // 10] = 255
    return np.ascontiguousarray(img)


def _quat_looking(yaw, pitch, roll=0.0):
    """a camera (z forward, x right, y down) that looks along world +x turned by yaw about world z and pitched down by `pitch`; the result
    is deliberately not normalised exactly (inverse() divides by the squared norm)"""
    cy_, sy_, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    fwd = np.array([cy_ * cp, sy_ * cp, -sp])
    right = np.array([sy_, -cy_, 0.0])
    down = np.cross(fwd, right)
    right, down = cr * right + sr * down, cr * down - sr * right
    m = np.stack([right, down, fwd], 1)                # columns: the camera's axes in the world
    w = math.sqrt(max(1e-12, 1.0 + m[0, 0] + m[1, 1] + m[2, 2])) / 2.0
    if w > 1e-3:
        q = (w, (m[2, 1] - m[1, 2]) / (4 * w), (m[0, 2] - m[2, 0]) / (4 * w), (m[1, 0] - m[0, 1]) / (4 * w))
    else:                                               # a half turn: x is the largest component for the poses used here
        x = math.sqrt(max(1e-12, 1.0 + m[0, 0] - m[1, 1] - m[2, 2])) / 2.0
        q = ((m[2, 1] - m[1, 2]) / (4 * x), x, (m[0, 1] + m[1, 0]) / (4 * x), (m[0, 2] + m[2, 0]) / (4 * x))
    return tuple(1.0003 * v for v in q)


def scene_camera(pose, which_image):
    rows, cols = IMAGE_SIZES[which_image]
    f = 0.36 * cols
    yaw, pitch, roll, t = pose
    return Camera(_quat_looking(yaw, pitch, roll), t, f, 1.02 * f, cols / 2.0 + 3.25, rows / 2.0 - 2.5, 0.005)


# (yaw, pitch down, roll, position)
POSES = (
    (0.0, 0.45, 0.0, (-13.0, 0.5, 4.0)),               # overview from behind the scene
    (0.1, 0.35, 0.02, (-2.0, 0.0, 0.3)),               # inside the scene, close to the ground: first observations from near
    (0.0, 0.45, 0.0, (-13.0, 0.5, 4.0)),               # the overview again: farther than 1.2 x the near observation for many points
    (0.25, 0.5, -0.03, (2.5, -2.0, -0.6)),             # close to the wall and pitched down: its upper part leaves through the top of the image
    (-0.5, 0.2, 0.0, (0.5, 4.0, 0.0)),                 # among the points: many behind the camera
    (0.1, 0.35, 0.02, (-2.0, 0.0, 0.3)),
)
# (pose, image, observation time, which visited lists make the call's list)
RENDERS = (
    (0, 0, 10.0, (0, 1, 2)),                            # the temp list accumulated over three sweeps: voxels named up to three times
    (1, 1, 10.1, (0, 1, 2)),
    (2, 0, 10.1, (2,)),                                 # the same time as the render before: a zero time step
    (3, 1, 10.35, (1, 2)),
    (4, 0, 10.3, (0,)),                                 # an EARLIER time: a negative step
    (5, 1, 10.6, (0, 2, 0)),
)


@functools.lru_cache(maxsize=None)
def scene_map():
    """the map of the scene and the visited list of each of its three insertions"""
    chk = cc.ColorChecker(*OPT)
    visited = [chk.insert(cc.scene_batch(j), BATCH_TIMES[j], 0.0)[2] for j in range(3)]
    return chk, visited


def render_call(k, visited):
    pose, which, obs_time, lists = RENDERS[k]
    return scene_camera(POSES[pose], which), which, obs_time, np.concatenate([visited[j] for j in lists])


@functools.lru_cache(maxsize=None)
def scene_sequence():
    """the whole sequence through the checker: (RenderChecker, totals per render, map_state per render, registered_state per render)"""
    chk, visited = scene_map()
    rc = RenderChecker(chk)
    totals, map_states, reg_states = [], [], []
    for k in range(len(RENDERS)):
        cam, which, obs_time, voxels = render_call(k, visited)
        totals.append(rc.render(cam, scene_image(which), voxels, obs_time))
        map_states.append(rc.map_state())
        reg_states.append(rc.registered_state())
    return rc, totals, map_states, reg_states


# ------------------------------------------------------------------------------------------------ the golden file's layout
def golden_pack(totals, map_states):
    """arrays of tests/golden/golden_color_render.npz: per render the totals and the state in map order (voxel after voxel, slot order).
    observe_distance is recorded as the entries that changed since the render before (it only moves at a first observation or a new
    minimum; whole, it alone would not fit the size limit of a committed file)."""
    out = {"option_set": np.array(OPT), "num_renders": np.array(len(totals))}
    prev = np.zeros(len(map_states[0][3]))
    for k, (tot, (rgb, n_rgb, cov, dist, time)) in enumerate(zip(totals, map_states)):
        out[f"r{k}_totals"] = np.array([tot[name] for name in TOTALS], dtype=np.int64)
        # the scene's colours are bytes, its counts small, and the three channels of cov_rgb always move together
        assert rgb.min() >= 0 and rgb.max() <= 255 and n_rgb.min() >= 0 and n_rgb.max() <= 255
        bits = np.ascontiguousarray(cov).view(np.uint32)
        assert (bits == bits[:, :1]).all()
        out[f"r{k}_rgb"] = rgb.astype(np.uint8)
        out[f"r{k}_n_rgb"] = n_rgb.astype(np.uint8)
        out[f"r{k}_cov_bits"] = np.ascontiguousarray(bits[:, 0])
        out[f"r{k}_time"] = time
        changed = np.flatnonzero(dist.view(np.uint64) != prev.view(np.uint64))
        out[f"r{k}_dist_index"] = changed.astype(np.int32)
        out[f"r{k}_dist_value"] = dist[changed]
        prev = dist
    return out


def golden_unpack(g):
    """(totals as tuples, map states) from the arrays of golden_pack"""
    totals, states = [], []
    dist = None
    for k in range(int(g["num_renders"])):
        totals.append(tuple(int(v) for v in g[f"r{k}_totals"]))
        dist = np.zeros(len(g[f"r{k}_n_rgb"])) if dist is None else dist.copy()
        dist[g[f"r{k}_dist_index"]] = g[f"r{k}_dist_value"]
        cov = np.repeat(g[f"r{k}_cov_bits"][:, None], 3, 1).view(np.float32)
        states.append((g[f"r{k}_rgb"].astype(np.int16), g[f"r{k}_n_rgb"].astype(np.int16), np.ascontiguousarray(cov), dist, g[f"r{k}_time"]))
    return totals, states
