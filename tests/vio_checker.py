"""Sequential restatement of the per-point loops of imageProcessing::vioEsikf (src/imageProcessing.cpp:308-349) and
imageProcessing::vioPhotometric (:463-518) with cloudFrame::getRgb(u, v, 0, &dx, &dy) (src/lioOptimization.cpp:99-140), on top of
tests/render_checker.py's map, camera and sub-pixel colour and tests/select_checker.py's pool positions.  One point after the other in
the list's order, Python floats (IEEE doubles) with explicit np.float32 steps where the reference holds floats, sums of three as
(a0 + a1) + a2, matrix products coefficient-wise with their zeros multiplied and added.  What the device pass (srl_color_map_vio_rows)
and the recorded golden file are compared with: per point 24 doubles and an outcome, and the sums H^T H, H^T r and acc_residual added
up in list order.

The contract's departures from the reference's loops (include/srlivo_hip.h): the list's order instead of a std::map keyed by pointer
value; a pool position outside the map (`unknown`), a point with z < 0.001 (`behind`) and, in photometric mode, a point whose 17 samples
would leave the image (`outside`) are left out and counted where the reference divides or reads unguarded.

Also the scenes of the tests: render_checker's map after its render sequence, seen by the cameras of its first two renders (480 x 640 and
375 x 500), the tracked lists taken from select_checker's selections at minimum_dis 40 with seeded matches and float-valued velocities.
"""
import functools
import math
import zlib

import numpy as np

import render_checker as rk
import select_checker as sk

F32 = np.float32
REPROJECTION, PHOTOMETRIC = 0, 1
USED, FEW_VIEWS, BEHIND, OUTSIDE, UNKNOWN = 0, 1, 2, 3, 4
COUNTS = ("used", "few_views", "behind", "outside", "unknown")
POINT_DTYPE = np.dtype([("pool", "<i4"), ("pad", "<i4"), ("match_u", "<f8"), ("match_v", "<f8"), ("vel_u", "<f8"), ("vel_v", "<f8")])
PAIRS = tuple((a, b) for a in range(11) for b in range(a, 11))             # the upper triangle, row after row
N_SUMS = len(PAIRS) + 11 + 1                                               # + H^T r + acc_residual


def huber(residual):
    """getHuberLoss(residual, 1.0) (imageProcessing.cpp:202-216): residual / 1.0 and sqrt(1.0) change no bit"""
    if residual < 1.0:
        return 1.0
    return (2 * math.sqrt(residual) - 1.0) / residual


def row_times(j, m):
    """one row of a coefficient-wise product with a 3 x 3 matrix (row-major list of 9)"""
    return [(j[0] * m[k] + j[1] * m[3 + k]) + j[2] * m[6 + k] for k in range(3)]


def footprint_inside(u, v, rows, cols):
    """the 17 samples of getRgb read columns floor(u) - 4 ... floor(u) + 5 and rows likewise"""
    if not (math.isfinite(u) and math.isfinite(v)):
        return False
    fu, fv = math.floor(u), math.floor(v)
    return fu - 4 >= 0 and fu + 5 <= cols - 1 and fv - 4 >= 0 and fv + 5 <= rows - 1


def get_rgb(img, u, v):
    """cloudFrame::getRgb(u, v, 0, &dx, &dy): (colour, dx, dy) as three lists of doubles"""
    rgb, _ = rk.sub_pixel(img, v, u)
    left, right, down, up = ([F32(0)] * 3 for _ in range(4))
    pixel_dif = F32(0)
    for bias in range(1, 5):                                               # ssd = 5
        a, b = rk.sub_pixel(img, v, u - bias)[0], rk.sub_pixel(img, v, u + bias)[0]
        left = [F32(left[k] + F32(a[k])) for k in range(3)]
        right = [F32(right[k] + F32(b[k])) for k in range(3)]
        a, b = rk.sub_pixel(img, v - bias, u)[0], rk.sub_pixel(img, v + bias, u)[0]
        down = [F32(down[k] + F32(a[k])) for k in range(3)]
        up = [F32(up[k] + F32(b[k])) for k in range(3)]
        pixel_dif = F32(pixel_dif + F32(2 * bias))
    dx = [float(F32(right[k] - left[k])) / float(pixel_dif) for k in range(3)]
    dy = [float(F32(up[k] - down[k])) / float(pixel_dif) for k in range(3)]
    return [float(c) for c in rgb], dx, dy


class Scene:
    """a map with colour state by pool position, an image, a camera state and a tracked list"""

    def __init__(self, position, n_rgb, cov, rgb, img, camera, time_td, R_imu_camera, points):
        self.position, self.n_rgb, self.cov, self.rgb = position, n_rgb, cov, rgb      # (P, 3) float32, (P,) int16, (P, 3) float32, (P, 3) int16
        self.img = img
        self.camera = camera                                               # rk.Camera
        self.time_td = float(time_td)
        self.R = [float(x) for x in np.asarray(R_imu_camera).reshape(9)]   # row-major
        self.points = points                                               # POINT_DTYPE

    @property
    def num_points(self):
        return len(self.position)


def point_rows(scene, q, mode, estimate_extrinsic, estimate_intrinsic):
    """one list entry: (outcome, 24 doubles, acc_residual term, flags of the huber branch)"""
    row = [0.0] * 24
    pool = int(q["pool"])
    if pool < 0 or pool >= scene.num_points:
        return UNKNOWN, row, 0.0, None
    if mode == PHOTOMETRIC and int(scene.n_rgb[pool]) < 3:                 # :465
        return FEW_VIEWS, row, 0.0, None
    cam = scene.camera
    p = [float(c) for c in scene.position[pool]]                           # getPosition(): position.cast<double>()
    R, t = cam.R, cam.t_cw
    x = ((R[0][0] * p[0] + R[0][1] * p[1]) + R[0][2] * p[2]) + t[0]
    y = ((R[1][0] * p[0] + R[1][1] * p[1]) + R[1][2] * p[2]) + t[1]
    z = ((R[2][0] * p[0] + R[2][1] * p[1]) + R[2][2] * p[2]) + t[2]
    if z < 0.001:
        return BEHIND, row, 0.0, None
    vel_u, vel_v = float(q["vel_u"]), float(q["vel_v"])
    u = (cam.fx * x / z + cam.cx) + scene.time_td * vel_u
    v = (cam.fy * y / z + cam.cy) + scene.time_td * vel_v
    J0 = [cam.fx / z, 0.0, -(cam.fx * x) / (z * z)]
    J1 = [0.0, cam.fy / z, -(cam.fy * y) / (z * z)]
    S = [0.0, -z, y, z, 0.0, -x, -y, x, 0.0]                                # numType::skewSymmetric(point_camera)
    Rt = [scene.R[c * 3 + r] for r in range(3) for c in range(3)]          # R_imu_camera.transpose()

    if mode == REPROJECTION:
        du, dv = u - float(q["match_u"]), v - float(q["match_v"])
        residual = math.sqrt(du * du + dv * dv)
        h = huber(residual)
        row[11], row[23] = du * h, dv * h
        row[0], row[12] = vel_u * h, vel_v * h
        if estimate_extrinsic:
            for i, J in ((0, J0), (1, J1)):
                a = row_times(J, S)
                b = row_times([-J[0], -J[1], -J[2]], Rt)
                for k in range(3):
                    row[i * 12 + 1 + k] = a[k] * h
                    row[i * 12 + 4 + k] = b[k] * h
        if estimate_intrinsic:
            row[7:11] = [x / z * h, 0.0 * h, 1.0 * h, 0.0 * h]
            row[19:23] = [0.0 * h, y / z * h, 0.0 * h, 1.0 * h]
        return USED, row, residual, residual >= 1.0

    rows_, cols_ = scene.img.shape[0], scene.img.shape[1]
    if not footprint_inside(u, v, rows_, cols_):
        return OUTSIDE, row, 0.0, None
    obs, dx, dy = get_rgb(scene.img, u, v)
    with np.errstate(divide="ignore"):
        info = [float(np.float64(1.0) / np.float64(scene.cov[pool][k])) for k in range(3)]
    res = [obs[k] - float(scene.rgb[pool][k]) for k in range(3)]
    norm = math.sqrt((res[0] * res[0] + res[1] * res[1]) + res[2] * res[2])
    h = huber(norm)
    r = [res[k] * h for k in range(3)]
    acc = ((r[0] * info[0]) * r[0] + (r[1] * info[1]) * r[1]) + (r[2] * info[2]) * r[2]
    for k in range(3):
        row[k * 8 + 6], row[k * 8 + 7] = r[k], info[k]
        if estimate_extrinsic:
            Jc = [dx[k] * J0[j] + dy[k] * J1[j] for j in range(3)]         # J_color_u * J_u_pc
            a = row_times(Jc, S)
            b = row_times([-Jc[0], -Jc[1], -Jc[2]], Rt)
            for j in range(3):
                row[k * 8 + j] = a[j] * h
                row[k * 8 + 3 + j] = b[j] * h
    return USED, row, acc, norm >= 1.0


def _point_terms(row, acc, mode):
    """the 78 terms one used point adds to the sums (numpy scalar doubles, one IEEE operation per ufunc call)"""
    r = np.asarray(row, dtype=np.float64)
    t = np.zeros(N_SUMS)
    ncol = 11 if mode == REPROJECTION else 6
    ia = np.array([a for a, b in PAIRS if b < ncol] + list(range(ncol)))
    ib = np.array([b for a, b in PAIRS if b < ncol] + [ncol] * ncol)
    at = np.array([k for k, (a, b) in enumerate(PAIRS) if b < ncol] + [len(PAIRS) + a for a in range(ncol)])
    if mode == REPROJECTION:
        t[at] = r[ia] * r[ib] + r[12 + ia] * r[12 + ib]
    else:
        t[at] = ((r[ia] * r[7]) * r[ib] + (r[8 + ia] * r[15]) * r[8 + ib]) + (r[16 + ia] * r[23]) * r[16 + ib]
    t[N_SUMS - 1] = acc
    return t


class Result:
    """rows (n, 24), outcome (n,), per point the 78 terms it adds (zeros for a point left out), the in-order sums and, per sum, the
    absolute sum of its terms (the bound of a reordered sum)"""

    def __init__(self, rows, outcome, terms, big):
        self.rows, self.outcome, self.terms, self.big = rows, outcome, terms, big
        sums = np.zeros(N_SUMS)
        for i in np.flatnonzero(outcome == USED):                          # one point after the other
            sums = sums + terms[i]
        self.sums = sums
        self.abs_sums = np.abs(terms).sum(axis=0)
        used = outcome == USED
        self.branches = (int((used & ~big).sum()), int((used & big).sum()))      # used points with residual < 1, >= 1

    @property
    def counts(self):
        return tuple(int((self.outcome == k).sum()) for k in range(5))

    def take(self, index):
        """the result of the list cut, cycled or permuted by `index`: a point's rows do not depend on its place, the sums do"""
        index = np.asarray(index, dtype=np.int64)
        return Result(self.rows[index], self.outcome[index], self.terms[index], self.big[index])

    def matrices(self, sums=None):
        """(HtH (11, 11) full and symmetric, Htr (11,), acc_residual)"""
        s = self.sums if sums is None else sums
        H = np.zeros((11, 11))
        for k, (a, b) in enumerate(PAIRS):
            H[a, b] = H[b, a] = s[k]
        return H, s[len(PAIRS):len(PAIRS) + 11].copy(), float(s[N_SUMS - 1])

    def bound(self):
        """per sum: n_used * 2^-52 * sum |terms|, what reordering a sum of n_used doubles can move it by"""
        return self.counts[USED] * 2.0 ** -52 * self.abs_sums


def vio_rows(scene, mode, estimate_extrinsic=True, estimate_intrinsic=True, points=None):
    pts = scene.points if points is None else points
    n = len(pts)
    rows = np.zeros((n, 24))
    outcome = np.zeros(n, np.uint8)
    terms = np.zeros((n, N_SUMS))
    big = np.zeros(n, bool)
    for i in range(n):
        o, row, acc, is_big = point_rows(scene, pts[i], mode, estimate_extrinsic, estimate_intrinsic)
        outcome[i] = o
        if o != USED:
            continue
        rows[i] = row
        big[i] = is_big
        terms[i] = _point_terms(row, acc, mode)
    return Result(rows, outcome, terms, big)


# ------------------------------------------------------------------------------------------------ the scenes
TIME_TD = 0.0125
SCENE_RENDERS = (0, 1)                    # the renders whose camera and image size a scene uses: 480 x 640 and 375 x 500
EXTRA_RENDERS = ()                        # further renders behind render_checker's sequence (none needed: see the preconditions' test)
EXTRAS_PER_CLASS = 4


def r_imu_camera():
    """a rotation that is no permutation: every entry of J R^T is a sum of three non-zero terms"""
    w, x, y, z = 0.5, -0.48, 0.52, -0.49
    n = math.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


@functools.lru_cache(maxsize=None)
def map_state():
    """render_checker's map after its render sequence by pool position: (position, N_rgb, cov_rgb, rgb)"""
    smap, _ = sk.scene_map()
    rc = rk.scene_sequence()[0]
    P = len(smap.pool_of)
    position = np.zeros((P, 3), np.float32); n_rgb = np.zeros(P, np.int16); cov = np.zeros((P, 3), np.float32); rgb = np.zeros((P, 3), np.int16)
    for (key, slot), pool in smap.pool_of.items():
        position[pool] = smap.chk.voxels[key].points[slot]
        st = rc.state.get((key, slot))
        if st is not None:
            n_rgb[pool] = st.n_rgb; cov[pool] = st.cov; rgb[pool] = st.rgb
    return position, n_rgb, cov, rgb


def _tracked(which, camera, rows, cols, state):
    """the selection at minimum_dis 40 of the scene's render, with seeded matches (most within a pixel of the prediction, some farther)
    and float-valued velocities (cv::Point2f); behind it a few points of every class the selection does not bring: pool positions -1 and
    num_points, points behind the camera, points with three views whose footprint leaves the image"""
    k = SCENE_RENDERS[which]
    n_seq = sk.SEQUENCE.index((k, 2, 0))
    rec = sk.sequence_results()[n_seq][0]
    rng = np.random.default_rng(9100 + which)
    n = len(rec)
    pts = np.zeros(n, POINT_DTYPE)
    pts["pool"] = rec["pool"]
    vel = rng.uniform(-20.0, 20.0, (n, 2)).astype(np.float32)
    pts["vel_u"], pts["vel_v"] = vel[:, 0], vel[:, 1]
    spread = np.where(rng.random(n) < 0.7, 0.45, 3.0)
    pts["match_u"] = rec["u"].astype(np.float64) + rng.uniform(-1, 1, n) * spread
    pts["match_v"] = rec["v"].astype(np.float64) + rng.uniform(-1, 1, n) * spread
    position, n_rgb = state[0], state[1]
    behind, behind_any, outside = [], [], []
    for pool in range(len(position)):
        if len(behind) >= EXTRAS_PER_CLASS and len(outside) >= EXTRAS_PER_CLASS:
            break
        outcome, u, v = camera.project([float(c) for c in position[pool]], rows, cols)
        if outcome == 1:
            # with three views where the map has such a point: in photometric mode the views are asked first
            if n_rgb[pool] >= 3 and len(behind) < EXTRAS_PER_CLASS:
                behind.append(pool)
            elif len(behind_any) < EXTRAS_PER_CLASS:
                behind_any.append(pool)
        elif n_rgb[pool] >= 3 and not footprint_inside(u, v, rows, cols) and len(outside) < EXTRAS_PER_CLASS:
            outside.append(pool)
    behind = behind or behind_any
    extra = np.zeros(2 + len(behind) + len(outside), POINT_DTYPE)
    extra["pool"] = [-1, len(position)] + behind + outside
    extra["match_u"], extra["match_v"] = 100.0, 100.0
    return np.concatenate([pts, extra])


@functools.lru_cache(maxsize=None)
def scene(which):
    state = map_state()
    k = SCENE_RENDERS[which]
    pose, image, _, _ = rk.RENDERS[k]
    assert image == which
    cam = rk.scene_camera(rk.POSES[pose], image)
    rows, cols = rk.IMAGE_SIZES[image]
    return Scene(*state, rk.scene_image(image), cam, TIME_TD, r_imu_camera(), _tracked(which, cam, rows, cols, state))


def cut_or_cycle(length, n):
    """the index of a list of n entries cut or cycled from a tracked list of `length`"""
    return np.arange(n) % length


def edge_list(sc):
    """a used point of the scene moved by its velocity onto the footprint's edges in u: floor(u) = 4 (inside), 3 (outside), cols - 6
    (inside), cols - 5 (outside); and likewise in v against the rows"""
    res = vio_rows(sc, PHOTOMETRIC)
    i = int(np.flatnonzero(res.outcome == USED)[0])
    q = sc.points[i]
    cam = sc.camera
    p = [float(c) for c in sc.position[int(q["pool"])]]
    _, u0, v0 = cam.project(p, 10**6, 10**6)
    rows, cols = sc.img.shape[0], sc.img.shape[1]
    out = []
    for axis, base, size in (("u", u0, cols), ("v", v0, rows)):
        for target in (4.5, 3.5, size - 6 + 0.5, size - 5 + 0.5):
            e = q.copy()
            e["vel_u"], e["vel_v"] = 0.0, 0.0
            e["vel_" + axis] = float(np.float32((target - base) / sc.time_td))
            out.append(e)
    return np.array(out, dtype=POINT_DTYPE), (USED, OUTSIDE, USED, OUTSIDE) * 2


CONFIGS = tuple((mode, ext, intr) for mode in (REPROJECTION, PHOTOMETRIC) for ext in (1, 0) for intr in (1, 0))


@functools.lru_cache(maxsize=None)
def scene_results(which):
    """the checker's Result of every entry of CONFIGS on the scene's tracked list"""
    sc = scene(which)
    return tuple(vio_rows(sc, mode, bool(ext), bool(intr)) for mode, ext, intr in CONFIGS)


# ------------------------------------------------------------------------------------------------ the updates around the loops
# the camera state imageProcessing::vioEsikf (:220-380) and vioPhotometric (:402-552) work on, the initial state and covariance of the
# tests, and the measure of a difference between two runs.  The updates themselves with the EXPLICIT gain K, as the reference forms it
# (:361, :528), are tests/vio_ref_reader.cpp's: what the host mirror's solve from the sums (csrc/host/imageProcessing.cpp) is compared with.
STATE_DOUBLES = 31


def _quat_to_R(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _quat_from_R(m):
    """Eigen::Quaterniond(Matrix3d): Shepperd's method"""
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = math.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return np.array([w, (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t])
    i = int(np.argmax([m[0, 0], m[1, 1], m[2, 2]]))
    j, k = (i + 1) % 3, (i + 2) % 3
    t = math.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
    q = np.zeros(4)
    q[1 + i] = 0.5 * t
    t = 0.5 / t
    q[0] = (m[k, j] - m[j, k]) * t
    q[1 + j] = (m[j, i] + m[i, j]) * t
    q[1 + k] = (m[k, i] + m[i, k]) * t
    return q


class CameraState:
    """the camera members of class state the two updates read and write; as 31 doubles: time_td, R_imu_camera (9), t_imu_camera (3),
    fx fy cx cy, q_world_camera (w x y z), t_world_camera (3), rotation (w x y z), translation (3)"""

    def __init__(self, vector):
        v = np.asarray(vector, dtype=np.float64)
        self.time_td = float(v[0]); self.R = v[1:10].reshape(3, 3).copy(); self.t = v[10:13].copy()
        self.fx, self.fy, self.cx, self.cy = (float(x) for x in v[13:17])
        self.q_wc = v[17:21].copy(); self.t_wc = v[21:24].copy(); self.rotation = v[24:28].copy(); self.translation = v[28:31].copy()

    def vector(self):
        return np.concatenate([[self.time_td], self.R.ravel(), self.t, [self.fx, self.fy, self.cx, self.cy], self.q_wc, self.t_wc, self.rotation,
                               self.translation])

    def camera(self):
        return rk.Camera(self.q_wc, self.t_wc, self.fx, self.fy, self.cx, self.cy)

    def follow_pose(self):                                                 # :396-397
        Rw = _quat_to_R(self.rotation)
        self.q_wc = _quat_from_R(Rw @ self.R)
        self.t_wc = Rw @ self.t + self.translation


def scene_at(base, st, tracked):
    """the scene's map and image seen from a camera state"""
    return Scene(base.position, base.n_rgb, base.cov, base.rgb, base.img, st.camera(), st.time_td, st.R, tracked)


def initial_state(which):
    """a camera state whose camera is the scene's: the IMU pose is chosen so that the chain rotation * R_imu_camera ends there"""
    sc = scene(which)
    R_ic, t_ic = r_imu_camera(), np.array([0.05, -0.02, 0.1])
    R_wc = _quat_to_R(np.array(sc.camera.q) / np.linalg.norm(sc.camera.q))
    R_wi = R_wc @ R_ic.T
    v = np.concatenate([[TIME_TD], R_ic.ravel(), t_ic, [sc.camera.fx, sc.camera.fy, sc.camera.cx, sc.camera.cy], sc.camera.q, sc.camera.t,
                        _quat_from_R(R_wi), np.array(sc.camera.t) - R_wi @ t_ic])
    return CameraState(v)


def initial_cov():
    """setInitialCov (:65-72)"""
    c = np.eye(11) * 0.0001
    c[0, 0] = 0.00001
    c[1:7, 1:7] = np.eye(6) * 1e-3
    c[7:11, 7:11] = np.eye(4) * 1e-3
    return c


NEW_VISITED_VOXELS = 800                  # number_of_new_visited_voxel: cam_measurement_weight = 5 / 800 lies between its two clamps


def difference(got_states, got_cov, want_states, want_cov):
    """the largest difference of the states (per block of the vector, relative to the block's largest magnitude) and of the covariance
    (relative to its largest magnitude)"""
    blocks = ((0, 1), (1, 10), (10, 13), (13, 17), (17, 21), (21, 24))
    worst = float(np.abs(got_cov - want_cov).max() / np.abs(want_cov).max())
    for g, w in zip(got_states, want_states):
        for lo, hi in blocks:
            worst = max(worst, float(np.abs(g[lo:hi] - w[lo:hi]).max() / np.abs(w[lo:hi]).max()))
    return worst


def fill_sums(sums, res):
    """a Result's in-order sums and counts into a srl_color_vio_sums record (a ctypes structure)"""
    H, r, acc = res.matrices()
    for k, v in enumerate(H.ravel()):
        sums.HtH[k] = v
    for k, v in enumerate(r):
        sums.Htr[k] = v
    sums.acc_residual = acc
    sums.used, sums.few_views, sums.behind, sums.outside, sums.unknown = res.counts


# ------------------------------------------------------------------------------------------------ the golden file's layout
def golden_pack():
    """arrays of tests/golden/golden_color_vio.npz: per scene the list, and per configuration the outcomes, the in-order sums and the
    number and a CRC-32 of the rows' bytes (the rows themselves would not fit the size limit of a committed file)"""
    out = {"configs": np.array(CONFIGS, dtype=np.int32), "time_td": np.array(TIME_TD), "R_imu_camera": r_imu_camera()}
    for which in range(len(SCENE_RENDERS)):
        out["s%d_points" % which] = scene(which).points
        for c, res in enumerate(scene_results(which)):
            name = "s%d_c%d" % (which, c)
            out[name + "_outcome"] = res.outcome
            out[name + "_sums"] = res.sums
            out[name + "_crc"] = np.array([len(res.rows), zlib.crc32(np.ascontiguousarray(res.rows).tobytes())], dtype=np.int64)
    return out


def golden_pack_reader(lib):
    """... and per scene the states behind every iteration, the covariances and the used counts of vioEsikf then vioPhotometric run by
    tests/vio_ref_reader.cpp (vio_reader.sequence): the reference's own pieces and the explicit K on the stand-in Eigen"""
    import vio_reader as vr
    out = {}
    for which in range(len(SCENE_RENDERS)):
        for name, (accepted, states, cov, used) in zip(("esikf", "photometric"), vr.sequence(lib, which)):
            out["s%d_%s_states" % (which, name)] = np.array(states).reshape(-1, STATE_DOUBLES)
            out["s%d_%s_cov" % (which, name)] = cov
            out["s%d_%s_used" % (which, name)] = np.array([int(accepted), used])
    return out


def golden_check(g, name, rows, outcome):
    """rows and outcomes against the golden arrays of that name: None, or what differs"""
    if not np.array_equal(g[name + "_outcome"], outcome):
        return "outcome"
    if (len(rows), zlib.crc32(np.ascontiguousarray(rows).tobytes())) != tuple(int(v) for v in g[name + "_crc"]):
        return "rows (CRC)"
    return None
