"""Exact model of the sweep reconstruction -- distortFrameByConstant, distortFrameByImu (src/utility.cpp:203-306) and
transformAllImuPoint (:320-332) -- and the scenes that reach their edges: slerp with d < 0, its linear branch, absD a few ulps below the
1 - eps switch, the alpha clamps, both 1e-6 nudges of the point time, timestamps of Unix-epoch magnitude, non-unit state quaternions,
zero-length IMU intervals, both branches of so3ToQuat, every way the interval walk of distortFrameByImu stops, and the sizes around one
block of the device kernel.

The model does the TIME arithmetic in IEEE doubles exactly as the reference does (time_point, the nudges, alpha and its clamps, dt, the
interval walk, the decisions theta < 1e-4, absD >= 1 - eps and d < 0: these are what the functions mean, not rounding error) and evaluates
everything behind those decisions with mpmath at PREC bits.  It reports the branch every point took.  What the CPU oracle, and the device
kernel k_undistort, are measured against; the device tests read the recorded fixture (tests/golden/golden_undistort_edges*.npz, written by
tests/golden/make_golden_undistort.py) and never import mpmath.

Error measure, per point: e = max_c |got_c - exact_c| / (2^-52 * s) with s = |R_il raw + t_il| + |trans| for imu_point and
s = |imu_point| + |t_end| + |t_il| for the corrected raw_point -- norms, so that cancellation in one component does not inflate it.
"""
import functools
import math
import os

import numpy as np

MC_IMU, MC_CONSTANT_VELOCITY, MC_NONE = 0, 1, 2            # sr_livo_amd.capi
PREC = 256                                                  # bits of the exact model
EPS = 2.0 ** -52

# what a point went through: a branch in the low bits, flags above them
UNTOUCHED, LINEAR, SLERP, SMALL, SO3, NAN_TIME = 0, 1, 2, 3, 4, 5
BRANCH_MASK = 7
BRANCH_NAMES = {UNTOUCHED: "untouched", LINEAR: "slerp_linear", SLERP: "slerp_general", SMALL: "so3_small", SO3: "so3_general",
                NAN_TIME: "nan_time"}
D_NEG, CLAMP_HI, CLAMP_LO, NUDGE_BEGIN, NUDGE_END, DT_NEG, ZERO_GYRO, NEAR_ONE = (1 << b for b in range(4, 12))
FLAG_NAMES = {D_NEG: "d_negative", CLAMP_HI: "alpha_above_1", CLAMP_LO: "alpha_below_0", NUDGE_BEGIN: "nudge_begin", NUDGE_END: "nudge_end",
              DT_NEG: "dt_negative", ZERO_GYRO: "zero_gyro", NEAR_ONE: "absD_below_the_switch"}
BIT_EXACT = (UNTOUCHED, LINEAR, SMALL)                      # no sin / cos / acos evaluated: the device must equal the oracle bit for bit

# Worst e of the CPU oracle (oracle/srl_oracle.cpp with glibc's sin / cos / acos; bit-equal to the reference's own translation units on
# every scene) over all scenes against the exact model, as tests/test_undistort_checker.py measures and asserts it:
#   constant velocity  imu_point 2.29   raw_point 2.57
#   IMU                imu_point 1.79   raw_point 2.46
#   none                                raw_point 1.17   (transformAllImuPoint of what imu_point held)
ORACLE_WORST = 2.57
ORACLE_WORST_BY_MODE = {MC_CONSTANT_VELOCITY: 2.57, MC_IMU: 2.46, MC_NONE: 1.17}
# Bound of the device tests: 4 x the oracle's own worst error, rounded up.  The factor covers the documented bounds of the device math
# library (sin, cos, acos: a couple of ulp against glibc's < 1 ulp), which enter through a quaternion that multiplies the whole scale.
# Set from the oracle and the model, never from what the kernel returns.
K = int(math.ceil(4 * ORACLE_WORST))
# For the record only, nothing asserts against it: the device's worst e per mode (imu_point, raw_point) as
# tests/test_gpu_undistort_edges.py prints it per scene, measured on an MI355X with the ROCm device library.  The figures equal the
# oracle's: device and oracle differ in their bits at 6 of the 12 923 points only (5 of scene b_large, 1 of scene m), none of them a worst one.
DEVICE_WORST_BY_MODE = {MC_CONSTANT_VELOCITY: (2.29, 2.57), MC_IMU: (1.79, 2.46), MC_NONE: (0.0, 1.17)}

R_IL_ROTVEC = (0.02, 0.01, -0.04)
T_IL = np.array([0.05, 0.02, -0.03])
EPOCH = 1.7e9 + 0.123


# ------------------------------------------------------------------------------------------------ double-precision helpers of the scenes
def quat_from_rotvec(w):
    w = np.asarray(w, dtype=np.float64)
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.array([1.0, 0.0, 0.0, 0.0])
    return np.concatenate([[math.cos(th / 2)], w / th * math.sin(th / 2)])


def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx])


def quat_to_rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


R_IL = quat_to_rot(quat_from_rotvec(R_IL_ROTVEC))


def slerp_dot(qa, qb):
    """d of Eigen's slerp in its order of operations, as a double"""
    return float(((np.float64(qa[1]) * qb[1] + np.float64(qa[2]) * qb[2]) + np.float64(qa[3]) * qb[3]) + np.float64(qa[0]) * qb[0])


def make_track(seed, times, gyr_scale=0.3, acc_scale=0.5, gyr=None):
    """imu states (S, 17) = timestamp, un_acc, un_gyr, trans, quat wxyz, vel at `times`; the quaternion follows the gyro of the NEXT state
    over each interval, as distortFrameByImu reads it"""
    rng = np.random.default_rng(seed)
    times = np.asarray(times, dtype=np.float64)
    S = len(times)
    st = np.zeros((S, 17))
    st[:, 0] = times
    st[:, 1:4] = rng.normal(0, acc_scale, (S, 3))
    st[:, 4:7] = rng.normal(0, gyr_scale, (S, 3)) if gyr is None else np.asarray(gyr, dtype=np.float64).reshape(S, 3)
    q = quat_from_rotvec([0.1, -0.05, 0.3]); p = np.array([1.0, 2.0, 0.3]); v = np.array([1.5, -0.4, 0.1])
    for k in range(S):
        st[k, 7:10] = p; st[k, 10:14] = q; st[k, 14:17] = v
        if k + 1 < S:
            dt = times[k + 1] - times[k]
            q = quat_mul(q, quat_from_rotvec(st[k + 1, 4:7] * dt))
            q = q / np.linalg.norm(q)
            p = p + v * dt; v = v + st[k + 1, 1:4] * dt
    return st


def raw_points(seed, n):
    """sensor-frame points within +-30 m, on the float grid (a lidar delivers floats; the file compresses better)"""
    return np.random.default_rng(seed).uniform(-30, 30, (n, 3)).astype(np.float32).astype(np.float64)


def sentinel_points(n):
    """what imu_point holds before the call: non-zero, different for every point and component"""
    i = np.arange(n, dtype=np.float64)
    return np.stack([7.0 + i % 13, -3.5 - 0.25 * (i % 7), 0.125 * (i + 1)], 1)


def uniform_times(seed, n, sweep_ms):
    rel = np.sort(np.random.default_rng(seed).uniform(0.0, sweep_ms, n))
    rel[0] = 0.0; rel[-1] = sweep_ms
    return rel


def scene(name, mode, raw, rel, states, tfb, sentinel=True):
    raw = np.ascontiguousarray(raw, dtype=np.float64).reshape(-1, 3)
    rel = np.ascontiguousarray(rel, dtype=np.float64)
    assert len(raw) == len(rel)
    return dict(name=name, mode=int(mode), raw=raw, rel=rel, states=np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 17),
                tfb=float(tfb), sentinel=sentinel_points(len(raw)) if sentinel is True else sentinel)


# ------------------------------------------------------------------------------------------------ the scenes
SWEEP = 0.1                       # s
D_THETAS = (2.9e-8, 3.5e-8, 5e-8, 7e-8, 1e-7)       # quaternion angles of scene d: 1 - cos(theta) = 4.2e-16 .. 5e-15
D_SWITCH_THETA = 2.7e-8                             # absD == 1 - eps as a double: the last value of the linear branch
T_SIZES = (1, 255, 256, 257)


def _times(t0, n_states, dt=0.01):
    return t0 + dt * np.arange(n_states)


def _clamp_times(sweep_ms):
    """scene e: out of range on both sides (two different times each, for identical raw points), and both sides of both nudges"""
    return np.array([-5.0, -7.0, 1.2 * sweep_ms, 1.5 * sweep_ms, 0.0, 4e-4, -4e-4, sweep_ms + 4e-4, sweep_ms - 4e-4, sweep_ms, 1.5e-3, -1.5e-3,
                     sweep_ms + 1.5e-3, sweep_ms - 1.5e-3])


def _scene_e(name, t0):
    st = make_track(31, _times(t0, 11))
    edge = _clamp_times(1000.0 * SWEEP)
    rel = np.concatenate([edge, np.random.default_rng(32).uniform(0, 100.0, 64 - len(edge))])
    raw = raw_points(33, 64)
    raw[1] = raw[0]; raw[3] = raw[2]                 # the clamped pairs
    return scene(name, MC_CONSTANT_VELOCITY, raw, rel, st, t0)


def _boundary_scene(name, t0):
    """scene n: points at te, te +- 5e-7 s, te +- 1.5e-6 s of every interior state, and around the first state, in time order"""
    S = 6
    st = make_track(41, _times(t0, S))
    rel = [-5e-4, 0.0, 5e-4]
    rng = np.random.default_rng(42)
    for k in range(1, S):
        rel += list(np.sort(rng.uniform(10.0 * (k - 1) + 0.01, 10.0 * k - 0.01, 8)))
        if k < S - 1:
            rel += [10.0 * k + off for off in (-1.5e-3, -5e-4, 0.0, 5e-4, 1.5e-3)]
    rel = np.array(rel)
    return scene(name, MC_IMU, raw_points(43, len(rel)), rel, st, t0)


@functools.lru_cache(maxsize=None)
def scenes():
    """every scene, in the order the device tests run them on one context"""
    out = []
    cv, imu = MC_CONSTANT_VELOCITY, MC_IMU
    st11 = make_track(1, _times(200.0, 11))
    # a: an ordinary track; imu_point_in = NULL
    out.append(scene("a", cv, raw_points(2, 300), uniform_times(3, 300, 100.0), st11, 200.0, sentinel=None))
    # b: q_end = -(q_begin (x) delta): d < 0
    for tag, ang in (("b_small", 0.01), ("b_large", 1.3)):
        st = st11[[0, 5, 10]].copy()
        st[-1, 10:14] = -quat_mul(st[0, 10:14], quat_from_rotvec(ang * np.array([0.6, -0.48, 0.64])))
        out.append(scene(tag, cv, raw_points(4, 256), uniform_times(5, 256, 100.0), st, 200.0))
    # c: q_end = +-q_begin: the linear branch
    for tag, sign in (("c_same", 1.0), ("c_negated", -1.0)):
        st = st11.copy()
        st[-1, 10:14] = sign * st[0, 10:14]
        out.append(scene(tag, cv, raw_points(6, 256), uniform_times(7, 256, 100.0), st, 200.0))
    # d: absD a few ulps below 1 - eps: the general branch with theta of some 1e-8
    for j, th in enumerate(D_THETAS + (D_SWITCH_THETA,)):
        st = st11[[0, 10]].copy()
        st[-1, 10:14] = quat_mul(st[0, 10:14], np.array([math.cos(th), 0.6 * math.sin(th), -0.48 * math.sin(th), 0.64 * math.sin(th)]))
        out.append(scene("d%d" % j if j < len(D_THETAS) else "d_switch", cv, raw_points(8 + j, 64), uniform_times(20 + j, 64, 100.0), st, 200.0))
    # e: the clamps and the nudges
    out.append(_scene_e("e", 200.0))
    # f: a and e at epoch magnitude
    out.append(scene("f_a", cv, raw_points(2, 300), uniform_times(3, 300, 100.0), make_track(1, _times(EPOCH, 11)), EPOCH))
    out.append(_scene_e("f_e", EPOCH))
    # g: non-unit quaternions
    for tag, scale in (("g_long", 1.001), ("g_short", 0.999)):
        st = st11.copy()
        st[:, 10:14] *= scale
        out.append(scene(tag, cv, raw_points(50, 256), uniform_times(51, 256, 100.0), st, 200.0))
    # h: two states; one state behind the sweep's begin
    out.append(scene("h_two", cv, raw_points(52, 256), uniform_times(53, 256, 100.0), st11[[0, 10]], 200.0))
    out.append(scene("h_one", cv, raw_points(54, 256), uniform_times(55, 256, 100.0), st11[[10]], 200.0))
    # i: a trailing NaN time
    out.append(scene("i", cv, raw_points(56, 257), np.concatenate([uniform_times(57, 256, 100.0), [np.nan]]), st11, 200.0))

    # j: unequal intervals
    lengths = np.array([0.004, 0.013, 0.01, 0.007, 0.016, 0.002, 0.011, 0.0095, 0.0125, 0.015])
    tj = 200.0 + np.concatenate([[0.0], np.cumsum(lengths)])
    out.append(scene("j", imu, raw_points(60, 300), uniform_times(61, 300, 1000.0 * (tj[-1] - 200.0)), make_track(62, tj), 200.0))
    # k: |gyr| dt crosses 1e-4 inside every interval
    g = np.random.default_rng(63).normal(0, 1, (11, 3))
    g = 0.02 * g / np.linalg.norm(g, axis=1)[:, None]
    out.append(scene("k", imu, raw_points(64, 256), uniform_times(65, 256, 100.0), make_track(66, _times(200.0, 11), gyr=g), 200.0))
    # l: gyro exactly zero over two intervals
    st = make_track(67, _times(200.0, 11))
    st[3, 4:7] = 0.0; st[7, 4:7] = 0.0
    out.append(scene("l", imu, raw_points(68, 256), uniform_times(69, 256, 100.0), st, 200.0))
    # m: 35 rad/s
    g = np.random.default_rng(70).normal(0, 1, (11, 3))
    g = 35.0 * g / np.linalg.norm(g, axis=1)[:, None]
    out.append(scene("m", imu, raw_points(71, 256), uniform_times(72, 256, 100.0), make_track(73, _times(200.0, 11), gyr=g), 200.0))
    # n: points on the state timestamps
    out.append(_boundary_scene("n_200", 200.0))
    out.append(_boundary_scene("n_epoch", EPOCH))
    # o: equal timestamps: the first two states (the interval that takes the first points) and two in the middle (an interval that takes none)
    to = 200.0 + np.array([0.0, 0.0, 0.01, 0.02, 0.02, 0.03, 0.04])
    rel = np.concatenate([[-4e-4, 0.0, 4e-4], np.sort(np.random.default_rng(74).uniform(0.01, 39.9, 61))])
    out.append(scene("o", imu, raw_points(75, 64), rel, make_track(76, to), 200.0))
    # p: the first point lies before the first state: nothing is touched
    rel = uniform_times(77, 64, 100.0); rel[0] = -2e-3
    out.append(scene("p", imu, raw_points(78, 64), rel, make_track(79, _times(200.0, 11)), 200.0))
    # q: a point goes back in time: everything behind it keeps the sentinel
    rel = uniform_times(80, 256, 100.0); rel[150] = rel[5]
    out.append(scene("q", imu, raw_points(81, 256), rel, make_track(82, _times(200.0, 11)), 200.0))
    # r: one state: no interval
    out.append(scene("r", imu, raw_points(83, 64), uniform_times(84, 64, 100.0), make_track(85, _times(200.0, 1)), 200.0))
    # s: a trailing NaN time
    out.append(scene("s", imu, raw_points(86, 257), np.concatenate([uniform_times(87, 256, 100.0), [np.nan]]), make_track(88, _times(200.0, 11)), 200.0))

    # t: the sizes around one block of 256 threads, every mode
    stt = make_track(90, _times(200.0, 11))
    for n in T_SIZES:
        for mode, tag in ((cv, "cv"), (imu, "imu"), (MC_NONE, "none")):
            rel = uniform_times(91 + n, n, 100.0) if n > 1 else np.array([37.5])
            out.append(scene("t%d_%s" % (n, tag), mode, raw_points(92 + n, n), rel, stt, 200.0))
    # u: a sweep past the first allocation of 4096 points, then a small one without imu_point_in and with a stop
    out.append(scene("u_large", imu, raw_points(95, 5000), uniform_times(96, 5000, 100.0), stt, 200.0))
    rel = uniform_times(97, 300, 100.0); rel[200] = rel[3]
    out.append(scene("u_small", imu, raw_points(98, 300), rel, stt, 200.0, sentinel=None))
    assert len({s["name"] for s in out}) == len(out)
    return tuple(out)


def scene_by_name(name):
    return next(s for s in scenes() if s["name"] == name)


# ------------------------------------------------------------------------------------------------ the exact model
def _f64_walk(sc):
    """the interval every point falls into (-1: never reached) as distortFrameByImu's loop assigns it, in doubles"""
    rel, st, tfb = sc["rel"], sc["states"], np.float64(sc["tfb"])
    n, seg, it = len(rel), np.full(len(rel), -1, np.int64), 0
    for k in range(len(st) - 1):
        tb, te = np.float64(st[k, 0]), np.float64(st[k + 1, 0])
        while it != n:
            tp = tfb + np.float64(rel[it]) / np.float64(1000.0)
            if tp > tb - np.float64(1e-6) and tp < te + np.float64(1e-6):
                seg[it] = k
                it += 1
            else:
                break
    return seg, it


def _nudged(tp, tb, te):
    flags = 0
    if abs(tp - tb) < 1e-6:
        tp = tb + np.float64(1e-6); flags |= NUDGE_BEGIN
    if abs(tp - te) < 1e-6:
        tp = te - np.float64(1e-6); flags |= NUDGE_END
    return tp, flags


def exact_model(sc):
    """-> dict(branch (n,) int32, imu (n, 3) and raw (n, 3) lists of mpf (None components where the exact value is NaN), s_imu, s_raw (n,))"""
    import mpmath
    mpf = mpmath.mpf
    with mpmath.workprec(PREC), np.errstate(all="ignore"):
        raw, rel, st, mode = sc["raw"], sc["rel"], sc["states"], sc["mode"]
        n = len(raw)
        tfb = np.float64(sc["tfb"])
        Ril = [[mpf(float(v)) for v in row] for row in R_IL]
        til = [mpf(float(v)) for v in T_IL]

        def mv(M, v):
            return [M[r][0] * v[0] + M[r][1] * v[1] + M[r][2] * v[2] for r in range(3)]

        def rot(q):                                      # Eigen's toRotationMatrix: no normalisation
            w, x, y, z = q
            return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                    [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                    [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]

        def qmul(a, b):
            return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                    a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]]

        def qnormalized(q):
            z = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
            if z > 0:
                s = mpmath.sqrt(z)
                return [c / s for c in q]
            return q

        def norm3(v):
            return mpmath.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])

        def m(v):
            return [mpf(float(c)) for c in v]

        # transformAllImuPoint
        qe = m(st[-1, 10:14]); te_ = m(st[-1, 7:10])
        n2 = qe[0] * qe[0] + qe[1] * qe[1] + qe[2] * qe[2] + qe[3] * qe[3]
        Rinv = rot([qe[0] / n2, -qe[1] / n2, -qe[2] / n2, -qe[3] / n2])
        tinv = [-c for c in mv(Rinv, te_)]
        RilT = [[Ril[c][r] for c in range(3)] for r in range(3)]
        RilT_til = mv(RilT, til)
        norm_tend, norm_til = norm3(te_), norm3(til)

        def to_raw(p):
            e = mv(Rinv, p)
            o = mv(RilT, [e[0] + tinv[0], e[1] + tinv[1], e[2] + tinv[2]])
            return [o[0] - RilT_til[0], o[1] - RilT_til[1], o[2] - RilT_til[2]]

        branch = np.zeros(n, np.int32)
        imu, rawx = [None] * n, [None] * n
        s_imu, s_raw = np.zeros(n), np.zeros(n)

        if mode == MC_CONSTANT_VELOCITY:
            tfe = np.float64(st[-1, 0])
            qa64, qb64 = st[0, 10:14], st[-1, 10:14]
            d64 = slerp_dot(qa64, qb64)
            linear = abs(d64) >= 1.0 - 2.220446049250313e-16
            qa, qb, tr0, tr1 = m(qa64), m(qb64), m(st[0, 7:10]), m(st[-1, 7:10])
            scene_flags = (D_NEG if d64 < 0.0 else 0) | (NEAR_ONE if (not linear and 1.0 - abs(d64) <= 1e-14) else 0)
            if not linear:
                dE = abs(qa[1] * qb[1] + qa[2] * qb[2] + qa[3] * qb[3] + qa[0] * qb[0])
                assert dE < 1, "the double d is below 1 - eps but the exact d is not below 1"
                theta = mpmath.acos(dE)
                sin_theta = mpmath.sin(theta)
            for i in range(n):
                tp = tfb + np.float64(rel[i]) / np.float64(1000.0)
                tp, flags = _nudged(tp, tfb, tfe)
                alpha = (tp - tfb) / (tfe - tfb)
                if alpha > 1:
                    alpha = np.float64(1.0); flags |= CLAMP_HI
                if alpha < 0:
                    alpha = np.float64(0.0); flags |= CLAMP_LO
                l = mv(Ril, m(raw[i]))
                l = [l[0] + til[0], l[1] + til[1], l[2] + til[2]]
                if np.isnan(alpha):
                    branch[i] = NAN_TIME | scene_flags
                    s_imu[i] = s_raw[i] = float("nan")
                    continue
                a = mpf(float(alpha))
                if linear:
                    s0, s1 = 1 - a, a
                else:
                    s0, s1 = mpmath.sin((1 - a) * theta) / sin_theta, mpmath.sin(a * theta) / sin_theta
                if d64 < 0.0:
                    s1 = -s1
                R = rot([s0 * qa[c] + s1 * qb[c] for c in range(4)])
                tr = [(1 - a) * tr0[c] + a * tr1[c] for c in range(3)]
                p = mv(R, l)
                p = [p[0] + tr[0], p[1] + tr[1], p[2] + tr[2]]
                imu[i], rawx[i] = p, to_raw(p)
                s_imu[i] = float(norm3(l) + norm3(tr))
                s_raw[i] = float(norm3(p) + norm_tend + norm_til)
                branch[i] = (LINEAR if linear else SLERP) | scene_flags | flags
        else:
            seg = _f64_walk(sc)[0] if mode == MC_IMU else np.full(n, -1, np.int64)
            for i in range(n):
                k = int(seg[i])
                l = mv(Ril, m(raw[i]))
                l = [l[0] + til[0], l[1] + til[1], l[2] + til[2]]
                if k < 0:
                    p = m(sc["sentinel"][i]) if sc["sentinel"] is not None else [mpf(0)] * 3
                    imu[i], rawx[i] = p, to_raw(p)
                    s_imu[i] = float(norm3(l))
                    s_raw[i] = float(norm3(p) + norm_tend + norm_til)
                    branch[i] = UNTOUCHED
                    continue
                a64, b64 = st[k], st[k + 1]
                tb, te = np.float64(a64[0]), np.float64(b64[0])
                tp = tfb + np.float64(rel[i]) / np.float64(1000.0)
                tp, flags = _nudged(tp, tb, te)
                dt64 = tp - tb
                if dt64 < 0:
                    flags |= DT_NEG
                w64 = b64[4:7] * dt64
                theta64 = np.sqrt((w64[0] * w64[0] + w64[1] * w64[1]) + w64[2] * w64[2])
                if not np.any(b64[4:7]):
                    flags |= ZERO_GYRO
                dt = mpf(float(dt64))
                w = [c * dt for c in m(b64[4:7])]
                if theta64 < 0.0001:
                    dq = qnormalized([mpf(1), w[0] / 2, w[1] / 2, w[2] / 2])
                    br = SMALL
                else:
                    th = norm3(w)
                    sh = mpmath.sin(th / 2)
                    dq = qnormalized([mpmath.cos(th / 2), w[0] / th * sh, w[1] / th * sh, w[2] / th * sh])
                    br = SO3
                R = rot(qnormalized(qmul(m(a64[10:14]), dq)))
                tr0, vel, acc = m(a64[7:10]), m(a64[14:17]), m(b64[1:4])
                tr = [tr0[c] + vel[c] * dt + acc[c] * dt * dt / 2 for c in range(3)]
                p = mv(R, l)
                p = [p[0] + tr[0], p[1] + tr[1], p[2] + tr[2]]
                imu[i], rawx[i] = p, to_raw(p)
                s_imu[i] = float(norm3(l) + norm3(tr))
                s_raw[i] = float(norm3(p) + norm_tend + norm_til)
                branch[i] = br | flags

        def split(rows):
            hi, lo = np.full((n, 3), np.nan), np.zeros((n, 3))
            for i, p in enumerate(rows):
                if p is None:
                    continue
                for c in range(3):
                    h = float(p[c])
                    hi[i, c] = h
                    lo[i, c] = float(p[c] - mpf(h))
            return hi, lo

        imu_hi, imu_lo = split(imu)
        raw_hi, raw_lo = split(rawx)
    return dict(branch=branch, imu_hi=imu_hi, imu_lo=imu_lo, raw_hi=raw_hi, raw_lo=raw_lo, s_imu=s_imu, s_raw=s_raw)


# ------------------------------------------------------------------------------------------------ the error measure
def ulp_error(got, hi, lo, s):
    """e per point against the exact value hi + lo.  Where the exact value is NaN (a NaN time) e is 0 if `got` is NaN in all three components
    and inf otherwise; a NaN or inf in `got` anywhere else gives inf."""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = np.abs((got - hi) - lo)
        e = np.max(d, axis=1) / (EPS * s)
    nan_exact = np.isnan(hi).any(axis=1)
    return np.where(nan_exact, np.where(np.isnan(got).all(axis=1), 0.0, np.inf), np.where(np.isfinite(got).all(axis=1), e, np.inf))


def same_bits(a, b):
    """bit equality per point (NaN payloads and signs of zero included)"""
    a = np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).reshape(-1, 3)
    b = np.ascontiguousarray(b, dtype=np.float64).view(np.uint64).reshape(-1, 3)
    return (a == b).all(axis=1)


def census(branches):
    """how many points took every branch and carry every flag, over a list of branch arrays"""
    seen = {name: 0 for name in list(BRANCH_NAMES.values()) + list(FLAG_NAMES.values())}
    for b in branches:
        for code, name in BRANCH_NAMES.items():
            seen[name] += int(((b & BRANCH_MASK) == code).sum())
        for bit, name in FLAG_NAMES.items():
            seen[name] += int(((b & bit) != 0).sum())
    return seen


def run_oracle(sc, po, backend="plain"):
    """the CPU oracle on a scene -> imu_point, points written, raw_point"""
    imu, k = po.distort_frame(sc["raw"], sc["rel"], sc["states"], sc["tfb"], sc["mode"], R_IL, T_IL, imu_point_in=sc["sentinel"], backend=backend)
    return imu, k, po.transform_all_imu_point(imu, sc["states"], R_IL, T_IL, backend=backend)


# ------------------------------------------------------------------------------------------------ the fixture
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_STEM = "golden_undistort_edges"
PART_LIMIT = 900 * 1024            # bytes of arrays per part before compression: every file stays below the 1 MiB of a committed file
INPUT_KEYS = ("raw", "rel", "states")
MODEL_KEYS = ("branch", "imu_hi", "imu_lo", "raw_hi", "raw_lo", "s_imu", "s_raw")


def golden_paths():
    out, k = [], 1
    while True:
        p = os.path.join(GOLDEN_DIR, GOLDEN_STEM + (".npz" if k == 1 else "_part%d.npz" % k))
        if not os.path.exists(p):
            return out
        out.append(p)
        k += 1


def golden_pack():
    """the parts of the fixture, each a dict of arrays: for every scene its inputs, the branch per point and the exact outputs as hi + lo"""
    parts, cur, size = [], {}, 0
    for sc in scenes():
        ex = exact_model(sc)
        arrays = {"mode_tfb": np.array([sc["mode"], sc["tfb"]]), "has_sentinel": np.array([sc["sentinel"] is not None])}
        arrays.update({k: sc[k] for k in INPUT_KEYS})
        if sc["sentinel"] is not None:
            arrays["sentinel"] = sc["sentinel"]
        arrays.update({k: ex[k] for k in MODEL_KEYS})
        nbytes = sum(a.nbytes for a in arrays.values())
        if cur and size + nbytes > PART_LIMIT:
            parts.append(cur); cur, size = {}, 0
        cur.update({sc["name"] + "." + k: a for k, a in arrays.items()})
        size += nbytes
    parts.append(cur)
    parts[0]["R_il"] = R_IL; parts[0]["t_il"] = T_IL
    parts[0]["scenes"] = np.array([s["name"] for s in scenes()])
    return parts


def save_npz_reproducibly(path, arrays):
    """an .npz whose bytes depend on the arrays alone (np.savez stamps every member with the time of writing)"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


@functools.lru_cache(maxsize=None)
def golden_load():
    """-> (R_il, t_il, [scene dicts with the model's arrays beside the inputs]) from the committed files"""
    g = {}
    for p in golden_paths():
        g.update(np.load(p, allow_pickle=False))
    out = []
    for name in g["scenes"]:
        name = str(name)
        sc = {k: g[name + "." + k] for k in INPUT_KEYS + MODEL_KEYS}
        sc["name"] = name
        sc["mode"], sc["tfb"] = int(g[name + ".mode_tfb"][0]), float(g[name + ".mode_tfb"][1])
        sc["sentinel"] = g[name + ".sentinel"] if bool(g[name + ".has_sentinel"][0]) else None
        out.append(sc)
    return g["R_il"], g["t_il"], out
