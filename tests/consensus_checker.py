"""An independent NumPy restatement of what srl_consensus_fundamental / srl_consensus_pnp (include/srlivo_hip.h) promise -- not a port of
the kernels: the two error functions in the header's operation order (float64, so the device's masks can be recomputed bit for bit from
the returned model), a 7-point solver by SVD null space and np.roots, a linear six-point pose and a Gauss-Newton pose refinement that
share nothing with the device's P3P, a plain sequential RANSAC on NumPy's own generator (used only to validate scenes), the contract's
counter-based sampler restated from the header's text in Python integers (what every hypothesis must have drawn), and the scene
generators of the tests: camera fx = fy = 400, cx, cy = 320, 240, image 640 x 480; points x in [-4, 4], y in [-3, 3], depth 4 ... 12 m;
the second view rotated by 0.04 rad and moved by (0.3, 0.05, 0.1); every coordinate rounded to float32."""
import numpy as np

K = np.array([400.0, 400.0, 320.0, 240.0])
ROWS, COLS = 480, 640
ANGLE = 0.04
T_VIEW = np.array([0.3, 0.05, 0.1])


# ------------------------------------------------------------------------------------------------ the two error functions
def error_fundamental(F, x1, x2):
    """the larger of the two squared point-to-epipolar-line distances, in the header's order; NaN where either is NaN"""
    F = np.asarray(F, dtype=np.float64).reshape(-1)[:9]
    x1 = np.asarray(x1).astype(np.float64).reshape(-1, 2)
    x2 = np.asarray(x2).astype(np.float64).reshape(-1, 2)
    X1, Y1, X2, Y2 = x1[:, 0], x1[:, 1], x2[:, 0], x2[:, 1]
    with np.errstate(all="ignore"):
        a = (F[0] * X1 + F[1] * Y1) + F[2]
        b = (F[3] * X1 + F[4] * Y1) + F[5]
        c = (F[6] * X1 + F[7] * Y1) + F[8]
        d2 = (a * X2 + b * Y2) + c
        e2 = (d2 * d2) / (a * a + b * b)
        at = (F[0] * X2 + F[3] * Y2) + F[6]
        bt = (F[1] * X2 + F[4] * Y2) + F[7]
        ct = (F[2] * X2 + F[5] * Y2) + F[8]
        d1 = (at * X1 + bt * Y1) + ct
        e1 = (d1 * d1) / (at * at + bt * bt)
        return np.where(np.isnan(e1) | np.isnan(e2), np.nan, np.maximum(e1, e2))


def error_pnp(R, t, Kc, X, uv):
    """(squared reprojection error, camera-frame depth) in the header's order"""
    R = np.asarray(R, dtype=np.float64).reshape(-1)[:9]
    t = np.asarray(t, dtype=np.float64).reshape(3)
    Kc = np.asarray(Kc, dtype=np.float64).reshape(4)
    X = np.asarray(X).astype(np.float64).reshape(-1, 3)
    uv = np.asarray(uv).astype(np.float64).reshape(-1, 2)
    with np.errstate(all="ignore"):
        xc = ((R[0] * X[:, 0] + R[1] * X[:, 1]) + R[2] * X[:, 2]) + t[0]
        yc = ((R[3] * X[:, 0] + R[4] * X[:, 1]) + R[5] * X[:, 2]) + t[1]
        zc = ((R[6] * X[:, 0] + R[7] * X[:, 1]) + R[8] * X[:, 2]) + t[2]
        du = (Kc[0] * (xc / zc) + Kc[2]) - uv[:, 0]
        dv = (Kc[1] * (yc / zc) + Kc[3]) - uv[:, 1]
        return du * du + dv * dv, zc


def mask_fundamental(F, x1, x2, threshold):
    with np.errstate(invalid="ignore"):
        return (error_fundamental(F, x1, x2) <= threshold * threshold).astype(np.uint8)


def mask_pnp(model, Kc, X, uv, threshold):
    e, z = error_pnp(model[:9], model[9:12], Kc, X, uv)
    with np.errstate(invalid="ignore"):
        return ((z > 0) & (e <= threshold * threshold)).astype(np.uint8)


def p3p_residual(R, t, Kc, X, uv):
    """the largest squared reprojection error a pose leaves on (sample) points; inf behind the camera"""
    e, z = error_pnp(R, t, Kc, X, uv)
    return float(np.max(np.where(z > 0, e, np.inf)))


# ------------------------------------------------------------------------------------------------ minimal and reference solvers
def _hartley(x):
    m = x.mean(axis=0)
    s = np.sqrt(2.0) / np.mean(np.linalg.norm(x - m, axis=1))
    return np.array([[s, 0, -s * m[0]], [0, s, -s * m[1]], [0, 0, 1.0]])


def seven_point(x1, x2):
    """the up to three unit-norm fundamental matrices (3 x 3) through seven correspondences: SVD null space, np.roots"""
    return seven_point_with_roots(x1, x2)[0]


def close_roots(roots, rel=1e-6):
    """whether two of the (complex) roots lie within rel of each other, relative to the larger magnitude (1 at least): a cubic so close
    to a double root has a number of REAL roots that rounding decides"""
    r = np.asarray(roots, dtype=np.complex128)
    return any(abs(r[i] - r[j]) <= rel * max(1.0, abs(r[i]), abs(r[j])) for i in range(len(r)) for j in range(i + 1, len(r)))


def seven_point_with_roots(x1, x2):
    """(the matrices of seven_point, all three complex roots of its cubic)"""
    x1 = np.asarray(x1).astype(np.float64).reshape(7, 2)
    x2 = np.asarray(x2).astype(np.float64).reshape(7, 2)
    T1, T2 = _hartley(x1), _hartley(x2)
    a = (T1 @ np.c_[x1, np.ones(7)].T).T
    b = (T2 @ np.c_[x2, np.ones(7)].T).T
    A = np.stack([b[:, 0] * a[:, 0], b[:, 0] * a[:, 1], b[:, 0], b[:, 1] * a[:, 0], b[:, 1] * a[:, 1], b[:, 1], a[:, 0], a[:, 1], np.ones(7)], 1)
    _, _, vt = np.linalg.svd(A)
    F1, F2 = vt[7].reshape(3, 3), vt[8].reshape(3, 3)
    # det(l F1 + (1 - l) F2) is a cubic in l: through four values
    ls = np.array([-1.0, 0.0, 1.0, 2.0])
    coef = np.polyfit(ls, [np.linalg.det(l * F1 + (1 - l) * F2) for l in ls], 3)
    out = []
    roots = np.roots(coef)
    for r in roots:
        if abs(r.imag) > 1e-9 * max(1.0, abs(r.real)):
            continue
        F = T2.T @ (r.real * F1 + (1 - r.real) * F2) @ T1
        out.append(F / np.linalg.norm(F))
    return out, roots


def _project(R, t, Kc, X):
    Y = X @ R.T + t
    return np.stack([Kc[0] * Y[:, 0] / Y[:, 2] + Kc[2], Kc[1] * Y[:, 1] / Y[:, 2] + Kc[3]], 1), Y[:, 2]


def six_point_pose(Kc, X, uv):
    """a pose from six or more points by the direct linear transform on normalised image points (None if it fails)"""
    X = np.asarray(X, dtype=np.float64)
    uv = np.asarray(uv, dtype=np.float64)
    xn = np.stack([(uv[:, 0] - Kc[2]) / Kc[0], (uv[:, 1] - Kc[3]) / Kc[1]], 1)
    c = X.mean(axis=0)
    s = 1.0 / np.mean(np.linalg.norm(X - c, axis=1))
    Xh = np.c_[(X - c) * s, np.ones(len(X))]
    rows = []
    for p, q in zip(Xh, xn):
        rows.append(np.r_[p, np.zeros(4), -q[0] * p])
        rows.append(np.r_[np.zeros(4), p, -q[1] * p])
    _, _, vt = np.linalg.svd(np.array(rows))
    P = vt[-1].reshape(3, 4)
    if np.linalg.det(P[:, :3]) < 0:
        P = -P
    U, S, Vt = np.linalg.svd(P[:, :3])
    if S.min() < 1e-12:
        return None
    R = U @ Vt
    tt = P[:, 3] / S.mean()
    # undo the normalisation Xn = s (X - c): x ~ R s (X - c) + tt ~ R X + (tt / s - R c)
    return R, tt / s - R @ c


def refine_pose(R, t, Kc, X, uv, iterations=10):
    """Gauss-Newton on the reprojection error from (R, t): the least-squares pose of the points, P3P-free"""
    X = np.asarray(X, dtype=np.float64)
    uv = np.asarray(uv, dtype=np.float64)
    R = np.array(R, dtype=np.float64).reshape(3, 3)
    t = np.array(t, dtype=np.float64).reshape(3)
    for _ in range(iterations):
        Y = X @ R.T + t
        r = np.stack([Kc[0] * Y[:, 0] / Y[:, 2] + Kc[2] - uv[:, 0], Kc[1] * Y[:, 1] / Y[:, 2] + Kc[3] - uv[:, 1]], 1).reshape(-1)
        J = np.zeros((2 * len(X), 6))
        for i, y in enumerate(Y):
            dp = np.array([[Kc[0] / y[2], 0, -Kc[0] * y[0] / y[2] ** 2], [0, Kc[1] / y[2], -Kc[1] * y[1] / y[2] ** 2]])
            skew = np.array([[0, -y[2], y[1]], [y[2], 0, -y[0]], [-y[1], y[0], 0]])
            J[2 * i:2 * i + 2, :3] = dp @ (-skew)          # d (exp(w) Y) / d w = -[Y]x
            J[2 * i:2 * i + 2, 3:] = dp
        d = np.linalg.lstsq(J, -r, rcond=None)[0]
        w = d[:3]
        th = np.linalg.norm(w)
        Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        dR = np.eye(3) + Wx + 0.5 * Wx @ Wx if th < 1e-8 else np.eye(3) + np.sin(th) / th * Wx + (1 - np.cos(th)) / th ** 2 * Wx @ Wx
        R = dR @ R
        t = dR @ t + d[3:]
        if np.linalg.norm(d) < 1e-14:
            break
    return R, t


# ------------------------------------------------------------------------------------------------ a plain sequential RANSAC
def ransac_fundamental(x1, x2, threshold=1.0, hypotheses=512, seed=0):
    rng = np.random.default_rng(seed)
    n = len(x1)
    best, best_mask = -1, np.zeros(n, np.uint8)
    for _ in range(hypotheses):
        s = rng.choice(n, 7, replace=False)
        for F in seven_point(x1[s], x2[s]):
            m = mask_fundamental(F, x1, x2, threshold)
            if m.sum() > best:
                best, best_mask = int(m.sum()), m
    return best_mask


def ransac_pnp(X, uv, Kc=K, threshold=1.5, hypotheses=400, seed=0):
    rng = np.random.default_rng(seed)
    n = len(X)
    best, best_mask = -1, np.zeros(n, np.uint8)
    for _ in range(hypotheses):
        s = rng.choice(n, 6, replace=False)
        pose = six_point_pose(Kc, X[s], uv[s])
        if pose is None:
            continue
        m = mask_pnp(np.r_[pose[0].reshape(-1), pose[1]], Kc, X, uv, threshold)
        if m.sum() > best:
            best, best_mask = int(m.sum()), m
    return best_mask


# ------------------------------------------------------------------------------------------------ scenes
def _rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    Wx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Wx + (1 - np.cos(angle)) * Wx @ Wx


R_VIEW = _rotation([0.2, 1.0, 0.1], ANGLE)


def true_fundamental():
    """F with x2^T F x1 = 0 for the two views (first camera at the origin)"""
    Kin = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]])
    tx = np.array([[0, -T_VIEW[2], T_VIEW[1]], [T_VIEW[2], 0, -T_VIEW[0]], [-T_VIEW[1], T_VIEW[0], 0]])
    F = np.linalg.inv(Kin).T @ tx @ R_VIEW @ np.linalg.inv(Kin)
    return F / np.linalg.norm(F)


def _points(rng, n, planar):
    """n points (float32) seen inside the image by both views"""
    out = []
    while len(out) < n:
        p = np.array([rng.uniform(-4, 4), rng.uniform(-3, 3), rng.uniform(4, 12)])
        if planar:
            p[2] = 8.0 + 0.2 * p[0] - 0.1 * p[1]
        p = p.astype(np.float32).astype(np.float64)
        ok = True
        for R, t in ((np.eye(3), np.zeros(3)), (R_VIEW, T_VIEW)):
            uv, z = _project(R, t, K, p[None])
            ok = ok and z[0] > 0 and 2 <= uv[0, 0] <= COLS - 3 and 2 <= uv[0, 1] <= ROWS - 3
        if ok:
            out.append(p)
    return np.array(out)


def scene_fundamental(seed, n, n_outliers, noise=0.0, planar=False):
    """(last_xy, cur_xy) float32 and the truth mask.  An outlier's current point is moved by 8 ... 40 px PERPENDICULAR to its true epipolar
    line (either side) and by up to 30 px along it: moved along the line alone it would still be a true inlier of F."""
    rng = np.random.default_rng(seed)
    X = _points(rng, n, planar)
    x1, _ = _project(np.eye(3), np.zeros(3), K, X)
    x2, _ = _project(R_VIEW, T_VIEW, K, X)
    if noise:
        x1 = x1 + rng.uniform(-noise, noise, x1.shape)
        x2 = x2 + rng.uniform(-noise, noise, x2.shape)
    truth = np.ones(n, np.uint8)
    out = rng.choice(n, n_outliers, replace=False)
    F = true_fundamental()
    for i in out:
        line = F @ np.r_[x1[i], 1.0]
        nrm = line[:2] / np.linalg.norm(line[:2])
        tan = np.array([-nrm[1], nrm[0]])
        x2[i] = x2[i] + rng.choice([-1.0, 1.0]) * rng.uniform(8, 40) * nrm + rng.uniform(-30, 30) * tan
        truth[i] = 0
    return x1.astype(np.float32), x2.astype(np.float32), truth


def scene_pnp(seed, n, n_outliers, noise=0.0, planar=False):
    """(xyz, uv) float32 and the truth mask for the second view's pose.  An outlier's pixel is moved by 8 ... 40 px in any direction."""
    rng = np.random.default_rng(seed)
    X = _points(rng, n, planar)
    uv, _ = _project(R_VIEW, T_VIEW, K, X)
    if noise:
        uv = uv + rng.uniform(-noise, noise, uv.shape)
    truth = np.ones(n, np.uint8)
    for i in rng.choice(n, n_outliers, replace=False):
        a = rng.uniform(0, 2 * np.pi)
        uv[i] = uv[i] + rng.uniform(8, 40) * np.array([np.cos(a), np.sin(a)])
        truth[i] = 0
    return X.astype(np.float32), uv.astype(np.float32), truth


def scene_all_outliers(seed, n):
    """unrelated points everywhere: (last_xy, cur_xy, xyz, uv) float32"""
    rng = np.random.default_rng(seed)
    px = lambda: np.stack([rng.uniform(2, COLS - 3, n), rng.uniform(2, ROWS - 3, n)], 1).astype(np.float32)      # noqa: E731
    X = np.stack([rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(4, 12, n)], 1).astype(np.float32)
    return px(), px(), X, px()


# ------------------------------------------------------------------------------------------------ the contract's sampler
# Written from the text of include/srlivo_hip.h in Python integers (unbounded, hence the masks): not a port of the library's code.
_M64 = (1 << 64) - 1
MAX_DRAWS = 64


def draw(seed, h, k, m):
    """draw(seed, h, k, m) of the header: a position in [0, m)"""
    z = ((((seed & 0xFFFFFFFF) << 32) | (h & 0xFFFFFFFF)) * 0x9E3779B97F4A7C15 + (k + 1) * 0xBF58476D1CE4E5B9) & _M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & _M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return ((z >> 32) * m) >> 32


def sample(seed, h, m, S):
    """the S distinct positions in [0, m) of hypothesis h in the order drawn, or None: draws k = 0, 1, ..., a repeated position is rejected,
    no sample after 64 draws (or with m < S)"""
    if m < S:
        return None
    got = []
    for k in range(MAX_DRAWS):
        c = draw(seed, h, k, m)
        if c not in got:
            got.append(c)
            if len(got) == S:
                return got
    return None


def sample_indices(seed, h, usable, S):
    """the row of eight the contract reports for hypothesis h: the sample positions mapped through the usable list, padded with -1"""
    row = np.full(8, -1, np.int32)
    pos = sample(seed, h, len(usable), S)
    if pos is not None:
        row[:S] = np.asarray(usable)[pos]
    return row


def usable_points(*arrays):
    """ascending indices of the points whose coordinates are all finite"""
    ok = np.ones(len(arrays[0]), bool)
    for a in arrays:
        ok &= np.isfinite(np.asarray(a, dtype=np.float64).reshape(len(a), -1)).all(axis=1)
    return np.flatnonzero(ok).astype(np.int32)


def hartley_values(x1, x2, usable):
    """mx1, my1, s1, mx2, my2, s2 of the header: centroid and sqrt 2 / mean distance of the usable points of each view, float64"""
    out = []
    for x in (x1, x2):
        p = np.asarray(x).astype(np.float64)[usable]
        m = p.mean(axis=0)
        out += [m[0], m[1], np.sqrt(2.0) / np.mean(np.sqrt(((p - m) ** 2).sum(axis=1)))]
    return np.array(out)


def confidence_reached(inliers, n, S, H, confidence):
    """1 - (1 - w^S)^H >= confidence, w = inliers / n, powers by repeated multiplication in float64"""
    w = float(inliers) / float(n) if n > 0 else 0.0
    ws = 1.0
    for _ in range(S):
        ws *= w
    miss = 1.0
    for _ in range(H):
        miss *= 1.0 - ws
    return 1 if 1.0 - miss >= confidence else 0


# the scene shapes of tests/test_gpu_consensus.py: name -> (generator, arguments); truth-mask scenes first
FUNDAMENTAL_SCENES = {"f120": (11, 120, 42, 0.0), "f40": (12, 40, 10, 0.0), "f120_noise": (13, 120, 42, 0.05)}
PNP_SCENES = {"p120": (21, 120, 48, 0.0), "p12": (22, 12, 2, 0.0), "p120_noise": (23, 120, 48, 0.05)}


# ------------------------------------------------------------------------------------------------ tests/test_gpu_consensus_trace.py
# Every hypothesis of a call is held against the contract there; what the cases need of the SAMPLES (which depend on the seed, the
# hypothesis and the number of usable points alone) is checked on the CPU by tests/test_consensus_checker.py.
TRACE_H = (1, 21, 22, 85, 86, 200, 512)
TRACE_SEEDS = (0, 1, 0xFFFFFFFF)
TRACE_FUNDAMENTAL = ("f120", "f120_noise", "f_planar", "f_random", "f120_holes")
TRACE_PNP = ("p120", "p120_noise", "p_planar", "p_random", "p120_holes")
TRACE_EXACT = ("f120", "f120_holes", "p120", "p120_holes")          # noise-free and not planar: one consensus, the truth mask
# (scene, seed, H) where a LATER hypothesis sampled inside the truth inliers has all its model indices at a lower index % 256 than the first
# such hypothesis has: a pick that broke ties by thread (256 of them stride over the models) would take the later one
TRACE_TIE_CASES = (("f120", 0, 200), ("f120", 0, 512), ("p120", 0, 200), ("p120", 0, 512))


def trace_scene(name):
    """(first array, second array, truth mask or None) of a scene of the trace tests; *_holes: f120 / p120 with three true inliers made
    non-finite (and taken out of the truth mask)"""
    if name in ("f_random", "p_random"):
        a, b, X, uv = scene_all_outliers(31, 90)
        return (a, b, None) if name == "f_random" else (X, uv, None)
    if name == "f_planar":
        return scene_fundamental(14, 120, 42, 0.0, planar=True)
    if name == "p_planar":
        return scene_pnp(24, 120, 48, 0.0, planar=True)
    if name == "f120_holes":
        x1, x2, truth = scene_fundamental(*FUNDAMENTAL_SCENES["f120"])
        hurt = np.flatnonzero(truth)[[0, 17, 40]]
        x1[hurt[0], 0] = np.nan
        x2[hurt[1], 1] = np.inf
        x1[hurt[2]] = np.nan
        x2[hurt[2]] = np.nan
        truth[hurt] = 0
        return x1, x2, truth
    if name == "p120_holes":
        X, uv, truth = scene_pnp(*PNP_SCENES["p120"])
        hurt = np.flatnonzero(truth)[[1, 20, 50]]
        X[hurt[0], 2] = np.nan
        uv[hurt[1], 0] = -np.inf
        X[hurt[2]] = np.nan
        truth[hurt] = 0
        return X, uv, truth
    if name in FUNDAMENTAL_SCENES:
        return scene_fundamental(*FUNDAMENTAL_SCENES[name])
    return scene_pnp(*PNP_SCENES[name])


_TRACE_CACHE = {}


def trace_samples(name, seed, H=512):
    """(usable list, rows (H, 8) of sample indices padded with -1) the contract fixes for a scene and a seed: computed once"""
    key = ("samples", name, seed)
    if key not in _TRACE_CACHE:
        a, b, _ = trace_scene(name)
        usable = usable_points(a, b)
        S = 7 if name.startswith("f") else 3
        _TRACE_CACHE[key] = (usable, np.array([sample_indices(seed, h, usable, S) for h in range(max(TRACE_H))]))
    usable, rows = _TRACE_CACHE[key]
    return usable, rows[:H]


def trace_seven_point(name, seed, H=512):
    """per hypothesis of a fundamental scene: (the number of real solutions the checker's seven_point finds, whether its cubic has two
    roots within 1e-6 of each other -- the hypothesis is then excused from the comparison of that number)"""
    key = ("seven", name, seed)
    if key not in _TRACE_CACHE:
        a, b, _ = trace_scene(name)
        _, rows = trace_samples(name, seed)
        out = []
        for row in rows:
            if row[0] < 0:
                out.append((0, False))
                continue
            sols, roots = seven_point_with_roots(a[row[:7]], b[row[:7]])
            out.append((len(sols), close_roots(roots)))
        _TRACE_CACHE[key] = out
    return _TRACE_CACHE[key][:H]


# Sampled inside the truth inliers and still without the true matrix: the seven float32-rounded points of this one hypothesis leave a
# cubic whose two roots near 1.5535 have become a complex pair (imaginary part 0.023), so NO 7-point solver finds the scene's matrix from
# them -- the checker's own does not (tests/test_consensus_checker.py asserts that this is the whole list).
TRACE_INCOMPLETE = {("f120_holes", 1): (328,)}


def trace_complete(name, seed, H=512):
    """the hypotheses that must hold a model with the truth mask: sampled inside the truth inliers, less TRACE_INCOMPLETE"""
    return [h for h in trace_inside_truth(name, seed, H) if h not in TRACE_INCOMPLETE.get((name, seed), ())]


def trace_inside_truth(name, seed, H=512):
    """the hypotheses whose whole sample lies in the scene's truth inliers"""
    truth = trace_scene(name)[2]
    S = 7 if name.startswith("f") else 3
    _, rows = trace_samples(name, seed, H)
    return [h for h, row in enumerate(rows) if row[0] >= 0 and truth[row[:S]].all()]
