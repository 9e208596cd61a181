"""The prefilter's threshold from the bound (srl_kernels.hip: thr_from_bound).

A pass that starts from bounds takes r^2 = (sqrt(tau_prev) + |p_w - p_w_prev| + slack)^2 -- phase 0's squared cull radius, qf[5] -- as an
upper bound of the K-th smallest FP32 prefilter distance d2f.  That holds if every one of the previous pass's K neighbours has
d2f <= r^2 in this pass: the slack phase 0 puts into r (1e-3 + 1e-6 mag, the 1.000001 / 1.00001 factors) has to dominate what is rounded
on the way -- the FP32 query and the FP32 previous position (a = 2^-24 |q|_inf per axis each), the FP32 tau, and d2f's own arithmetic
(the prefilter's error model m(T) = 4 a sqrt(T) + 8 u T + 4 a^2).

This file restates phase 0's r^2 and d2_f32 operation by operation in numpy float32 (the library is built with -ffp-contract=off, so
phase 0 has no FMA; d2_f32 allows contraction, so both the plain and the fused evaluation are modelled and the larger one counts) and
checks the inequality in FP64 world coordinates up to the largest magnitude int16 voxel keys allow (32 767 voxel sizes).  No GPU."""
import numpy as np

F = np.float32
K_SLACK0, K_SLACK1, K_F1, K_F2 = F(1e-3), F(1e-6), F(1.000001), F(1.00001)


def _phase0_r2(p_w, p_prev, tau64):
    """qf[5] of assoc_tile's phase 0 for keypoints whose `inside` test holds: FP32 throughout, one rounding per operation"""
    qf = p_w.astype(F)
    bp = p_prev.astype(F)
    tau = tau64.astype(F)
    ex, ey, ez = qf[:, 0] - bp[:, 0], qf[:, 1] - bp[:, 1], qf[:, 2] - bp[:, 2]
    mag = np.maximum((np.abs(qf[:, 0]) + np.abs(qf[:, 1])) + np.abs(qf[:, 2]), (np.abs(bp[:, 0]) + np.abs(bp[:, 1])) + np.abs(bp[:, 2]))
    slack = K_SLACK0 + K_SLACK1 * mag
    rt = np.sqrt(tau) * K_F1
    r = (rt + np.sqrt((ex * ex + ey * ey) + ez * ez) * K_F1) + slack
    assert r.dtype == F
    return (r * r) * K_F2, qf


def _d2_f32(p, qf):
    """d2_f32 of the prefilter: FP32 differences, sum of squares -- plain, and with the two FMAs the contraction may form
    (a product of two FP32 values is exact in FP64: the fused operation is one rounding of that sum)"""
    dx, dy, dz = p[:, 0] - qf[:, 0], p[:, 1] - qf[:, 1], p[:, 2] - qf[:, 2]
    assert dx.dtype == F
    plain = (dx * dx + dy * dy) + dz * dz
    d = np.float64
    f1 = (dy.astype(d) * dy.astype(d) + (dx * dx).astype(d)).astype(F)
    fused = (dz.astype(d) * dz.astype(d) + f1.astype(d)).astype(F)
    return np.maximum(plain, fused)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _case(p_prev, direction, sqrt_tau, step):
    """A neighbour (an FP32 map point) at distance ~sqrt_tau from the previous position, the exact FP64 tau the previous pass stored
    for it (the reference's evaluation order), and the new position `step` away."""
    nb = (p_prev + sqrt_tau[:, None] * direction).astype(F)
    d = nb.astype(np.float64) - p_prev
    tau64 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return nb, tau64, p_prev + step


def _margin(p_prev, direction, sqrt_tau, step):
    nb, tau64, p_w = _case(p_prev, direction, sqrt_tau, step)
    r2, qf = _phase0_r2(p_w, p_prev, tau64)
    d2f = _d2_f32(nb, qf)
    return np.sqrt(r2.astype(np.float64)) - np.sqrt(d2f.astype(np.float64)), r2, d2f


def _positions(rng, n, mag):
    """positions whose largest coordinate has magnitude `mag` (an array), the others anywhere below it, any signs"""
    p = rng.uniform(-1.0, 1.0, (n, 3)) * mag[:, None]
    ax = rng.integers(0, 3, n)
    p[np.arange(n), ax] = mag * rng.choice([-1.0, 1.0], n)
    return p


def test_previous_neighbours_lie_under_the_bound_random():
    rng = np.random.default_rng(20251)
    n = 100_000
    mag = np.exp(rng.uniform(np.log(1.0), np.log(3e4), n))
    sqrt_tau = np.exp(rng.uniform(np.log(1e-3), np.log(1.7), n))
    move = rng.uniform(0.0, 2.0, n)
    move[: n // 20] = 0.0                                                  # the pose that did not move at all
    p_prev = _positions(rng, n, mag)
    m, r2, d2f = _margin(p_prev, _unit(rng, n), sqrt_tau, move[:, None] * _unit(rng, n))
    assert np.all(np.isfinite(r2)) and np.all(d2f <= r2), (int((d2f > r2).sum()), float(m.min()))
    assert m.min() > 0.0


def test_worst_corners_keep_a_strict_margin_at_the_largest_magnitude():
    """The neighbour exactly sqrt(tau) away on the far side of the movement: its distance from the new position is the whole of
    sqrt(tau) + |movement|, nothing of r but the slack is left.  All coordinates at the top of the int16 key range, where an FP32 ulp
    is 2 mm; axis-aligned and diagonal movements; distances and movements on a grid down to zero movement."""
    rng = np.random.default_rng(20252)
    top = 32767.0
    dirs = [np.array(v, np.float64) / np.linalg.norm(v) for v in
            [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, -1, 1), (1, 1, 1), (-1, 1, 1), (3, -2, 1)]]
    worst = np.inf
    for sign in (1.0, -1.0):
        for d in dirs:
            st, mv = np.meshgrid(np.geomspace(1e-3, 1.7, 40), np.concatenate([[0.0], np.geomspace(1e-4, 2.0, 39)]))
            st, mv = st.ravel(), mv.ravel()
            n = st.size
            # every coordinate within a few metres of +-32 767, jittered so that the FP32 roundings of q and q_prev fall anywhere
            p_prev = sign * (top - rng.uniform(2.0, 6.0, (n, 3)))
            for dd in (d, -d):
                m, r2, d2f = _margin(p_prev, dd[None, :].repeat(n, 0), st, -mv[:, None] * dd[None, :])
                assert np.all(d2f <= r2), (sign, dd, int((d2f > r2).sum()))
                worst = min(worst, float(m.min()))
    # what the slack has to cover there: three position roundings of sqrt(3) a each (the query's, the previous position's twice -- in
    # the stored position and in the measured movement) with a = 2^-24 * 32 767 = 1.95 mm, i.e. ~10 mm, against 1 mm + 1e-6 * mag >= 99 mm
    a = 2.0 ** -24 * top
    need = 3 * np.sqrt(3.0) * a
    slack = 1e-3 + 1e-6 * 3 * (top - 6.0)
    print(f"worst margin {worst:.4f} m; needed {need:.4f} m of a slack of {slack:.4f} m")
    assert slack > 2 * need
    assert worst > 0.0 and worst > slack - 2 * need
