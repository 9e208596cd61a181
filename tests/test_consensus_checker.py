"""The checker of the consensus tests checked by itself (CPU): the two error functions on hand-computed cases, and every scene shape of
tests/test_gpu_consensus.py validated by the checker's own sequential RANSAC (NumPy's generator, its own minimal solvers): ten seeds
each return exactly the ground-truth mask, so "the mask equals the truth" is a property of the scene and not of one sampler.  A planar
scene does NOT have that property for the fundamental model (a plane leaves a two-parameter family of matrices, and members of it pick
up outliers), which is why the truth-mask tests leave it out."""
import numpy as np
import pytest

import consensus_checker as ck


def test_error_fundamental_known_answers():
    # a pure x-translation: x2^T F x1 = y1 - y2, every epipolar line horizontal
    F = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], dtype=np.float64)
    e = ck.error_fundamental(F, np.float32([[10, 20], [5, 7], [0, 0]]), np.float32([[50, 23], [-3, 7], [1, -0.5]]))
    assert e.tolist() == [9.0, 0.0, 0.25]
    # the two distances differ in general, the larger counts.  F = [[0, 0, 2], [0, 0, -1], [0, 1, 0]], x1 = (3, 4), x2 = (1, 2):
    # F x1 = (2, -1, 4): d2 = 2 - 2 + 4 = 4, e2 = 16 / 5; F^T x2 = (0, 1, 2 - 2) = (0, 1, 0): d1 = 4, e1 = 16 / 1
    e = ck.error_fundamental([0, 0, 2, 0, 0, -1, 0, 1, 0], np.float32([[3, 4]]), np.float32([[1, 2]]))
    assert e.tolist() == [16.0]
    # a degenerate line (0 / 0) and a NaN coordinate are NaN, hence never inliers
    e = ck.error_fundamental(np.zeros(9), np.float32([[1, 1]]), np.float32([[2, 2]]))
    assert np.isnan(e).all()
    assert ck.mask_fundamental(F, np.float32([[np.nan, 1], [1, 1]]), np.float32([[1, 1], [1, 1.5]]), 1.0).tolist() == [0, 1]


def test_error_pnp_known_answers():
    R, t = np.eye(3), np.zeros(3)
    e, z = ck.error_pnp(R, t, ck.K, np.float32([[1, 2, 4], [1, 2, -4]]), np.float32([[423, 436], [423, 436]]))
    assert e[0] == 25.0 and z.tolist() == [4.0, -4.0]            # u = 400 / 4 + 320 = 420, v = 800 / 4 + 240 = 440
    assert ck.mask_pnp(np.r_[R.reshape(-1), t], ck.K, np.float32([[1, 2, 4], [1, 2, -4], [1, 2, 4]]),
                       np.float32([[420, 441.5], [220, 40], [420, 441.6]]), 1.5).tolist() == [1, 0, 0]       # on the threshold, behind, just past it
    # a rotation by 90 degrees about z and a shift: (x, y, z) -> (-y, x, z) + (0, 0, 1)
    Rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
    e, z = ck.error_pnp(Rz, [0, 0, 1], ck.K, np.float32([[1, 2, 3]]), np.float32([[120, 340]]))
    assert e.tolist() == [0.0] and z.tolist() == [4.0]           # u = 400 (-2 / 4) + 320, v = 400 (1 / 4) + 240
    assert ck.p3p_residual(Rz, [0, 0, 1], ck.K, np.float32([[1, 2, 3]]), np.float32([[121, 340]])) == 1.0


def test_the_solvers_of_the_checker_fit_exact_data():
    x1, x2, truth = ck.scene_fundamental(5, 7, 0)
    fits = [float(np.max(ck.error_fundamental(F, x1, x2))) for F in ck.seven_point(x1, x2)]
    assert fits and max(fits) < 1e-12
    Ft = ck.true_fundamental()
    assert min(min(np.linalg.norm(F - Ft), np.linalg.norm(F + Ft)) for F in ck.seven_point(x1, x2)) < 1e-3
    X, uv, _ = ck.scene_pnp(6, 8, 0)
    R, t = ck.six_point_pose(ck.K, X[:6], uv[:6])
    assert np.abs(R - ck.R_VIEW).max() < 1e-3 and np.abs(t - ck.T_VIEW).max() < 1e-2
    R, t = ck.refine_pose(R, t, ck.K, X, uv)
    assert ck.p3p_residual(R, t, ck.K, X, uv) < 1e-8 and np.abs(R - ck.R_VIEW).max() < 1e-5


def test_the_outliers_of_the_scenes_are_outliers_of_the_truth():
    for seed, n, n_out, noise in ck.FUNDAMENTAL_SCENES.values():
        x1, x2, truth = ck.scene_fundamental(seed, n, n_out, noise)
        e = ck.error_fundamental(ck.true_fundamental(), x1, x2)
        assert truth.sum() == n - n_out and e[truth == 1].max() < 0.05 and e[truth == 0].min() > 7.8 ** 2      # (the noise moves both by <= 0.15)
    for seed, n, n_out, noise in ck.PNP_SCENES.values():
        X, uv, truth = ck.scene_pnp(seed, n, n_out, noise)
        e, z = ck.error_pnp(ck.R_VIEW, ck.T_VIEW, ck.K, X, uv)
        assert truth.sum() == n - n_out and (z > 0).all() and e[truth == 1].max() < 0.02 and e[truth == 0].min() > 7.9 ** 2


@pytest.mark.parametrize("name", sorted(ck.FUNDAMENTAL_SCENES))
def test_fundamental_scenes_have_one_consensus(name):
    seed, n, n_out, noise = ck.FUNDAMENTAL_SCENES[name]
    x1, x2, truth = ck.scene_fundamental(seed, n, n_out, noise)
    for s in range(10):
        assert np.array_equal(ck.ransac_fundamental(x1, x2, 1.0, 512, s), truth), (name, s)


@pytest.mark.parametrize("name", sorted(ck.PNP_SCENES))
def test_pnp_scenes_have_one_consensus(name):
    seed, n, n_out, noise = ck.PNP_SCENES[name]
    X, uv, truth = ck.scene_pnp(seed, n, n_out, noise)
    for s in range(10):
        assert np.array_equal(ck.ransac_pnp(X, uv, ck.K, 1.5, 400, s), truth), (name, s)


def test_a_planar_scene_has_no_single_consensus_for_the_fundamental_model():
    x1, x2, truth = ck.scene_fundamental(14, 120, 42, 0.0, planar=True)
    same = [np.array_equal(ck.ransac_fundamental(x1, x2, 1.0, 512, s), truth) for s in range(10)]
    assert not all(same), same


# ------------------------------------------------------------------------------------------------ what tests/test_gpu_consensus_trace.py relies on
def test_the_sampler_of_the_checker_draws_distinct_positions_and_fails_as_the_contract_says():
    for S in (7, 3):
        assert ck.sample(0, 0, S - 1, S) is None
        for seed in ck.TRACE_SEEDS:
            for m in (S, S + 1, 90, 117, 120, 1025):
                for h in (0, 1, 85, 511):
                    pos = ck.sample(seed, h, m, S)
                    # (with m = S a hypothesis may exhaust its 64 draws: tests/test_consensus_math.py pins some that do)
                    assert pos is None and m == S or len(set(pos)) == S and 0 <= min(pos) and max(pos) < m
    usable = np.array([2, 3, 5, 7, 11, 13, 17, 19, 23], np.int32)
    row = ck.sample_indices(1, 4, usable, 3)
    assert row.dtype == np.int32 and (row[3:] == -1).all() and row[:3].tolist() == [int(usable[p]) for p in ck.sample(1, 4, 9, 3)]
    assert (ck.sample_indices(1, 4, usable[:2], 3) == -1).all()
    assert ck.usable_points(np.float32([[1, 2], [np.nan, 1], [3, 4]]), np.float32([[1, 2], [0, 1], [np.inf, 4]])).tolist() == [0]
    # the confidence formula on values worked by hand: w = 1 / 2, S = 3: w^S = 1 / 8; H = 2: 1 - (7 / 8)^2 = 15 / 64
    assert ck.confidence_reached(60, 120, 3, 2, 15.0 / 64.0) == 1 and ck.confidence_reached(60, 120, 3, 2, 0.235) == 0
    assert ck.confidence_reached(0, 120, 7, 512, 0.5) == 0 and ck.confidence_reached(120, 120, 7, 1, 0.999) == 1


@pytest.mark.parametrize("name", ck.TRACE_FUNDAMENTAL)
def test_few_trace_hypotheses_sit_at_a_double_root(name):
    """a hypothesis whose cubic has two roots within 1e-6 is excused from the comparison of the number of solutions: at most 2 % of any
    case (scene, seed, H) may be, and every hypothesis of these scenes has a sample"""
    for seed in ck.TRACE_SEEDS:
        ref = ck.trace_seven_point(name, seed)
        _, rows = ck.trace_samples(name, seed)
        assert (rows[:, :7] >= 0).all() and (rows[:, 7] == -1).all()
        for H in ck.TRACE_H:
            excused = sum(1 for h in range(H) if ref[h][1])
            assert excused <= 0.02 * H, (name, seed, H, excused)


@pytest.mark.parametrize("name", ck.TRACE_EXACT)
def test_the_trace_cases_exercise_ties_both_confidence_values_and_completeness(name):
    a, b, truth = ck.trace_scene(name)
    is_f = name.startswith("f")
    S, slots, conf = (7, 3, 0.997) if is_f else (3, 4, 0.99)
    n, inl = len(truth), int(truth.sum())
    assert 0.35 <= 1.0 - inl / n <= 0.45
    # one hypothesis never reaches the confidence, whatever it finds (the truth inliers bound every model's count), 512 do with the truth
    assert max(ck.confidence_reached(k, n, S, 1, conf) for k in range(inl + 1)) == 0 and ck.confidence_reached(inl, n, S, 512, conf) == 1
    for seed in ck.TRACE_SEEDS:
        inside = ck.trace_inside_truth(name, seed)
        for H in (200, 512):                                          # at least two hypotheses that must tie at the maximum
            assert len(ck.trace_complete(name, seed, H)) >= 2, (name, seed, H)
        if is_f:
            # the checker's own solver finds the truth mask from every such sample -- but for the one listed
            lost = [h for h in inside if not any(np.array_equal(ck.mask_fundamental(F, a, b, 1.0), truth)
                                                 for F in ck.seven_point(a[ck.trace_samples(name, seed)[1][h, :7]], b[ck.trace_samples(name, seed)[1][h, :7]]))]
            assert tuple(lost) == ck.TRACE_INCOMPLETE.get((name, seed), ()), (name, seed, lost)
    for tname, seed, H in ck.TRACE_TIE_CASES:
        if tname != name:
            continue
        must = ck.trace_complete(name, seed, H)
        first = min((must[0] * slots + s) % 256 for s in range(slots))
        assert must[0] * slots // 256 == (must[0] * slots + slots - 1) // 256          # (its slots do not straddle a stride)
        assert any(max((h * slots + s) % 256 for s in range(slots)) < first and h * slots // 256 == (h * slots + slots - 1) // 256 for h in must[1:]), (name, seed, H)
