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
