"""k_undistort (srl_frame_undistort: distortFrameByConstant / distortFrameByImu + transformAllImuPoint) at the edges of slerp, of the
point time and of the IMU interval walk, against the exact model recorded in tests/golden/golden_undistort_edges*.npz
(tests/undistort_checker.py; no mpmath and no reference tree here).

Bit for bit against the CPU oracle wherever no sin / cos / acos is evaluated: transformAllImuPoint applied to the device's own
imu_point, slerp's linear branch, so3ToQuat's small-angle branch, untouched points, the whole of MC_NONE.  Bounded by
undistort_checker.K (4 x the oracle's own worst error against the exact model, set before the kernel was measured) per point where a
transcendental runs.  All scenes run once, in the checker's order, on ONE context: the sizes around a block, a sweep past the first
allocation and a small sweep without imu_point_in behind it are part of that order."""
import numpy as np
import pytest

import sr_livo_amd as srl
import undistort_checker as uc

pytestmark = pytest.mark.gpu

MODES = (uc.MC_CONSTANT_VELOCITY, uc.MC_IMU, uc.MC_NONE)


def same_bits_or_both_nan(a, b):
    """a NaN's sign and payload are not part of the contract (the CPU's default NaN and the device's differ in sign)"""
    a, b = np.asarray(a).reshape(-1, 3), np.asarray(b).reshape(-1, 3)
    au, bu = np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)
    return ((au == bu) | (np.isnan(a) & np.isnan(b))).all(axis=1)


@pytest.fixture(scope="module")
def runs(oracle_lib, oracle_backend):
    """every scene in its own mode (first, in order), then in the other two: {(name, mode): (scene, imu_g, raw_g, imu_o, raw_o)}"""
    R_il, t_il, scenes = uc.golden_load()
    out = {}
    ctx = srl.Context(0)
    try:
        def run(sc, mode):
            imu_g, raw_g = ctx.frame_undistort(sc["raw"], sc["rel"], sc["states"], sc["tfb"], mode, R_il, t_il, imu_point_in=sc["sentinel"])
            imu_o, _ = oracle_lib.distort_frame(sc["raw"], sc["rel"], sc["states"], sc["tfb"], mode, R_il, t_il, imu_point_in=sc["sentinel"],
                                                backend=oracle_backend)
            raw_o = oracle_lib.transform_all_imu_point(imu_o, sc["states"], R_il, t_il, backend=oracle_backend)
            stage2 = oracle_lib.transform_all_imu_point(imu_g, sc["states"], R_il, t_il, backend=oracle_backend)
            out[(sc["name"], mode)] = dict(scene=sc, imu_g=imu_g, raw_g=raw_g, imu_o=imu_o, raw_o=raw_o, stage2=stage2)
        for sc in scenes:
            run(sc, sc["mode"])
        for sc in scenes:
            for mode in MODES:
                if mode != sc["mode"]:
                    run(sc, mode)
    finally:
        ctx.close()
    return out


def own(runs):
    return [r for (name, mode), r in runs.items() if mode == r["scene"]["mode"]]


def test_the_fixture_reaches_the_branches():
    seen = uc.census([sc["branch"] for sc in uc.golden_load()[2]])
    assert all(v > 0 for v in seen.values()), seen


def test_transform_all_imu_point_is_bit_exact_in_every_scene_and_mode(runs):
    assert len(runs) == 3 * len(uc.golden_load()[2])
    for key, r in runs.items():
        bad = np.flatnonzero(~same_bits_or_both_nan(r["raw_g"], r["stage2"]))
        assert len(bad) == 0, (key, bad[:5], r["raw_g"][bad[:2]], r["stage2"][bad[:2]])


def test_branches_without_a_transcendental_equal_the_oracle_bit_for_bit(runs):
    counted = {b: 0 for b in uc.BIT_EXACT}
    for r in own(runs):
        sc = r["scene"]
        branch = sc["branch"] & uc.BRANCH_MASK
        for b in uc.BIT_EXACT:
            sel = branch == b
            counted[b] += int(sel.sum())
            bad = np.flatnonzero(sel & ~uc.same_bits(r["imu_g"], r["imu_o"]))
            assert len(bad) == 0, (sc["name"], uc.BRANCH_NAMES[b], bad[:5], r["imu_g"][bad[:2]], r["imu_o"][bad[:2]])
            bad = np.flatnonzero(sel & ~uc.same_bits(r["raw_g"], r["raw_o"]))
            assert len(bad) == 0, (sc["name"], uc.BRANCH_NAMES[b], "raw_point", bad[:5])
    assert all(v >= 256 for v in counted.values()), counted


def test_mode_none_equals_the_oracle_bit_for_bit(runs):
    for (name, mode), r in runs.items():
        if mode == uc.MC_NONE:
            sc = r["scene"]
            start = np.zeros_like(sc["raw"]) if sc["sentinel"] is None else sc["sentinel"]
            assert uc.same_bits(r["imu_g"], start).all() and uc.same_bits(r["imu_g"], r["imu_o"]).all(), name
            assert same_bits_or_both_nan(r["raw_g"], r["raw_o"]).all(), name


def test_every_point_is_within_k_of_the_exact_model(runs):
    """K = 4 x ORACLE_WORST rounded up: the oracle's own worst error against the model times the allowance for the device math library"""
    assert uc.K == int(np.ceil(4 * uc.ORACLE_WORST))
    worst, failures = {}, []
    for r in own(runs):
        sc = r["scene"]
        e_imu = uc.ulp_error(r["imu_g"], sc["imu_hi"], sc["imu_lo"], sc["s_imu"])
        e_raw = uc.ulp_error(r["raw_g"], sc["raw_hi"], sc["raw_lo"], sc["s_raw"])
        o_imu = uc.ulp_error(r["imu_o"], sc["imu_hi"], sc["imu_lo"], sc["s_imu"])
        o_raw = uc.ulp_error(r["raw_o"], sc["raw_hi"], sc["raw_lo"], sc["s_raw"])
        differ = int((~same_bits_or_both_nan(r["imu_g"], r["imu_o"])).sum()), int((~same_bits_or_both_nan(r["raw_g"], r["raw_o"])).sum())
        print("undistort e  %-10s mode %d  n %4d   device imu_point %6.2f raw_point %6.2f   oracle imu_point %5.2f raw_point %5.2f   "
              "points whose bits differ from the oracle's: imu_point %d raw_point %d"
              % (sc["name"], sc["mode"], len(e_imu), e_imu.max(), e_raw.max(), o_imu.max(), o_raw.max(), differ[0], differ[1]))
        w = worst.setdefault(sc["mode"], [0.0, 0.0])
        w[0], w[1] = max(w[0], float(e_imu.max())), max(w[1], float(e_raw.max()))
        if not (e_imu.max() <= uc.K and e_raw.max() <= uc.K):
            failures.append((sc["name"], float(e_imu.max()), int(e_imu.argmax()), float(e_raw.max()), int(e_raw.argmax())))
    print("undistort e  worst per mode {mode: [imu_point, raw_point]}:", worst, " K =", uc.K, " ORACLE_WORST =", uc.ORACLE_WORST)
    assert not failures, failures


def test_untouched_points_keep_what_imu_point_held(runs):
    checked = 0
    for r in own(runs):
        sc = r["scene"]
        untouched = (sc["branch"] & uc.BRANCH_MASK) == uc.UNTOUCHED
        if not untouched.any():
            continue
        start = np.zeros_like(sc["raw"]) if sc["sentinel"] is None else sc["sentinel"]
        assert uc.same_bits(r["imu_g"][untouched], start[untouched]).all(), sc["name"]
        checked += 1
    assert checked >= 8
    for name, count in (("p", 64), ("r", 64), ("q", 106), ("s", 1)):              # before the first state, one state, a stop, a NaN time
        sc = runs[(name, uc.MC_IMU)]["scene"]
        assert int(((sc["branch"] & uc.BRANCH_MASK) == uc.UNTOUCHED).sum()) == count, name
    # after the 5000-point sweep with non-zero sentinels, the 300-point sweep without imu_point_in: zeros behind its stop, not stale values
    large, small = runs[("u_large", uc.MC_IMU)], runs[("u_small", uc.MC_IMU)]
    assert large["scene"]["sentinel"] is not None and len(large["imu_g"]) == 5000 and np.all(large["scene"]["sentinel"] != 0.0)
    assert small["scene"]["sentinel"] is None
    assert not small["imu_g"][200:].any() and small["imu_g"][:200].all()
    assert not np.signbit(small["imu_g"][200:]).any()


def test_clamped_times_give_identical_points(runs):
    for name in ("e", "f_e"):
        r = runs[(name, uc.MC_CONSTANT_VELOCITY)]
        sc = r["scene"]
        for i, j, flag in ((0, 1, uc.CLAMP_LO), (2, 3, uc.CLAMP_HI)):
            assert sc["branch"][i] & flag and sc["branch"][j] & flag and sc["rel"][i] != sc["rel"][j] and np.array_equal(sc["raw"][i], sc["raw"][j])
            assert uc.same_bits(r["imu_g"][i], r["imu_g"][j]).all() and uc.same_bits(r["raw_g"][i], r["raw_g"][j]).all(), (name, i, j)


def test_nan_and_inf_only_where_the_oracle_has_them(runs):
    nans = 0
    for key, r in runs.items():
        for got, want in ((r["imu_g"], r["imu_o"]), (r["raw_g"], r["raw_o"])):
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want)), key
            nans += int(np.isnan(got).sum())
    assert nans == 12                                                        # scenes i and s under constant velocity: one point each, imu_point and raw_point
