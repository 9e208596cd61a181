"""tests/undistort_checker.py by itself, without a device: the preconditions of its scenes -- every branch and edge the device tests
rest on is reached, counted per point from the branch the exact model reports --, the recorded fixture against a fresh run of the model,
the error measure on known answers, and the CPU oracle's own worst error against the exact model (ORACLE_WORST, from which the bound of
the device tests follows).

The preconditions are conditions, not measurements: if a scene misses one, the scene is wrong, not the bar."""
import math

import numpy as np
import pytest

import undistort_checker as uc

CV, IMU, NONE = uc.MC_CONSTANT_VELOCITY, uc.MC_IMU, uc.MC_NONE


@pytest.fixture(scope="module")
def golden():
    R_il, t_il, scenes = uc.golden_load()
    return R_il, t_il, {sc["name"]: sc for sc in scenes}


def kind(sc):
    return sc["branch"] & uc.BRANCH_MASK


def has(sc, flag):
    return (sc["branch"] & flag) != 0


# ------------------------------------------------------------------------------------------------ the fixture
def test_the_fixture_is_what_the_scenes_and_the_model_give(golden):
    """every array of the committed files against a fresh run (tests/golden/make_golden_undistort.py writes exactly these)"""
    mpmath = pytest.importorskip("mpmath")
    assert mpmath.mp.prec < uc.PREC                                       # the model raises the precision itself and restores it
    R_il, t_il, g = golden
    assert np.array_equal(R_il, uc.R_IL) and np.array_equal(t_il, uc.T_IL)
    assert [s["name"] for s in uc.scenes()] == list(g)
    for sc in uc.scenes():
        rec = g[sc["name"]]
        assert (rec["mode"], rec["tfb"]) == (sc["mode"], sc["tfb"])
        assert (rec["sentinel"] is None) == (sc["sentinel"] is None)
        for k in uc.INPUT_KEYS + (("sentinel",) if sc["sentinel"] is not None else ()):
            assert rec[k].dtype == sc[k].dtype and rec[k].tobytes() == sc[k].tobytes(), (sc["name"], k)
        if len(sc["raw"]) > 512:                                           # the 5000-point sweep: every 16th point
            pick = np.arange(0, len(sc["raw"]), 16)
            if sc["mode"] == IMU:
                assert uc._f64_walk(sc)[1] == len(sc["raw"])               # no stop: a point's result does not depend on the others
            sub = dict(sc, raw=sc["raw"][pick], rel=sc["rel"][pick], sentinel=None if sc["sentinel"] is None else sc["sentinel"][pick])
            ex = uc.exact_model(sub)
            for k in uc.MODEL_KEYS:
                assert ex[k].tobytes() == rec[k][pick].tobytes(), (sc["name"], k)
            continue
        ex = uc.exact_model(sc)
        for k in uc.MODEL_KEYS:
            assert ex[k].dtype == rec[k].dtype and ex[k].tobytes() == rec[k].tobytes(), (sc["name"], k)


def test_every_file_of_the_fixture_is_small_enough():
    import os
    paths = uc.golden_paths()
    assert len(paths) >= 1 and all(os.path.getsize(p) < 1024 * 1024 for p in paths)


def test_hi_plus_lo_is_a_proper_pair(golden):
    for sc in golden[2].values():
        for hi, lo in ((sc["imu_hi"], sc["imu_lo"]), (sc["raw_hi"], sc["raw_lo"])):
            ok = np.isfinite(hi)
            assert np.all(np.abs(lo[ok]) <= 0.5 * np.spacing(np.abs(hi[ok]))) and np.all(lo[~ok] == 0.0)


# ------------------------------------------------------------------------------------------------ the error measure
def test_the_error_measure_on_known_answers():
    hi = np.array([[1.0, -2.0, 4.0], [3.0, 0.0, 0.0], [np.nan] * 3, [np.nan] * 3, [1.0, 1.0, 1.0]])
    lo = np.array([[0.0, 0.0, 2.0 ** -54], [0.0] * 3, [0.0] * 3, [0.0] * 3, [0.0] * 3])
    s = np.array([8.0, 3.0, np.nan, np.nan, 1.0])
    got = hi.copy()
    got[0, 2] = 4.0 + 2.0 ** -50                                           # one ulp of 4 above hi: (2^-50 - 2^-54) / (2^-52 * 8)
    got[1, 1] = 3 * 2.0 ** -52                                             # a cancelling component is measured against the norm
    got[3, 0] = 1.0                                                        # a number where the exact value is NaN
    got[4, 1] = np.inf
    e = uc.ulp_error(got, hi, lo, s)
    assert e[0] == (2.0 ** -50 - 2.0 ** -54) / (2.0 ** -52 * 8.0) and e[1] == 1.0 and e[2] == 0.0 and np.isinf(e[3]) and np.isinf(e[4])
    assert uc.same_bits(np.array([[0.0, 1.0, 2.0]]), np.array([[-0.0, 1.0, 2.0]])).tolist() == [False]


# ------------------------------------------------------------------------------------------------ the scenes' preconditions
def test_every_branch_and_flag_is_reached(golden):
    seen = uc.census([sc["branch"] for sc in golden[2].values()])
    for name in ("untouched", "slerp_linear", "slerp_general", "so3_small", "so3_general"):
        assert seen[name] >= 256, (name, seen)
    for name in ("d_negative", "absD_below_the_switch"):
        assert seen[name] >= 256, (name, seen)
    for name in ("alpha_above_1", "alpha_below_0", "dt_negative", "nan_time"):
        assert seen[name] >= 1, (name, seen)
    for name in ("nudge_begin", "nudge_end", "zero_gyro"):
        assert seen[name] >= 20, (name, seen)
    assert all(len(sc["raw"]) <= 512 for name, sc in golden[2].items() if name != "u_large")


def test_constant_velocity_scenes(golden):
    g = golden[2]
    one = 1.0 - 2.220446049250313e-16
    assert np.all(kind(g["a"]) == uc.SLERP) and g["a"]["sentinel"] is None and len(g["a"]["raw"]) % 256 != 0 and len(g["a"]["raw"]) > 256
    for name, angle in (("b_small", 0.01), ("b_large", 1.3)):                 # d < 0 at both rotations
        sc = g[name]
        d = uc.slerp_dot(sc["states"][0, 10:14], sc["states"][-1, 10:14])
        assert d < 0 and abs(2 * math.acos(-d) - angle) < 1e-9 and np.all(kind(sc) == uc.SLERP) and np.all(has(sc, uc.D_NEG))
    assert np.array_equal(g["c_same"]["states"][-1, 10:14], g["c_same"]["states"][0, 10:14])
    assert np.array_equal(g["c_negated"]["states"][-1, 10:14], -g["c_negated"]["states"][0, 10:14])
    assert np.all(kind(g["c_same"]) == uc.LINEAR) and not has(g["c_same"], uc.D_NEG).any()
    assert np.all(kind(g["c_negated"]) == uc.LINEAR) and has(g["c_negated"], uc.D_NEG).all()
    gaps = []
    for j in range(len(uc.D_THETAS)):                                         # a few ulps below the switch: the general branch
        sc = g["d%d" % j]
        d = uc.slerp_dot(sc["states"][0, 10:14], sc["states"][-1, 10:14])
        assert 2.0 ** -52 <= 1.0 - abs(d) <= 1e-14 and abs(d) < one
        assert np.all(kind(sc) == uc.SLERP) and has(sc, uc.NEAR_ONE).all()
        assert np.isfinite(sc["imu_hi"]).all() and np.isfinite(sc["raw_hi"]).all()
        gaps.append(1.0 - abs(d))
    assert len(set(gaps)) >= 4 and min(gaps) <= 3 * 2.0 ** -52 and max(gaps) >= 4e-15
    sc = g["d_switch"]                                                        # absD == 1 - eps: the last double of the linear branch
    assert abs(uc.slerp_dot(sc["states"][0, 10:14], sc["states"][-1, 10:14])) == one and np.all(kind(sc) == uc.LINEAR)
    for name, t0 in (("e", 200.0), ("f_e", uc.EPOCH)):
        sc = g[name]
        rel, sweep = sc["rel"], 100.0
        assert sc["tfb"] == t0 and sc["states"][0, 0] == t0
        assert list(rel[:4]) == [-5.0, -7.0, 1.2 * sweep, 1.5 * sweep]
        assert has(sc, uc.CLAMP_LO)[:2].all() and has(sc, uc.CLAMP_HI)[2:4].all()
        assert np.array_equal(sc["raw"][0], sc["raw"][1]) and np.array_equal(sc["raw"][2], sc["raw"][3])
        for t, begin, end in ((0.0, 1, 0), (4e-4, 1, 0), (-4e-4, 1, 0), (1.5e-3, 0, 0), (-1.5e-3, 0, 0),
                              (sweep, 0, 1), (sweep + 4e-4, 0, 1), (sweep - 4e-4, 0, 1), (sweep + 1.5e-3, 0, 0), (sweep - 1.5e-3, 0, 0)):
            i = int(np.flatnonzero(rel == t)[0])
            assert (bool(has(sc, uc.NUDGE_BEGIN)[i]), bool(has(sc, uc.NUDGE_END)[i])) == (bool(begin), bool(end)), (name, t)
        assert has(sc, uc.CLAMP_LO).sum() == 3 and has(sc, uc.CLAMP_HI).sum() == 3       # -5, -7, -1.5e-3 ms; 1.2 x, 1.5 x, sweep + 1.5e-3 ms
    assert g["f_a"]["tfb"] == uc.EPOCH and np.spacing(uc.EPOCH) > 2e-7 and np.array_equal(g["f_a"]["rel"], g["a"]["rel"])
    assert np.all(np.diff(g["f_a"]["states"][:, 0]) > 0)
    for name, norm in (("g_long", 1.001), ("g_short", 0.999)):
        assert np.allclose(np.linalg.norm(g[name]["states"][:, 10:14], axis=1), norm, rtol=0, atol=1e-12)
    assert np.all(kind(g["g_long"]) == uc.LINEAR) and np.all(kind(g["g_short"]) == uc.SLERP)
    assert len(g["h_two"]["states"]) == 2 and len(g["h_one"]["states"]) == 1 and g["h_one"]["tfb"] < g["h_one"]["states"][0, 0]
    assert np.isnan(g["i"]["rel"][-1]) and kind(g["i"])[-1] == uc.NAN_TIME and np.all(kind(g["i"])[:-1] == uc.SLERP)
    assert np.isnan(g["i"]["imu_hi"][-1]).all() and np.isfinite(g["i"]["imu_hi"][:-1]).all()


def test_imu_scenes(golden):
    g = golden[2]
    lengths = np.diff(g["j"]["states"][:, 0])
    assert lengths.max() > 5 * lengths.min() and np.all(kind(g["j"]) != uc.UNTOUCHED)
    assert (kind(g["k"]) == uc.SMALL).sum() >= 64 and (kind(g["k"]) == uc.SO3).sum() >= 64
    assert np.allclose(np.linalg.norm(g["k"]["states"][:, 4:7], axis=1) * 0.01, 2e-4)      # crosses 1e-4 half-way through every interval
    zero = has(g["l"], uc.ZERO_GYRO)
    assert zero.sum() >= 20 and np.all(kind(g["l"])[zero] == uc.SMALL) and (kind(g["l"]) == uc.SO3).sum() >= 100
    assert np.allclose(np.linalg.norm(g["m"]["states"][:, 4:7], axis=1), 35.0) and (kind(g["m"]) == uc.SO3).sum() >= 250
    for name, t0 in (("n_200", 200.0), ("n_epoch", uc.EPOCH)):
        sc = g[name]
        assert sc["tfb"] == t0 and np.all(kind(sc) != uc.UNTOUCHED) and np.all(np.diff(sc["rel"]) > 0)
        assert has(sc, uc.NUDGE_BEGIN).sum() == 3                               # around the first state
        assert has(sc, uc.NUDGE_END).sum() >= 3 * 4                             # te - 5e-7, te, te + 5e-7 of four interior states
        for k in range(1, 5):
            for off in (-1.5e-3, -5e-4, 0.0, 5e-4, 1.5e-3):
                assert (sc["rel"] == 10.0 * k + off).sum() == 1
    st = g["o"]["states"][:, 0]
    assert st[0] == st[1] and st[3] == st[4] and has(g["o"], uc.DT_NEG).sum() >= 1 and np.all(kind(g["o"]) != uc.UNTOUCHED)
    assert g["p"]["tfb"] + g["p"]["rel"][0] / 1000.0 < g["p"]["states"][0, 0] - 1e-6 and np.all(kind(g["p"]) == uc.UNTOUCHED)
    assert np.all(kind(g["q"])[:150] != uc.UNTOUCHED) and np.all(kind(g["q"])[150:] == uc.UNTOUCHED) and g["q"]["rel"][150] < g["q"]["rel"][149]
    assert len(g["r"]["states"]) == 1 and np.all(kind(g["r"]) == uc.UNTOUCHED)
    assert np.isnan(g["s"]["rel"][-1]) and kind(g["s"])[-1] == uc.UNTOUCHED and np.all(kind(g["s"])[:-1] != uc.UNTOUCHED)
    for name in ("p", "q", "r", "s"):
        assert g[name]["sentinel"] is not None and np.all(g[name]["sentinel"] != 0.0)


def test_size_scenes(golden):
    g = golden[2]
    for n in (1, 255, 256, 257):
        for tag, mode in (("cv", CV), ("imu", IMU), ("none", NONE)):
            sc = g["t%d_%s" % (n, tag)]
            assert len(sc["raw"]) == n and sc["mode"] == mode
            assert np.all(kind(sc) == uc.UNTOUCHED) == (mode == NONE)
    names = list(g)
    assert names.index("u_small") == names.index("u_large") + 1               # the small sweep follows the large one on the same context
    large, small = g["u_large"], g["u_small"]
    assert large["mode"] == small["mode"] == IMU and len(large["raw"]) == 5000 > 4096 and np.all(large["sentinel"] != 0.0)
    assert len(small["raw"]) == 300 and small["sentinel"] is None
    assert np.all(kind(small)[:200] != uc.UNTOUCHED) and np.all(kind(small)[200:] == uc.UNTOUCHED)
    assert not small["imu_hi"][200:].any() and not small["imu_lo"][200:].any()


# ------------------------------------------------------------------------------------------------ the oracle against the exact model
def test_the_oracles_worst_error_is_oracle_worst(golden, oracle_lib, oracle_backend):
    """measured, per mode and stage, over every scene; the constants of the checker are these figures rounded up to two decimals.  The
    bit-exact branches are bit-exact for the oracle by definition; their error against the model is part of the figure all the same."""
    worst = {CV: [0.0, 0.0], IMU: [0.0, 0.0], NONE: [0.0, 0.0]}
    for sc in golden[2].values():
        imu, k, raw = uc.run_oracle(sc, oracle_lib, oracle_backend)
        assert k == (len(sc["raw"]) if sc["mode"] == CV else int((kind(sc) != uc.UNTOUCHED).sum())), sc["name"]     # the walk of the model
        untouched = kind(sc) == uc.UNTOUCHED
        start = np.zeros_like(sc["raw"]) if sc["sentinel"] is None else sc["sentinel"]
        assert uc.same_bits(imu[untouched], start[untouched]).all()
        e_imu = uc.ulp_error(imu, sc["imu_hi"], sc["imu_lo"], sc["s_imu"])
        e_raw = uc.ulp_error(raw, sc["raw_hi"], sc["raw_lo"], sc["s_raw"])
        assert np.isfinite(e_imu).all() and np.isfinite(e_raw).all(), sc["name"]          # NaN exactly where the model has one
        w = worst[sc["mode"]]
        w[0], w[1] = max(w[0], float(e_imu.max())), max(w[1], float(e_raw.max()))
    print("oracle worst e {mode: [imu_point, raw_point]}:", worst)
    for mode, w in worst.items():
        assert 0.9 * uc.ORACLE_WORST_BY_MODE[mode] <= max(w) <= uc.ORACLE_WORST_BY_MODE[mode], (mode, w)
    assert uc.ORACLE_WORST == max(uc.ORACLE_WORST_BY_MODE.values())
    assert uc.K == math.ceil(4 * uc.ORACLE_WORST) == 11
