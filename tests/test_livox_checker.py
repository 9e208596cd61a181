"""The checker of the point side (tests/livox_checker.py) checked by itself: the properties the case list is built for, the closed form
of the IMU interval walk against the walk as a loop, and the bit patterns of srl_time_unit_scale."""
import numpy as np

import livox_cases as lc
import livox_checker as lk
import sr_livo_amd as srl


def _check(case):
    return lk.decode(case["points"], case["stamp"], case["n_scans"], lk.time_unit_scale(case["unit"]), case["blind"], case["pfn"])


def test_the_cases_cover_what_they_are_built_for():
    by = {c["name"]: (c, _check(c)) for c in lc.all_cases()}
    for n in (2, 3, 63, 64, 65, 1023, 1024, 1025, 2049):
        assert by[f"size_{n}"][1]["valid"] == n - 1                 # every point but the first
    assert by["size_1"][1]["valid"] == 0
    c, w = by["size_131073"]
    assert w["valid"] == 131072 and w["picked"] == 131072 // 3 and len(c["points"]) > 131072
    for pfn, valids in ((1, (40,)), (3, (30, 31, 32)), (4, (40, 41, 43))):
        for v in valids:
            w = by[f"pfn{pfn}_valid{v}"][1]
            assert (w["valid"], w["picked"]) == (v, v // pfn)
    assert {v % 3 for v in (30, 31, 32)} == {0, 1, 2} and {v % 4 for v in (40, 41, 43)} == {0, 1, 3}
    assert by["no_valid_point"][1]["valid"] == 0 and np.isnan(by["no_valid_point"][1]["last_end_time"])
    assert by["one_valid_point"][1]["valid"] == 1 and by["one_valid_point"][1]["appended"] == 1
    c, _ = by["duplicates"]
    assert tuple(lk.valid_mask(c["points"], c["n_scans"]).astype(int)) == lc.DUPLICATES_VALID
    c, w = by["x_thresholds_and_tags"]
    m = lk.valid_mask(c["points"], c["n_scans"])
    x, tag = c["points"]["x"].astype(np.float64), c["points"]["tag"]
    assert not m[x <= 0.7].any() and m[(x > 0.7) & (x <= 2.0)][1:].all()      # float(0.7) < 0.7; tags are not looked at up to 2.0
    far = x > 2.0
    far[0] = False
    assert np.array_equal(m[far], (tag[far] & 0x0F) == 0) and m[far].any() and (~m[far]).any()
    c, _ = by["line_edges"]
    assert tuple(lk.valid_mask(c["points"], c["n_scans"]).astype(int)) == (0, 1, 0, 0, 0, 1, 1)
    c, w = by["nan_inf_1e8"]
    m = lk.valid_mask(c["points"], c["n_scans"])
    p = c["points"]
    assert not m[np.isnan(p["x"]) | np.isinf(p["x"]) | np.isinf(p["y"]) | np.isinf(p["z"])].any()
    assert m[np.isnan(p["y"]) | np.isnan(p["z"])].all()            # NaN in y or z passes every validity test
    assert not m[2] and m[4] and m[6] and m[13]                   # behind a NaN x: y and z did not move -> a duplicate
    assert tuple(m[14:22].astype(int)) == (1, 0, 1, 1, 0, 1, 0, 1)    # 1e8 itself is not > 1e8
    c, w = by["blind_edges"]
    assert w["valid"] == 10 and 0 < w["appended"] < 10
    xs = w["records"][:, 0]
    assert np.float32(1.5) not in xs and lc.up(1.5) in xs and lc.down(1.5) not in xs
    assert by["blind_zero_and_negative"][1]["appended"] == 49
    assert int(by["offsets_beyond_2_31"][0]["points"]["offset_time"].max()) >= 2 ** 31
    assert int(by["offsets_at_the_top"][0]["points"]["offset_time"].max()) == 2 ** 32 - 1
    for n in lc.TIE_CASES:
        assert by[n][1]["has_ties"]
    scales = {by[f"unit_{u}"][1]["records"][-1, 3] / float(by[f"unit_{u}"][0]["points"]["offset_time"][1:].max()) for u in (0, 1, 2, 3)}
    assert len(scales) == 4


def test_the_decode_is_sorted_stable_and_filters_by_sorted_position():
    for c in lc.all_cases():
        w = _check(c)
        rec = w["records"]
        assert np.all(rec[:-1, 3] <= rec[1:, 3]), c["name"]
        assert w["picked"] == w["valid"] // c["pfn"] and w["appended"] <= w["picked"]
        if w["appended"]:
            assert w["first_timestamp"] == rec[0, 4] and w["last_timestamp"] == rec[-1, 4]
    # ties keep message order: with every offset equal and no filter the queue IS the message order of the valid points
    c = lc.case_by_name("ties_all_zero")
    w = lk.decode(c["points"], c["stamp"], c["n_scans"], 1.0, 0.0, 1)
    assert np.array_equal(w["records"][:, 0].astype(np.float32), c["points"]["x"][1:])


def test_time_unit_scale_bit_patterns():
    # cloudProcessing.cpp:44-66: FLOAT literals widened to double
    want = {0: np.float32(1.e3), 1: np.float32(1.0), 2: np.float32(1.e-3), 3: np.float32(1.e-6), 7: np.float32(1.0), -1: np.float32(1.0)}
    for unit, f in want.items():
        got = srl.time_unit_scale(unit)
        assert np.float64(got).tobytes() == np.float64(f).tobytes() == np.float64(lk.time_unit_scale(unit)).tobytes(), unit
    assert srl.time_unit_scale(3) != 1e-6 and srl.time_unit_scale(2) != 1e-3
    assert np.float64(srl.time_unit_scale(3)).view(np.uint64) == 0x3EB0C6F7A0000000


def test_queue_cut_is_a_prefix():
    q = lk.PointQueue()
    assert q.info()[0] == 0 and len(q.cut(5.0)) == 0
    rec = np.zeros((6, 5))
    rec[:, 4] = [1.0, 2.0, 5.0, 3.0, 4.0, 6.0]                      # unsorted across messages
    q.push(rec)
    assert len(q.cut(0.5)) == 0 and q.info() == (6, 1.0, 6.0)
    assert np.array_equal(q.cut(4.5)[:, 4], [1.0, 2.0])            # stops at 5.0 although 3.0 and 4.0 would pass
    assert q.info() == (4, 5.0, 6.0)
    assert len(q.cut(5.0)) == 0                                    # <, not <=
    assert np.array_equal(q.cut(5.5)[:, 4], [5.0, 3.0, 4.0])
    assert len(q.cut(100.0)) == 1 and q.info()[0] == 0


def test_rewrite_times_both_branches():
    ts = np.array([9.9, 10.0, 10.05, 10.1, 10.2])
    keep, rel, alpha = lk.rewrite_times(ts, 10.0, 10.1, True)
    assert len(keep) == 5 and alpha[4] == 1.0 - 1e-5 and alpha[0] < 0 and rel[1] == 0.0 and alpha[3] <= 1.0
    keep, rel, alpha = lk.rewrite_times(ts, 10.0, 10.1, False)
    assert list(keep) == [1, 2, 3] and np.all(alpha <= 1.0)


def test_the_interval_rule_equals_the_walk():
    """400 000 random cases with intervals down to zero length and times on and around every boundary, where the preconditions hold (times
    and stamps non-decreasing): the closed form gives the walk's intervals, point for point."""
    rng = np.random.default_rng(20240611)
    N, SMAX, PMAX = 400_000, 6, 8
    eps = np.array([0.0, 1e-6, -1e-6, 1e-6 + 1e-9, 1e-6 - 1e-9, -1e-6 + 1e-9, -1e-6 - 1e-9, 2e-6, -2e-6, 5e-7, -5e-7])
    # the draws for all cases at once; case c uses its first S[c] stamps and first P[c] times
    S = rng.integers(1, SMAX + 1, N)
    P = rng.integers(0, PMAX + 1, N)
    gaps = rng.choice([0.0, 0.0, 1e-7, 1e-6, 2e-6, 1e-3, 5e-3], size=(N, SMAX - 1)) * rng.choice([1.0, 1.0, 0.37], size=(N, SMAX - 1))
    tfb = rng.choice([0.0, 10.0, 1.6e9], size=N)
    stamps = (tfb + rng.choice([-2e-3, 0.0, 0.0, 1e-3], size=N))[:, None] + np.concatenate([np.zeros((N, 1)), np.cumsum(gaps, axis=1)], axis=1)
    # times on and around the boundaries, in front of the first interval and beyond the last one
    which = rng.integers(-1, SMAX + 1, size=(N, PMAX))                         # -1: in front, >= S: beyond
    jitter = rng.choice(eps, size=(N, PMAX)) + rng.choice([0.0, 0.0, 1.0], size=(N, PMAX)) * 1e-4 * rng.random((N, PMAX))
    last = np.take_along_axis(stamps, (S - 1)[:, None], axis=1)
    base = np.where(which < 0, stamps[:, :1] - 1e-3, np.where(which >= S[:, None], last + 1e-3, np.take_along_axis(stamps, np.clip(which, 0, SMAX - 1), axis=1)))
    rel_all = (base + jitter - tfb[:, None]) * 1000.0
    different = reached_all = stopped = 0
    for c in range(N):
        st = stamps[c, :S[c]].tolist()
        rel = sorted(rel_all[c, :P[c]].tolist())                               # the precondition: non-decreasing (the stamps are by construction)
        walk = lk.walk_list(rel, st, float(tfb[c]))
        rule = lk.rule_list(rel, st, float(tfb[c]))
        different += walk != rule
        reached_all += bool(rel) and -1 not in walk
        stopped += -1 in walk and walk[0] != -1
    assert different == 0
    assert reached_all > 10_000 and stopped > 10_000                           # both outcomes are well represented


def test_the_rule_needs_its_preconditions():
    # a time that goes back: the walk's cursor cannot, the rule's search can -- this is what the fallback is for
    stamps = np.array([0.0, 0.01, 0.02])
    rel = np.array([15.0, 5.0])
    assert not lk.preconditions_hold(rel, stamps)
    assert list(lk.interval_walk(rel, stamps, 0.0)) == [1, -1] and list(lk.interval_rule(rel, stamps, 0.0)) == [1, 0]
