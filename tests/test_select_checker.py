"""tests/select_checker.py against itself and against known answers (CPU): the literal loop of rgbMapTracker::selectPointsForProjection
(rgbMapTracker.cpp:45-152) and the closed-form rule the device evaluates agree on every scene of the GPU tests and on random cells whose
depths lie within a few float ulps of each other; the cell key has known answers; the golden file holds what the checker computes."""
import os

import numpy as np

import render_checker as rk
import select_checker as sk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ------------------------------------------------------------------------------------------------ the key
def test_std_round_is_half_away_from_zero():
    assert [sk.std_round(x) for x in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999999999999994, -0.49999999999999994, 2.4999999999999996, 7.0, -7.0)] == \
        [1.0, 2.0, 3.0, -1.0, -2.0, -3.0, 0.0, -0.0, 2.0, 7.0, -7.0]


def test_a_sub_unit_minimum_dis_collapses_two_quotients_into_one_key():
    # 1.1 / 0.4 rounds to 3, 1.5 / 0.4 to 4; 3 * 0.4 = 1.2000000000000002 and 4 * 0.4 = 1.6 both truncate to 1
    assert sk.std_round(1.1 / 0.4) == 3.0 and sk.std_round(1.5 / 0.4) == 4.0
    assert sk.cell_coordinate(1.1, 0.4) == sk.cell_coordinate(1.5, 0.4) == 1
    assert sk.cell_coordinate(1.9, 0.4) == 2                               # 5 * 0.4 = 2.0
    # the key is the truncated product, not the quotient
    assert sk.cell_coordinate(101.0, 7.5) == 97 and sk.std_round(101.0 / 7.5) == 13.0      # 13 * 7.5 = 97.5


def test_a_negative_coordinate_truncates_toward_zero():
    # under a negative margin u_f may be negative: -11.2 / 7.5 rounds to -1, -7.5 truncates to -7 (not the floor, -8)
    assert sk.cell_coordinate(-11.2, 7.5) == -7
    assert sk.cell_coordinate(-0.3, 0.4) == 0 and sk.cell_coordinate(-0.19, 0.4) == 0      # -1 * 0.4 = -0.4 -> 0, and -0.0 -> 0
    assert sk.cell_coordinate(-255.9, 10.0) == -260
    cam = rk.Camera((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 100.0, 100.0, 320.0, 240.0, -0.4)
    outcome, u_f, v_f = cam.project((-4.0, 0.0, 1.0), 480, 640)            # u_f = -80: inside [-0.4 cols + 1, 1.4 cols)
    assert (outcome, u_f, v_f) == (0, -80.0, 240.0) and sk.cell_coordinate(u_f, 7.5) == -82      # -11 * 7.5 = -82.5
    cam.fov_margin = 0.005
    assert cam.project((-4.0, 0.0, 1.0), 480, 640)[0] == 2


def test_a_half_way_quotient_rounds_away_from_zero():
    assert sk.cell_coordinate(25.0, 10.0) == 30 and sk.cell_coordinate(35.0, 10.0) == 40 and sk.cell_coordinate(-25.0, 10.0) == -30
    assert sk.cell_coordinate(3.75, 7.5) == 7                              # 0.5 -> 1 -> 7.5 -> 7
    assert sk.cell_coordinate(24.999999999999996, 10.0) == 20


# ------------------------------------------------------------------------------------------------ the rule
def test_the_closed_form_equals_the_loop_on_random_cells_with_depths_within_ulps():
    rng = np.random.default_rng(77)
    below = ties = 0
    for _ in range(20000):
        base = F32(rng.uniform(0.2, 150.0))
        ulp = float(np.spacing(base))
        n = int(rng.integers(1, 9))
        depths = float(base) + rng.uniform(-1.5, 1.5, n) * ulp
        depths[rng.random(n) < 0.2] = float(base)                          # exactly representable ones among them
        cand = [(3 * i + 1, float(d)) for i, d in enumerate(depths)]
        a, b = sk.sequential_holder(cand), sk.closed_form_holder(cand)
        assert a == b, cand
        M = min(F32(d) for _, d in cand)
        below += 1 if any(d < float(M) for _, d in cand) else 0
        ties += 1 if sum(1 for _, d in cand if F32(d) == M) > 1 else 0
    assert below > 2000 and ties > 2000                                    # both branches of the rule were taken


def _agree(args):
    a, b = sk.select_sequential(*args), sk.select_closed_form(*args)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    return a


def test_the_closed_form_equals_the_loop_on_the_scenes():
    smap, visited = sk.scene_map()
    # list mode: one call per parameter set and margin (the poses differ), compared whole with the cached sequence
    for n, (k, s, m) in enumerate(sk.SEQUENCE):
        if k != (s + 2 * m) % len(rk.RENDERS):
            continue
        cam, rows, cols, lists = sk.scene_camera(k, sk.MARGINS[m])
        md, skip = sk.PARAMETER_SETS[s]
        got = _agree((smap, cam, rows, cols, np.concatenate([visited[j] for j in lists]), md, skip))
        want = sk.sequence_results()[n]
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1]
    # all points, and the shells
    for batches in (3, 4):
        cam, rows, cols, _ = sk.scene_camera(*sk.ALL_POINTS_CAMERAS[1])
        got = _agree((sk.scene_map(batches)[0], cam, rows, cols, None, 10.0, 1, True))
        assert got[0].tobytes() == sk.all_points_results(batches)[1][0].tobytes()
    shell_map, want = sk.shell_scene()
    got = _agree((shell_map, sk.shell_camera(), sk.SHELL_ROWS, sk.SHELL_COLS, None, 10.0, 1, True))
    assert got[0].tobytes() == want[0].tobytes()


def test_the_scenes_reach_what_the_tests_are_about():
    res = sk.sequence_results()
    tots = [r[1] for r in res]
    assert all(t["unknown"] == 0 and t["candidates"] > 5000 and t["selected"] > 50 for t in tots)
    assert any(t["far"] > 0 for t in tots) and any(t["behind"] > 1000 for t in tots) and all(t["outside"] > 0 for t in tots)
    # the lists name voxels up to three times: more candidates than voxels
    smap, visited = sk.scene_map()
    lists = np.concatenate([visited[j] for j in rk.RENDERS[0][3]])
    assert len({tuple(v) for v in lists.tolist()}) < len(lists) == tots[0]["candidates"]
    # negative u_f or v_f under the negative margin; distinct quotients in one key at 0.4
    assert any((r[0]["u"] < 0).any() or (r[0]["v"] < 0).any() for (k, s, m), r in zip(sk.SEQUENCE, res) if m == 1)
    # a last point that is not registered (point_index -1) is a candidate like any other
    assert any((r[0]["point_index"] == -1).any() for r in res)
    # the shells: both branches of the rule decide cells where the holder is not the nearest candidate
    several, below_not_nearest, tie_not_nearest = sk.rule_census(sk.shell_scene()[1][2])
    assert below_not_nearest >= 20 and tie_not_nearest >= 20, (several, below_not_nearest, tie_not_nearest)
    # the further insertion grows the registered list and moves tails
    a, b = sk.scene_map(3)[0], sk.scene_map(4)[0]
    assert len(b.chk.registered) > len(a.chk.registered) + 1000
    moved = sum(1 for key, v in a.chk.voxels.items() if len(b.chk.voxels[key].points) > len(v.points))
    assert moved > 100


def test_the_golden_file_is_the_checkers():
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_color_select.npz"), allow_pickle=False)
    want = sk.golden_pack()
    assert sorted(g.files) == sorted(want)
    for name in g.files:
        assert g[name].dtype == want[name].dtype and g[name].tobytes() == np.ascontiguousarray(want[name]).tobytes(), name
    for n, r in enumerate(sk.sequence_results()):
        assert sk.golden_check(g, "s%d" % n, r[0], r[1]) is None
    rec, tot, _ = sk.sequence_results()[0]
    changed = rec.copy(); changed["u"][3] = np.nextafter(changed["u"][3], F32(np.inf))
    assert sk.golden_check(g, "s0", changed, tot) is not None and sk.golden_check(g, "s0", rec[:-1], tot) is not None
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_color_select.npz")) < 1 << 20
