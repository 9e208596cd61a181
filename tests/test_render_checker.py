"""tests/render_checker.py by itself, without a device and without the reference: known answers of the OpenCV byte semantics the colour
fetch rests on (`double * Vec3b` = saturate_cast<uchar>(w * pixel), round to nearest even, clamped; `Vec3b + Vec3b`
saturates, left to right), saturate_cast against an independent integer formulation, the preconditions of the scene -- every outcome of
the loop occurs often enough for the device tests to mean something -- and the recorded golden file.

The preconditions are conditions, not measurements: if the checker misses one, the scene is wrong, not the bar."""
import fractions
import os

import numpy as np
import pytest

import render_checker as rk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flat(value, rows=4, cols=4):
    return np.full((rows, cols, 3), value, np.uint8)


# ------------------------------------------------------------------------------------------------ the pixel fetch: known answers
def test_the_colour_is_a_sum_of_four_rounded_bytes_not_a_rounded_bilinear_value():
    # 255 at weights 0.5 / 0.5: 128 + 128 saturates to 255; 1 at weight 0.5: round-half-even(0.5) = 0; 3 at 0.5: 1.5 -> 2
    assert rk.sub_pixel(_flat(255), 1.0, 1.5) == ([255, 255, 255], True)
    assert rk.sub_pixel(_flat(255), 1.5, 1.0) == ([255, 255, 255], True)
    assert rk.sub_pixel(_flat(1), 1.0, 1.5)[0] == [0, 0, 0]                 # bilinear: 1
    assert rk.sub_pixel(_flat(3), 1.0, 1.5)[0] == [4, 4, 4]                 # 2 + 2; bilinear: 3
    assert rk.sub_pixel(_flat(1), 1.5, 1.5)[0] == [0, 0, 0]                 # four times round(0.25)
    assert rk.sub_pixel(_flat(2), 1.5, 1.5)[0] == [0, 0, 0]                 # four times round-half-even(0.5) = 0; bilinear: 2
    assert rk.sub_pixel(_flat(6), 1.5, 1.5)[0] == [8, 8, 8]                 # four times round-half-even(1.5) = 2; bilinear: 6
    assert rk.sub_pixel(_flat(255), 1.5, 1.5) == ([255, 255, 255], True)    # 64 + 64 + 64 + 64 = 256 -> 255
    # an integral position reads one pixel with weight 1
    img = np.arange(4 * 5 * 3, dtype=np.uint8).reshape(4, 5, 3)
    assert rk.sub_pixel(img, 2.0, 3.0)[0] == [int(v) for v in img[2, 3]]
    # the channels lie as the image holds them (BGR stays BGR)
    img = _flat(0); img[..., 0] = 10; img[..., 1] = 20; img[..., 2] = 30
    assert rk.sub_pixel(img, 1.25, 1.75)[0] == [sum(rk.sat8(w, c) for w in (0.75 * 0.25, 0.25 * 0.25, 0.75 * 0.75, 0.25 * 0.75)) for c in (10, 20, 30)]


def test_254_at_four_quarters():
    # 254 * 0.25 = 63.5 rounds to the even 64, four times: 256 saturates to 255 -- one more than the byte itself
    assert rk.sub_pixel(_flat(254), 1.5, 1.5) == ([255, 255, 255], True)


@pytest.mark.parametrize("fr,fc", [(0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5), (0.25, 0.75), (0.75, 0.25), (0.125, 0.5), (0.999, 0.001)])
def test_every_weight_pattern_at_saturation(fr, fc):
    """an all-255 image: the four rounded terms add up to 255 +- rounding and the 8-bit adds clamp at 255, never wrap"""
    w = ((1 - fr) * (1 - fc), fr * (1 - fc), (1 - fr) * fc, fr * fc)
    terms = [rk.sat8(x, 255) for x in w]
    acc = 0
    for t in terms:
        acc = min(acc + t, 255)
    colour, saturated = rk.sub_pixel(_flat(255), 1.0 + fr, 1.0 + fc)
    assert colour == [acc] * 3 and saturated == (sum(terms) > 255) and 253 <= acc <= 255


def test_the_order_of_the_saturating_adds_is_left_to_right():
    # (200 + 100 -> 255) is not undone by what follows: saturation is not a final clamp of a wide sum in general, but with bytes >= 0
    # both give min(sum, 255); what the order decides is WHICH pixel meets WHICH weight
    img = _flat(0)
    img[1, 1] = 10; img[2, 1] = 20; img[1, 2] = 40; img[2, 2] = 80          # (floor, floor), (ceil_row, floor), (floor, ceil_col), (ceil, ceil)
    got = rk.sub_pixel(img, 1.25, 1.5)[0]
    want = rk.sat8(0.75 * 0.5, 10) + rk.sat8(0.25 * 0.5, 20) + rk.sat8(0.75 * 0.5, 40) + rk.sat8(0.25 * 0.5, 80)
    assert got == [want] * 3 == [4 + 2 + 15 + 10] * 3


def test_ties_round_to_even_for_odd_and_even_bytes():
    for b in range(256):
        half = rk.sat8(0.5, b)
        assert half == (b // 2 if b % 2 == 0 else (b // 2 if (b // 2) % 2 == 0 else b // 2 + 1)), b
    assert [rk.sat8(0.5, b) for b in (1, 3, 5, 7, 253, 255)] == [0, 2, 2, 4, 126, 128]
    assert [rk.sat8(0.25, b) for b in (2, 6, 10, 254)] == [0, 2, 2, 64]


def test_saturate_cast_against_an_independent_integer_formulation():
    """all 256 bytes over a few thousand weights: the double product w * b is formed exactly as a fraction and rounded to the nearest
    integer, ties to even, with integer arithmetic only"""
    rng = np.random.default_rng(11)
    weights = np.concatenate([rng.random(3000), rng.random(500) * rng.random(500), np.arange(0, 257) / 256.0, [0.0, 1.0, 0.5, 0.25, 0.75, 1e-300, 1 - 2.0**-53]])
    for w in weights:
        w = float(w)
        for b in range(256):
            x = fractions.Fraction(w * float(b))                            # the double the multiplication gives, exactly
            fl = x.numerator // x.denominator
            rem = x - fl
            want = fl + (1 if rem > fractions.Fraction(1, 2) or (rem == fractions.Fraction(1, 2) and fl % 2 == 1) else 0)
            assert rk.sat8(w, b) == min(max(want, 0), 255), (w, b)


def test_against_opencv_where_it_is_installed():
    """not depended on: OpenCV's own saturate_cast<uchar>(double) (convertScaleAbs of a CV_64F array) and its saturating 8-bit add"""
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(12)
    w = np.concatenate([rng.random(2000), [0.5, 0.25, 0.75, 0.125]])
    b = rng.integers(0, 256, len(w))
    b[-4:] = (3, 254, 2, 4)
    prod = (w * b.astype(np.float64)).reshape(1, -1)
    got = cv2.convertScaleAbs(prod).ravel()
    assert [int(v) for v in got] == [rk.sat8(float(x), int(y)) for x, y in zip(w, b)]
    x, y = rng.integers(0, 256, (1, 500)).astype(np.uint8), rng.integers(0, 256, (1, 500)).astype(np.uint8)
    assert [int(v) for v in cv2.add(x, y).ravel()] == [rk.add8(int(p), int(q)) for p, q in zip(x.ravel(), y.ravel())]


# ------------------------------------------------------------------------------------------------ updateRgb: known answers
def test_update_rgb_known_answers():
    s = rk.RgbState()
    assert s.update_rgb([10.0, 20.0, 30.0], 5.0, 1.0) == 0                  # the first observation returns 0 as the reference does
    assert (s.rgb, s.n_rgb, s.observe_distance, s.last_observe_time) == ([10, 20, 30], 1, 5.0, 1.0) and all(float(c) == 15.0 for c in s.cov)
    assert s.update_rgb([10.0, 20.0, 30.0], 6.0 + 1e-9, 2.0) == -1          # beyond 1.2 x the distance: nothing changes
    assert (s.n_rgb, s.last_observe_time) == (1, 1.0)
    assert s.update_rgb([10.0, 20.0, 30.0], 6.0, 1.0) == 1                  # exactly 1.2 x passes; a zero time step
    cov = np.float32(np.sqrt(1.0 / (1.0 / 225.0 + 1.0 / 225.0)))
    assert all(c == cov for c in s.cov) and s.n_rgb == 2 and s.observe_distance == 5.0
    # the (short) cast truncates: 10 * (cov^2 [FP32] * 2 / 225) is a hair off 10
    assert s.rgb[0] in (9, 10) and s.rgb[0] == int(float(cov * cov) * (10 / 225.0 + 10.0 / 225.0))
    assert rk.to_short(-3.9) == -3 and rk.to_short(3.9) == 3 and rk.to_short(40000.0) == 40000 - 65536
    assert rk.to_short(float("nan")) == 0 and rk.to_short(float("inf")) == 0 and rk.to_short(-1e30) == 0


# ------------------------------------------------------------------------------------------------ the scene's preconditions
def test_the_scene_reaches_every_outcome_often_enough():
    rc, totals, map_states, reg_states = rk.scene_sequence()
    seen = rc.seen
    assert len(rk.RENDERS) >= 4 and len({r[2] for r in rk.RENDERS}) >= 4 and len({r[0] for r in rk.RENDERS}) >= 4      # times, poses
    assert {r[1] for r in rk.RENDERS} == {0, 1} and rk.IMAGE_SIZES[1][1] % 64 != 0
    for name in ("behind", "u_low", "u_high", "v_low", "v_high", "gated", "first", "updated_n3", "repeated_voxels"):
        assert seen[name] >= 100, (name, seen[name])
    assert seen["coloured"] >= 0.30 * seen["listed"] and seen["not_coloured"] >= 0.05 * seen["listed"]
    assert seen["saturated"] >= 10
    assert seen["listed"] == sum(t["listed"] for t in totals)
    for t in totals:
        assert t["listed"] == t["behind"] + t["outside"] + t["gated"] + t["first"] + t["updated"] and t["unknown"] == 0
    # a zero and a negative time step are part of the sequence
    times = [r[2] for r in rk.RENDERS]
    assert any(b == a for a, b in zip(times, times[1:])) and any(b < a for a, b in zip(times, times[1:]))
    # the registered order is a selection of the map order
    assert len(reg_states[-1][1]) == len(rc.map.registered) < len(map_states[-1][1]) == rc.map.num_points


def test_the_golden_file_holds_the_checkers_states():
    g_totals, g_states = rk.golden_unpack(np.load(os.path.join(ROOT, "tests", "golden", "golden_color_render.npz"), allow_pickle=False))
    _, totals, map_states, _ = rk.scene_sequence()
    assert len(g_totals) == len(rk.RENDERS)
    for k in range(len(rk.RENDERS)):
        assert g_totals[k] == tuple(totals[k][name] for name in rk.TOTALS), k
        assert rk.state_bytes(g_states[k]) == rk.state_bytes(map_states[k]), k
        for a, b in zip(g_states[k], map_states[k]):
            assert a.dtype == b.dtype and a.shape == b.shape
