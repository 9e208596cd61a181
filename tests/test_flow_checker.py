"""Known answers and preconditions of tests/flow_checker.py, the sequential restatement the device's optical flow is compared with
(tests/test_gpu_flow.py).  No reference, no device.

Exit classes over the (point, level) visits of the tracking calls of all scenes, as the checker produces them (printed by
test_every_exit_class_occurs): start outside the admitted range 9, minEig rejection 33, walked out of range 1, stop by epsilon 2214,
stop by the oscillation rule 29, max_count exhausted 178; admitted window corners at ix == -21: 3, ix == cols - 1: 3, iy == -21: 2,
iy == rows - 1: 2."""
import numpy as np
import pytest

import flow_checker as fc


def test_pyr_down_of_a_constant_image_is_the_constant():
    for shape in ((7, 9), (8, 8), (1, 5), (5, 1), (23, 30)):
        for c in (0, 1, 127, 255):
            out = fc.pyr_down(np.full(shape, c, np.uint8))
            assert out.shape == ((shape[0] + 1) // 2, (shape[1] + 1) // 2) and (out == c).all()


def test_pyr_down_of_a_ramp():
    """img[y, x] = 3 x: inside, the symmetric kernel returns the centre tap, 3 * 2 x'; at the left edge the taps -2, -1 reflect to 2, 1:
    (6 + 4 * 3 + 0 + 4 * 3 + 6) / 16 = 2.25 -> (36 * 16 + 128) >> 8 = 2; at the right edge of 9 columns (x' = 4, taps 6, 7, 8, 7, 6):
    (18 + 4 * 21 + 6 * 24 + 4 * 21 + 18) / 16 = 21.75 -> 22"""
    img = np.tile((3 * np.arange(9)).astype(np.uint8), (6, 1))
    out = fc.pyr_down(img)
    assert out.shape == (3, 5)
    assert (out == np.array([2, 6, 12, 18, 22], np.uint8)[None, :]).all()
    assert (fc.pyr_down(img.T.copy()) == out.T).all()


def test_pyr_down_of_strips():
    """1 x N and N x 1: the pass across the single row or column sees one pixel five times (weight 16); along the strip
    [10 20 40 80 160 200]: x' = 0: taps 40 20 10 20 40 -> (40 + 80 + 60 + 80 + 40) / 16 = 18.75 -> 19; x' = 1: 10 20 40 80 160 ->
    (10 + 80 + 240 + 320 + 160) / 16 = 50.625 -> 51; x' = 2: 40 80 160 200 160 (6 reflects to 4) -> (40 + 320 + 960 + 800 + 160) / 16 = 142.5 -> 143
    ((2280 * 16 + 128) >> 8 = 143)"""
    strip = np.array([[10, 20, 40, 80, 160, 200]], np.uint8)
    assert fc.pyr_down(strip).tolist() == [[19, 51, 143]]
    assert fc.pyr_down(strip.T.copy()).tolist() == [[19], [51], [143]]
    assert fc.pyr_down(np.array([[77]], np.uint8)).tolist() == [[77]]


def test_reflect_and_padding():
    assert [fc.reflect101(p, 5) for p in range(-6, 11)] == [2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2]
    assert [fc.reflect101(p, 1) for p in (-3, 0, 4)] == [0, 0, 0]
    img = np.arange(12, dtype=np.uint8).reshape(3, 4)
    pad = fc.pad_reflect(img, 2)
    assert pad.shape == (7, 8) and pad[2:5, 2:6].tolist() == img.tolist()
    assert pad[0].tolist() == [10, 9, 8, 9, 10, 11, 10, 9] and pad[:, 0].tolist() == [10, 6, 2, 6, 10, 6, 2]


def test_scharr_of_a_ramp_is_32_times_the_slope_and_reflects_at_the_edges():
    """img = 5 x + 2 y: Ix = (3 + 10 + 3) * (2 * 5) / ... = 32 * 5 inside, Iy = 32 * 2; at an edge the neighbour beyond it is the reflected
    one, so the central difference across the edge is 0: Ix = 0 in the first and last column, Iy = 0 in the first and last row"""
    y, x = np.mgrid[0:9, 0:11]
    d = fc.scharr((5 * x + 2 * y).astype(np.uint8)).astype(np.int64)
    assert (d[1:-1, 1:-1, 0] == 32 * 5).all() and (d[1:-1, 1:-1, 1] == 32 * 2).all()
    assert (d[:, 0, 0] == 0).all() and (d[:, -1, 0] == 0).all() and (d[0, :, 1] == 0).all() and (d[-1, :, 1] == 0).all()
    assert (d[1:-1, 0, 1] == 32 * 2).all() and (d[0, 1:-1, 0] == 32 * 5).all()
    pz = fc.pad_zero(d.astype(np.int16))
    assert pz.shape == (9 + 42, 11 + 42, 2) and not pz[:21].any() and not pz[:, :21].any() and not pz[-21:].any() and not pz[:, -21:].any()


def test_level_rule():
    assert fc.num_levels(120, 160, 3) == 2 and fc.num_levels(157, 203, 3) == 2 and fc.num_levels(185, 233, 3) == 3
    assert fc.num_levels(44, 60, 3) == 1 and fc.num_levels(512, 640, 3) == 3 and fc.num_levels(30, 30, 3) == 0 and fc.num_levels(120, 160, 1) == 1
    p = fc.Pyramid(fc.scene("shift_203x157")[0][0], 3)
    assert p.sizes == [(157, 203), (79, 102), (40, 51)]      # odd extents at every level


def test_an_integer_translation_is_recovered():
    """a textured image displaced by whole pixels: every point whose window stays inside ends within 0.05 px of the displacement --
    the iteration stops once |delta|^2 <= 0.05 and the next step of a converging Gauss-Newton iteration is smaller than the last, so
    this is a sanity bound from the stop criterion, not a parity tolerance"""
    rows, cols = 120, 160
    tex = fc.texture(5, rows, cols)
    a, b = fc.crop(tex, rows, cols, 0, 0), fc.crop(tex, rows, cols, 2, 3)      # b(y, x) = a(y + 2, x + 3): content moves by (-3, -2)
    pts = fc.grid_points(8, rows - 50, cols - 50, 40) + np.float32(25.0)
    tr = fc.Tracker()
    tr.track_image(a, pts)
    nxt, status, nt = tr.track_image(b, pts)
    assert nt == 40 and status.all()
    err = np.abs((nxt - pts).astype(np.float64) - np.array([-3.0, -2.0]))
    print("largest error of the recovered translation:", err.max())
    assert err.max() <= 0.05


@pytest.fixture(scope="module")
def traces():
    out = {}
    for name in fc.SCENES:
        tr = []
        res = fc.run_scene(name, tr)
        out[name] = (res, tr)
    return out


def test_every_exit_class_occurs(traces):
    total = {k: 0 for k in fc.EXIT_CLASSES}
    edges = {"ix_min": 0, "ix_max": 0, "iy_min": 0, "iy_max": 0}
    for name, (res, tr) in traces.items():
        c, e = fc.exit_counts(tr), fc.admission_edges(tr)
        print(name, c, e)
        for k in total:
            total[k] += c[k]
        for k in edges:
            edges[k] += int(e[k])
    print("all scenes:", total, edges)
    for k in fc.EXIT_CLASSES:
        assert total[k] >= 1, k
    for k in edges:
        assert edges[k] >= 1, k
    # the crafted scenes are what they are named for
    assert fc.exit_counts(traces["gain_160x120"][1])[fc.OSCILLATION] >= 1
    assert fc.exit_counts(traces["flat_far_160x120"][1])[fc.MIN_EIG] >= 1 and fc.exit_counts(traces["flat_far_160x120"][1])[fc.MAX_COUNT] >= 1
    e = fc.exit_counts(traces["edges_160x120"][1])
    assert e[fc.START_OUTSIDE] >= 1 and e[fc.WALKED_OUT] >= 1


def test_the_oscillation_rule_applies_its_half_step():
    """a level-0 visit that ends by the oscillation rule leaves the point half a step behind the position of its last update"""
    imgs, pts, opts = fc.scene("gain_160x120")
    prev, cur = fc.Pyramid(imgs[0], opts.max_level), fc.Pyramid(imgs[1], opts.max_level)
    hit = 0
    with np.errstate(all="ignore"):
        for p in pts:
            tr = []
            nx, ny, _ = fc.track_point(prev, cur, prev.L, p, opts, tr)
            level, why, info = tr[-1]
            if level == 0 and why == fc.OSCILLATION:
                (dx, dy), (bx, by) = info["delta"], info["before"]
                assert float(dx) ** 2 + float(dy) ** 2 > opts.epsilon
                assert nx == bx - dx * np.float32(0.5) and ny == by - dy * np.float32(0.5) and (nx != bx or ny != by)
                hit += 1
    print("level-0 visits ended by the oscillation rule:", hit)
    assert hit >= 1


@pytest.mark.parametrize("name", ["shift_160x120", "shift_203x157", "shift_233x185"])
def test_at_least_half_the_points_of_a_shifted_texture_are_tracked(traces, name):
    for nxt, status, nt, _ in traces[name][0][1:]:
        assert nt == int(status.sum()) and 2 * nt >= len(status)


def test_first_image_and_size_change():
    imgs, pts, _ = fc.scene("lowered_60x44")
    tr = fc.Tracker()
    nxt, status, nt = tr.track_image(imgs[0], pts)
    assert status is None and nt == 0 and nxt.tobytes() == pts.tobytes() and tr.max_level == 1
    tr.track_image(imgs[1], pts)
    assert tr.max_level == 1                     # the lowered level count stays
    with pytest.raises(ValueError):
        tr.track_image(imgs[1][:, :50], pts)
    assert fc.guarded(np.float32(np.nan), np.float32(1)) and fc.guarded(np.float32(1), np.float32(-np.inf)) and fc.guarded(np.float32(1e12), np.float32(0))
    assert not fc.guarded(np.float32(-1e6), np.float32(2e9))
