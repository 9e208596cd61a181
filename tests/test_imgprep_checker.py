"""Known answers for tests/imgprep_checker.py itself (CPU): the yardstick of the image preparation is checked against cases whose
results follow from the specification by hand."""
from fractions import Fraction

import numpy as np

import imgprep_checker as ck


def _image(rows, cols, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(rows, cols, 3), dtype=np.uint8)


def test_zero_distortion_is_the_identity_map_and_the_identity_remap():
    rows, cols = 37, 53
    map1, map2 = ck.build_map(rows, cols, 400.0, 410.0, 26.3, 18.7, [0, 0, 0, 0, 0])
    jj, ii = np.meshgrid(np.arange(cols), np.arange(rows))
    assert (map2 == 0).all() and (map1[..., 0] == jj).all() and (map1[..., 1] == ii).all()
    img = _image(rows, cols, 1)
    assert np.array_equal(ck.remap(img, map1, map2), img)


def test_the_weights_sum_to_32768_for_all_1024_fractions():
    ax, ay = np.meshgrid(np.arange(32), np.arange(32))
    w = ck.weights(ax, ay)
    assert ax.size == 1024 and (sum(w) == 32768).all() and all((x >= 0).all() for x in w)


def test_a_half_pixel_shift_averages_neighbours_and_the_border_is_zero():
    img = np.zeros((16, 16, 3), np.uint8)
    img[:, :, :] = (np.arange(16) * 10)[None, :, None]
    map1 = np.zeros((16, 16, 2), np.int16)
    map1[..., 0] = np.arange(16)[None, :]
    map1[..., 1] = np.arange(16)[:, None]
    map2 = np.full((16, 16), 16, np.uint16)               # ax = 16, ay = 0
    out = ck.remap(img, map1, map2)
    assert (out[:, :15, 0] == (np.arange(15) * 10 + 5)[None, :]).all()
    assert (out[:, 15, 0] == 75).all()                    # (150 + 0) / 2: the neighbour outside contributes 0
    map1[...] = -32768
    assert (ck.remap(img, map1, np.zeros((16, 16), np.uint16)) == 0).all()


def test_gray_of_a_gray_pixel_is_that_value_and_the_ycrcb_round_trip_is_the_identity_on_gray():
    v = np.arange(256, dtype=np.uint8)
    img = np.stack([v, v, v], axis=-1)[None]
    assert np.array_equal(ck.gray(img)[0], v)
    Y, Cr, Cb = ck.bgr_to_ycrcb(img)
    assert np.array_equal(Y[0], v) and (Cr == 128).all() and (Cb == 128).all()
    assert np.array_equal(ck.ycrcb_to_bgr(Y, Cr, Cb), img)
    # channel 0 carries the RED weight (COLOR_RGB2GRAY on a BGR-held image)
    assert ck.gray(np.array([[[255, 0, 0]]], np.uint8))[0, 0] == (9798 * 255 + 16384) >> 15 == 76
    assert ck.gray(np.array([[[0, 0, 255]]], np.uint8))[0, 0] == (3735 * 255 + 16384) >> 15 == 29


def test_a_constant_plane_gives_a_constant_clahe_output():
    for rows, cols in ((37, 53), (96, 160)):
        for clip in (1.0, 3.0):
            out = ck.clahe(np.full((rows, cols), 93, np.uint8), clip)
            assert (out == out[0, 0]).all(), (rows, cols, clip)


def _round_half_even(fr):
    return int(round(fr))                                  # round() of a Fraction is exact and rounds halves to even


def test_a_hand_computed_16_by_16_image_with_one_tile_over_the_limit():
    clip, tiles = 40.0, 2
    plane = np.zeros((16, 16), np.uint8)
    # tile (0, 0): 40 pixels of 10, 8 of 20, 16 of 200; the other three tiles hold 0 ... 63 once each
    plane[:8, :8] = np.array([10] * 40 + [20] * 8 + [200] * 16, np.uint8).reshape(8, 8)
    ramp = np.arange(64, dtype=np.uint8).reshape(8, 8)
    plane[:8, 8:], plane[8:, :8], plane[8:, 8:] = ramp, ramp, ramp
    assert ck.tiling(16, 16, tiles) == (2, 8, 8, 16, 16)
    limit = ck.clip_limit(clip, 64)
    assert limit == 10                                     # (int)(40 * 64 / 256)
    hist = np.bincount(plane[:8, :8].ravel(), minlength=256)
    assert hist[10] == 40 and hist[20] == 8 and hist[200] == 16 and hist.sum() == 64
    lut, excess, batch, res, step = ck.tile_lut(hist, limit, 64)
    assert (excess, batch, res, step) == (30 + 6, 0, 36, 7)      # 256 // 36 = 7: bins 0, 7, ..., 245 get + 1 (36 of them)
    expect = []
    for i in range(256):
        c = min(i, 245) // 7 + 1 + (10 if i >= 10 else 0) + (8 if i >= 20 else 0) + (10 if i >= 200 else 0)
        expect.append(_round_half_even(Fraction(c * 255, 64)))
    assert expect[0] == 4 and expect[9] == 8 and expect[10] == 48 and expect[199] == 187 and expect[200] == 227 and expect[255] == 255
    assert lut.tolist() == expect
    luts, lim = ck.clahe_luts(plane, clip, tiles)
    assert lim == 10 and luts[0, 0].tolist() == expect
    ramp_lut = [_round_half_even(Fraction(min(i + 1, 64) * 255, 64)) for i in range(256)]      # no bin above the limit: the plain cumulative sum
    assert ramp_lut[31] == 128                             # 32 * 255 / 64 = 127.5 rounds to the even 128
    for t in ((0, 1), (1, 0), (1, 1)):
        assert luts[t].tolist() == ramp_lut
    # the corner pixels lie before the first tile centre: no blend, the tile's own table
    out = ck.clahe(plane, clip, tiles)
    assert out[0, 0] == expect[10] and out[15, 15] == ramp_lut[63] and out[0, 15] == ramp_lut[7]


def test_the_limit_saturates_at_int32_max_before_the_cast():
    assert ck.clip_limit(1e12, 300) == 2147483647                  # 1 171 875 000 000 without the min
    assert ck.clip_limit(1e300, 16) == 2147483647
    assert ck.clip_limit(2147483647.0, 256) == 2147483647 and ck.clip_limit(2147483646.5, 256) == 2147483646      # the last values below it
    assert ck.clip_limit(3.0, 140) == 1 and ck.clip_limit(1e-300, 256) == 1 and ck.clip_limit(40.0, 64) == 10     # truncated, raised to 1
    # a tile under a saturated limit is never cut
    lut, excess, batch, res, step = ck.tile_lut(np.bincount([7] * 300, minlength=256), ck.clip_limit(1e12, 300), 300)
    assert (excess, batch, res, step) == (0, 0, 0, 0) and lut[6] == 0 and lut[7] == 255


def test_the_extension_rule():
    assert ck.tiling(96, 160) == (8, 20, 12, 96, 160)              # both divide: no extension
    assert ck.tiling(96, 170) == (8, 22, 13, 104, 176)             # cols do not: rows grow by a whole T
    assert ck.tiling(37, 53) == (4, 14, 10, 40, 56)                # neither divides
    assert ck.tiling(1024, 1280) == (64, 20, 16, 1024, 1280)       # the product shape
    plane = np.arange(96 * 170, dtype=np.int64).reshape(96, 170)
    ext = ck.extend(plane, 8)
    assert ext.shape == (104, 176) and np.array_equal(ext[:96, :170], plane)
    for k in range(6):
        assert np.array_equal(ext[:96, 170 + k], plane[:, 168 - k])      # reflect-101: index 2 (n - 1) - (n + k) = n - 2 - k
    for k in range(8):
        assert np.array_equal(ext[96 + k, :170], plane[94 - k, :])
    assert np.array_equal(ck.extend(plane[:, :160], 8), plane[:, :160])


def test_non_finite_and_far_map_entries_are_the_outside_sentinel():
    # k1 so large that the polynomial overflows at the corners; the principal point itself stays finite
    map1, map2 = ck.build_map(32, 32, 1e-150, 1e-150, 16.0, 16.0, [1e300, 0, 0, 0, 0])
    assert (map1[0, 0] == -32768).all() and map2[0, 0] == 0
    assert tuple(map1[16, 16]) == (16, 16) and map2[16, 16] == 0
    # a finite position beyond int16 is clamped, not wrapped
    map1, map2 = ck.build_map(16, 16, 1e-4, 1e-4, 0.0, 0.0, [0, 0, 0, 0, 0])
    assert tuple(map1[0, 0]) == (0, 0) and tuple(map1[1, 1]) == (1, 1)
    map1, _ = ck.build_map(16, 16, 1.0, 1.0, 0.0, 0.0, [1.0, 0, 0, 0, 0])
    assert tuple(map1[15, 15]) == (15 * 451, 15 * 451)            # 15 (1 + 450)
    map1, _ = ck.build_map(16, 16, 1.0, 1.0, 0.0, 0.0, [100.0, 0, 0, 0, 0])
    assert tuple(map1[15, 15]) == (32767, 32767)
