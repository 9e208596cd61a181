"""The case grid of tests/imgprep_cases.py does what it is there for (CPU; everything here is computed from tests/imgprep_checker.py alone).

1. Preconditions: the (excess, batch, res, step) every constant frame reaches, no excess at limit >= area, different limits on the two
   planes of the swapped pairs, sentinel / clamped / inside entries of the hard maps, the four border taps of the mild one, exact ties of
   the blend, undist == raw on the identity cases, the tile geometry of every geometry case.
2. Wrong variants: twelve versions of the rule with ONE mistake each, written here as small local functions over the checker's own pieces.
   Each gives other bytes than the checker on the cases named in TELLS -- so a device that made that mistake would fail
   tests/test_gpu_image_prep_envelope.py on them.  The bytes counted are those the device test compares after the plane stages: both
   sets of tables and both results."""
import numpy as np
import pytest

import imgprep_cases as ic
import imgprep_checker as ck

F32, F64 = np.float32, np.float64
STAGES = ("lut_gray", "lut_y", "gray_eq", "bgr_eq")


# ------------------------------------------------------------------------------------------------ 1. preconditions
def _tile_stats(plane, clip, tiles):
    """the set of (excess, batch, res, step) over the tiles of the plane, and the limit"""
    T, tw, th, _, _ = ck.tiling(plane.shape[0], plane.shape[1], tiles)
    ext = ck.extend(plane, T)
    limit = ck.clip_limit(clip, tw * th)
    out = set()
    for ty in range(T):
        for tx in range(T):
            hist = np.bincount(ext[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=256)
            out.add(tuple(int(v) for v in ck.tile_lut(hist, limit, tw * th)[1:]))
    return out, limit


def _both_planes(case):
    w = ic.want(case["name"])
    return _tile_stats(w["gray"], case["clip_gray"], case["tiles"]), _tile_stats(w["y"], case["clip_color"], case["tiles"])


def test_the_grid_keeps_to_its_sizes_and_hands_over_strided_read_only_frames():
    assert len(ic.CASES) == len(ic.BY_NAME) == 74
    for c in ic.CASES:
        assert (c["rows"] <= 128 and c["cols"] <= 128) or (c["rows"], c["cols"]) in ((16, 400), (400, 16)), c["name"]
        img = c["image"]
        assert img.shape == (c["rows"], c["cols"], 3) and img.strides == (3 * c["cols"] + 13, 3, 1) and not img.flags.writeable
        rows_of_bytes = np.lib.stride_tricks.as_strided(img, shape=(c["rows"], img.strides[0]), strides=(img.strides[0], 1), writeable=False)
        assert (rows_of_bytes[:, 3 * c["cols"]:] == 0xA5).all(), c["name"]      # the buffer holds rows x stride bytes


@pytest.mark.parametrize("name", [c["name"] for c in ic.CASES if "expect" in c])
def test_every_tile_of_a_constant_frame_reaches_its_excess_batch_residual_and_step(name):
    c = ic.BY_NAME[name]
    (sg, lg), (sy, ly) = _both_planes(c)
    assert sg == {c["expect"]} and sy == {c["expect"]}, (sg, sy)
    if "limit" in name:
        assert lg == ly == int(name.split()[-1])


def test_the_constant_frames_reach_every_listed_residual():
    reached = {c["expect"] for c in ic.CASES if "expect" in c}
    assert {(r[2], r[3]) for r in reached if r[1] == 0} >= {(255, 1), (129, 1), (128, 2), (85, 3), (3, 85), (2, 128), (1, 256), (0, 0), (56, 4)}
    assert {r for r in reached if r[1]} == {(1023, 3, 255, 1), (769, 3, 1, 256), (768, 3, 0, 0)}


def test_no_tile_has_an_excess_at_a_limit_of_the_area_or_more():
    seen = 0
    for c in ic.CASES:
        w = ic.want(c["name"])
        area = w["info"][1] * w["info"][2]
        (sg, lg), (sy, ly) = _both_planes(c)
        for stats, limit in ((sg, lg), (sy, ly)):
            if limit >= area:
                assert stats == {(0, 0, 0, 0)}, c["name"]
                seen += 1
    assert seen >= 12          # the saturated limits among them
    assert ic.want("clip 64x64 (1e+300, 1000000000000.0)")["info"][5:] == (2147483647, 2147483647)
    assert ic.want("clip 37x53 (1e+12, 3.0)")["info"][5:] == (2147483647, 1)


def test_the_clip_cases_reach_their_limits():
    limits = [ic.want(c["name"])["info"][5:] for c in ic.CASES if c["group"] == "clip"]
    assert limits == [(1, 1), (1, 1), (2, 255), (255, 2), (256, 1), (1, 256), (1000000, 40), (2147483647, 2147483647), (6, 1), (2147483647, 1)]
    # 256 / 140 * 7 * 140 / 256 is 6.999... in FP64: truncated to 6 where rounding gives 7
    assert 6.99 < np.float64(256 / 140 * 7) * np.float64(140) / 256 < 7.0
    for a, b in ic.SWAPPED_PAIRS:
        la, lb = ic.want(a)["info"][5:], ic.want(b)["info"][5:]
        assert la[0] != la[1] and la == lb[::-1]
        # ... and the planes differ enough that the limits cannot be exchanged unseen
        assert not np.array_equal(ic.want(a)["lut_gray"], ic.want(b)["lut_gray"]) and not np.array_equal(ic.want(a)["lut_y"], ic.want(b)["lut_y"])


@pytest.mark.parametrize("name", [c["name"] for c in ic.CASES if c["identity"]])
def test_the_identity_cases_leave_the_raw_frame(name):
    c = ic.BY_NAME[name]
    w = ic.want(name)
    assert np.array_equal(w["undist"], ic.raw(c)) and (w["map2"] == 0).all()


def test_the_content_cases_are_what_they_claim():
    two = ic.raw(ic.BY_NAME["two levels 64x64"])[..., 0]
    assert set(np.unique(two)) == {0, 255} and (two[:, 1:] != two[:, :-1]).all() and (two[1:] != two[:-1]).all()
    per = ic.raw(ic.BY_NAME["one value per tile 64x64"])[..., 0].astype(int)
    tiles = per.reshape(4, 16, 4, 16)
    assert (tiles == tiles[:, :1, :, :1]).all()
    v = tiles[:, 0, :, 0]
    assert np.abs(np.diff(v, axis=0)).min() >= 77 and np.abs(np.diff(v, axis=1)).min() >= 77 and (np.abs(np.diff(v, axis=1)) == 255).any()
    cls = ic.raw(ic.BY_NAME["one class per tile 64x64"])[..., 0].reshape(4, 16, 4, 16)
    for ty in range(4):
        for tx in range(4):
            top = min(40 * (1 + tx + ty), 255)
            assert cls[ty, :, tx].max() <= top and cls[ty, :, tx].max() > 0.8 * top


@pytest.mark.parametrize("name", list(ic.GEOMETRY))
def test_the_geometry_cases_reach_their_tiles(name):
    rows, cols, tiles, info = ic.GEOMETRY[name]
    w = ic.want(name)
    assert w["info"][:5] == info
    assert (w["map1"][..., 0] < 0).any() and (w["map1"][..., 0] >= cols - 1).any()      # the mild map still reaches outside


def test_the_geometry_cases_cover_what_the_grid_is_for():
    info = {n: ic.want(n)["info"] for n in ic.GEOMETRY}
    area = {n: i[1] * i[2] for n, i in info.items()}
    assert area["geometry 16x16 default"] == 16 and area["geometry 16x16 tiles 8"] == 4 and area["geometry 32x32 tiles 4"] == 64
    assert area["geometry 20x52 tiles 4"] == 65 and area["geometry 16x400 tiles 8"] == area["geometry 400x16 tiles 8"] == 100
    assert info["geometry 16x16 default"][5:] == (1, 1) and 3.0 * 16 / 256 < 1      # the limit raised from 0
    assert (17 * 19) % 4 == 3 and (18 * 21) % 4 == 2
    assert info["geometry 32x37 default"][3] == 32 + 4 and 32 % 4 == 0               # rows divided and grew by a whole T
    assert ic.want("geometry 32x37 default clips (40, 20)")["info"][5:] == (14, 7)
    assert info["geometry 50x120 default"][0] == 6 and max(int(50 * 32.0 / 640), 4) == 4


def _map_counts(name):
    c = ic.BY_NAME[name]
    w = ic.want(name)
    sx, sy, m2 = w["map1"][..., 0].astype(int), w["map1"][..., 1].astype(int), w["map2"]
    sentinel = (sx == -32768) & (sy == -32768) & (m2 == 0)
    high = ((sx == 32767) | (sy == 32767)) & ~sentinel
    low = ((sx == -32768) | (sy == -32768)) & ~sentinel
    inside = (sx >= -1) & (sx < c["cols"]) & (sy >= -1) & (sy < c["rows"])           # at least one tap inside the image
    return int(sentinel.sum()), int(high.sum()), int(low.sum()), int(inside.sum())


def test_the_map_cases_hold_sentinels_clamps_and_a_few_pixels_inside():
    assert _map_counts("map 37x53 k3 1e9") == (819, 738, 749, 17)
    assert _map_counts("map 37x53 k3 1e12")[::3] == (1803, 2)
    s, hi, lo, inside = _map_counts("map 37x53 k1 1e4")
    assert s == 0 and hi > 0 and lo > 0 and inside > 0
    assert _map_counts("map 37x53 mild")[:3] == (0, 0, 0)
    for name in ic.MAPS:          # the frame is not black where it is read, and (0, 0) is not black either (variant 12)
        assert ic.want(name)["undist"].any() and ic.raw(ic.BY_NAME[name])[0, 0].any()


def test_the_mild_map_has_all_four_border_taps():
    w = ic.want("map 37x53 mild")
    sx, sy = w["map1"][..., 0], w["map1"][..., 1]
    assert (sx == -1).any() and (sx == 53 - 1).any() and (sy == -1).any() and (sy == 37 - 1).any()
    # ... whose inner neighbour is not black, so that a border of 0 differs from a clamped one
    raw = ic.raw(ic.BY_NAME["map 37x53 mild"])
    assert raw[0].any() and raw[-1].any() and raw[:, 0].any() and raw[:, -1].any()


# ------------------------------------------------------------------------------------------------ 2. the wrong variants
def _luts(plane, limit, tiles, extend, tile_lut):
    T, tw, th, _, _ = ck.tiling(plane.shape[0], plane.shape[1], tiles)
    ext = extend(plane, T)
    luts = np.zeros((T, T, 256), np.uint8)
    for ty in range(T):
        for tx in range(T):
            hist = np.bincount(ext[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=256)
            luts[ty, tx] = tile_lut(hist, limit, tw * th)
    return luts


def _chain(case, limits=None, tile_lut=None, apply=None, extend=None, tiles=None, remap=None):
    """ck.prepare with any piece replaced: the dict of STAGES"""
    c = case
    tiles = c["tiles"] if tiles is None else tiles
    map1, map2 = ck.build_map(c["rows"], c["cols"], c["fx"], c["fy"], c["cx"], c["cy"], list(c["dist"]))
    undist = (remap or ck.remap)(ic.raw(c), map1, map2)
    g = ck.gray(undist)
    Y, Cr, Cb = ck.bgr_to_ycrcb(undist)
    T, tw, th, _, _ = ck.tiling(c["rows"], c["cols"], tiles)
    lg, ly = (limits or (lambda cg, cc, area: (ck.clip_limit(cg, area), ck.clip_limit(cc, area))))(c["clip_gray"], c["clip_color"], tw * th)
    tile_lut = tile_lut or (lambda hist, limit, area: ck.tile_lut(hist, limit, area)[0])
    apply = apply or ck.clahe_apply
    extend = extend or ck.extend
    lut_gray, lut_y = _luts(g, lg, tiles, extend, tile_lut), _luts(Y, ly, tiles, extend, tile_lut)
    return dict(lut_gray=lut_gray, lut_y=lut_y, gray_eq=apply(g, lut_gray, tw, th), bgr_eq=ck.ycrcb_to_bgr(apply(Y, lut_y, tw, th), Cr, Cb))


def _differing(got, name):
    """bytes of STAGES that differ from the checker's (a stage of another shape counts whole)"""
    w = ic.want(name)
    return sum(int((got[s] != w[s]).sum()) if got[s].shape == w[s].shape else w[s].size for s in STAGES)


def _raw_limit(clip, area):
    return min(F64(clip) * F64(area) / 256, 2147483647.0)


def _lut_general(hist, limit, area, guard=True, skip_without_batch=False, scale64=False):
    h = np.asarray(hist, np.int64).copy()
    excess = int(np.maximum(h - limit, 0).sum())
    h = np.minimum(h, limit)
    batch, res = excess // 256, excess % 256
    h += batch
    if res > 0 and not (skip_without_batch and batch == 0):
        step = max(256 // res, 1)
        i = np.arange(256)
        h += ((i % step == 0) & ((i // step < res) | (not guard))).astype(np.int64)
    if scale64:
        return ck.sat8(np.rint(np.cumsum(h).astype(F64) * (255.0 / area))).astype(np.uint8)
    return ck.sat8(np.rint(np.cumsum(h).astype(F32) * (F32(255.0) / F32(area)))).astype(np.uint8)


def _blend(plane, luts, tw, th, dtype=F32):
    """the sum ck.clahe_apply rounds, with the floating type as a parameter"""
    rows, cols = plane.shape
    T = luts.shape[0]

    def axis(n, t):
        tf = np.arange(n).astype(dtype) * (dtype(1.0) / dtype(t)) - dtype(0.5)
        fl = np.floor(tf)
        a = (tf - fl).astype(dtype)
        t1 = fl.astype(np.int64)
        return np.maximum(t1, 0), np.minimum(t1 + 1, T - 1), a, (dtype(1.0) - a).astype(dtype)
    tx1, tx2, xa, xa1 = axis(cols, tw)
    ty1, ty2, ya, ya1 = axis(rows, th)
    v = plane.astype(np.int64)
    Y1, Y2, X1, X2 = ty1[:, None], ty2[:, None], tx1[None, :], tx2[None, :]
    l11, l12, l21, l22 = (luts[a, b, v].astype(dtype) for a, b in ((Y1, X1), (Y1, X2), (Y2, X1), (Y2, X2)))
    xa, xa1, ya, ya1 = xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]
    r = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya
    assert r.dtype == dtype
    return r


def _apply_general(plane, luts, tw, th, dtype=F32, half_up=False):
    r = _blend(plane, luts, tw, th, dtype)
    return ck.sat8(np.floor(r.astype(F64) + 0.5) if half_up else np.rint(r)).astype(np.uint8)      # r + 0.5 is exact in FP64 for an FP32 r


def _extend_duplicating(plane, T):
    rows, cols = plane.shape
    _, _, _, er, ec = ck.tiling(rows, cols, T)
    yy, xx = np.arange(er), np.arange(ec)
    return plane[np.where(yy >= rows, 2 * rows - 1 - yy, yy)][:, np.where(xx >= cols, 2 * cols - 1 - xx, xx)]


def _remap_general(img, map1, map2, clamp=False, sentinel_is_origin=False):
    rows, cols = img.shape[:2]
    sx, sy, m2 = map1[..., 0].astype(np.int64), map1[..., 1].astype(np.int64), map2.astype(np.int64)
    if sentinel_is_origin:
        s = (sx == -32768) & (sy == -32768) & (m2 == 0)
        sx, sy = np.where(s, 0, sx), np.where(s, 0, sy)
    w00, w01, w10, w11 = ck.weights(m2 & 31, m2 >> 5)
    src = img.astype(np.int64)

    def p(yy, xx):
        inside = (yy >= 0) & (yy < rows) & (xx >= 0) & (xx < cols)
        px = src[np.clip(yy, 0, rows - 1), np.clip(xx, 0, cols - 1)]
        return px if clamp else px * inside[..., None]
    acc = w00[..., None] * p(sy, sx) + w01[..., None] * p(sy, sx + 1) + w10[..., None] * p(sy + 1, sx) + w11[..., None] * p(sy + 1, sx + 1)
    return ((acc + 16384) >> 15).astype(np.uint8)


def _T_from_rows(case):
    assert case["tiles"] == 0
    return max(int(case["rows"] * 32.0 / 640), 4)


VARIANTS = {
    "1 limit rounded": lambda c: _chain(c, limits=lambda cg, cc, a: tuple(max(int(np.rint(_raw_limit(x, a))), 1) for x in (cg, cc))),
    "2 limit not raised to 1": lambda c: _chain(c, limits=lambda cg, cc, a: tuple(int(_raw_limit(x, a)) for x in (cg, cc))),
    "3 plane 1 with plane 0's limit": lambda c: _chain(c, limits=lambda cg, cc, a: (ck.clip_limit(cg, a),) * 2),
    "4 spread without i / step < res": lambda c: _chain(c, tile_lut=lambda h, l, a: _lut_general(h, l, a, guard=False)),
    "5 spread skipped at batch 0": lambda c: _chain(c, tile_lut=lambda h, l, a: _lut_general(h, l, a, skip_without_batch=True)),
    "6 table scale in FP64": lambda c: _chain(c, tile_lut=lambda h, l, a: _lut_general(h, l, a, scale64=True)),
    "7 blend in FP64": lambda c: _chain(c, apply=lambda p, l, tw, th: _apply_general(p, l, tw, th, dtype=F64)),
    "8 blend rounded half-up": lambda c: _chain(c, apply=lambda p, l, tw, th: _apply_general(p, l, tw, th, half_up=True)),
    "9 edge-duplicating reflection": lambda c: _chain(c, extend=_extend_duplicating),
    "10 T from rows": lambda c: _chain(c, tiles=_T_from_rows(c)),
    "11 outside neighbour clamped": lambda c: _chain(c, remap=lambda i, a, b: _remap_general(i, a, b, clamp=True)),
    "12 sentinel as pixel (0, 0)": lambda c: _chain(c, remap=lambda i, a, b: _remap_general(i, a, b, sentinel_is_origin=True)),
}

# variant -> {case that tells it from the checker: bytes of STAGES that differ}
TELLS = {
    "1 limit rounded": {"clip 37x53 (12.8, 0.01)": 3057, "map 37x53 mild": 5445},                       # 6.999... -> 7; 3.0 140 / 256 = 1.64 -> 2
    "2 limit not raised to 1": {"clip 64x64 (0.001, 1e-300)": 24363, "geometry 16x16 default": 7426, "geometry 16x16 tiles 8": 18493},
    "3 plane 1 with plane 0's limit": {"clip 64x64 (2.0, 255.0)": 14946, "clip 64x64 (255.0, 2.0)": 14946, "clip 64x64 (256.0, 0.5)": 14932,
                                       "clip 64x64 (0.5, 256.0)": 14932},
    # at the last bins the table is saturated whatever is added, so of the constant frames only 255 at res 129 shows the missing clause
    "4 spread without i / step < res": {"constant 255 64x64 limit 127": 4032, "two levels 64x64": 992, "clip 64x64 (255.0, 2.0)": 4262},
    "5 spread skipped at batch 0": {"constant 128 64x64 limit 1": 24576, "constant teal 64x64 limit 255": 16384, "two levels 64x64": 24576},
    "6 table scale in FP64": {"geometry 16x400 tiles 8": 1147, "geometry 400x16 tiles 8": 1051},
    "7 blend in FP64": {"geometry 40x48 tiles 4": 36, "geometry 20x52 tiles 4": 20, "geometry 400x16 tiles 8": 89, "map 37x53 mild": 12,
                        "geometry 17x19 default": 1},
    "8 blend rounded half-up": {"one class per tile 64x64": 516, "geometry 64x64 tiles 4 ties": 459, "geometry 32x32 tiles 4": 246},
    "9 edge-duplicating reflection": {"geometry 17x19 default": 1129, "geometry 18x21 default": 1324, "geometry 32x37 default clips (40, 20)": 4692},
    "10 T from rows": {"geometry 50x120 default": 41333},
    "11 outside neighbour clamped": {"map 37x53 mild": 11300, "geometry 16x16 tiles 8": 6683, "geometry 400x16 tiles 8": 21589},
    "12 sentinel as pixel (0, 0)": {"map 37x53 k3 1e9": 6270, "map 37x53 k3 1e12": 8379},
}


def test_the_chain_of_this_file_with_nothing_wrong_is_the_checkers():
    for name in ("clip 37x53 (1e+12, 3.0)", "geometry 17x19 default", "map 37x53 k3 1e9", "constant teal 64x64 limit 171", "one class per tile 64x64"):
        c = ic.BY_NAME[name]
        assert _differing(_chain(c), name) == 0, name
        assert _differing(_chain(c, tile_lut=_lut_general, apply=_apply_general, remap=_remap_general), name) == 0, name


def test_the_tie_cases_hold_exact_halves_that_half_up_rounds_elsewhere():
    for name in ("one class per tile 64x64", "geometry 64x64 tiles 4 ties"):
        w = ic.want(name)
        r = _blend(w["gray"], w["lut_gray"], 16, 16)
        ties = (r - np.floor(r)) == F32(0.5)
        assert ties.sum() >= 100, (name, int(ties.sum()))
        odd_floor = ties & (np.floor(r).astype(np.int64) % 2 == 0)           # rne goes down, half-up goes up
        assert odd_floor.sum() >= 40, (name, int(odd_floor.sum()))


@pytest.mark.parametrize("variant,name", [(v, n) for v, names in TELLS.items() for n in names])
def test_a_wrong_variant_gives_other_bytes(variant, name):
    assert _differing(VARIANTS[variant](ic.BY_NAME[name]), name) == TELLS[variant][name] > 0


def test_every_variant_is_told_apart():
    assert set(TELLS) == set(VARIANTS) and all(TELLS[v] for v in VARIANTS)
