"""The case grid of the image preparer's envelope, shared by tests/test_imgprep_cases.py (CPU: every case does what it is there for, and
every wrong variant of the rule is told apart by one of them) and tests/test_gpu_image_prep_envelope.py (GPU: the device equals the
checker bytewise on every case).  Pure NumPy: nothing here needs the library.

A case is a dict: name, group ("clip", "excess", "geometry", "map"), rows, cols, tiles (0 = the reference's rule), clip_gray, clip_color,
dist (k1 k2 p1 p2 k3), fx, fy, cx, cy, image -- the raw BGR frame as a (rows, cols, 3) uint8 view with a row stride of 3 cols + 13 bytes
into a buffer whose padding is 0xA5, read-only -- and identity: True where zero distortion and an integral principal point make the
undistorted frame the raw one.  The constant frames also carry expect = (excess, batch, res, step), what every tile of both planes
reaches.  CASES lists them, BY_NAME finds one, want(name) is the checker's chain on it, computed once and read-only.
Sizes are the smallest at which the rule can go wrong: nothing above 128 x 128 but the two strips of 16 x 400 and 400 x 16.
"""
import functools
import itertools

import numpy as np

import imgprep_checker as ck

MILD = (0.2, 0.05, 0.002, -0.003, 0.01)          # pincushion: the corners come from outside the image
ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)


def strided(img):
    """img (rows, cols, 3) uint8 -> the same pixels with a row stride of 3 cols + 13 bytes and 0xA5 between the rows; read-only"""
    rows, cols = img.shape[:2]
    stride = 3 * cols + 13
    buf = np.full(rows * stride, 0xA5, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, shape=(rows, cols, 3), strides=(stride, 3, 1))
    view[...] = img
    view.setflags(write=False)
    buf.setflags(write=False)
    return view


@functools.lru_cache(maxsize=None)
def image(rows, cols, seed):
    """the noisy content: gradients with +-12 noise, saturated blocks that overflow the clip limit, all 216 pixels of
    {0, 1, 127, 128, 254, 255}^3 (rows cols >= 216); strided, read-only"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols]
    img = np.stack([(xx * 255 // max(cols - 1, 1)), (yy * 255 // max(rows - 1, 1)), ((xx + yy) * 255 // (rows + cols - 2))], axis=-1).astype(np.int64)
    img += rng.integers(-12, 13, size=img.shape)
    for _ in range(max(4, rows * cols // 1500)):          # saturated blocks: their bins overflow the clip limit
        r, c = rng.integers(0, rows), rng.integers(0, cols)
        h, w = rng.integers(2, max(3, rows // 4)), rng.integers(2, max(3, cols // 4))
        img[r:r + h, c:c + w] = rng.choice([0, 255], size=3) if rng.random() < 0.5 else rng.choice([0, 255])
    img = np.clip(img, 0, 255).astype(np.uint8)
    combos = np.array(list(itertools.product((0, 1, 127, 128, 254, 255), repeat=3)), np.uint8)
    at = rng.choice(rows * cols, size=len(combos), replace=False)
    img.reshape(-1, 3)[at] = combos
    return strided(img)


def constant(rows, cols, bgr):
    return strided(np.broadcast_to(np.asarray(bgr, np.uint8), (rows, cols, 3)))


def two_level(rows, cols):
    """0 / 255 at one-pixel pitch in both directions, every channel alike: each tile holds the two bins half and half"""
    yy, xx = np.mgrid[0:rows, 0:cols]
    return strided(np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[..., None], 3, axis=-1))


TILE_VALUES = ((0, 255, 37, 218), (255, 0, 200, 60), (90, 230, 0, 255), (180, 20, 255, 0))      # neighbours at least 77 apart


def one_value_per_tile(side=64, T=4):
    """tile (tx, ty) holds TILE_VALUES[ty][tx] in every channel: each table is a step, and the blend crosses 0 beside 255"""
    t = side // T
    plane = np.kron(np.array(TILE_VALUES, np.uint8), np.ones((t, t), np.uint8))
    return strided(np.repeat(plane[..., None], 3, axis=-1))


def one_class_per_tile(side=64, T=4, seed=5):
    """tile (tx, ty) is uniform noise in 0 ... min(40 (1 + tx + ty), 255), every channel alike (gray = Y = the value).  With 16 x 16 tiles
    the blend weights are multiples of 1 / 32, exact in FP32, so sums land on exact halves: the round-half-even of the blend decides bytes"""
    rng = np.random.default_rng(seed)
    t = side // T
    plane = np.zeros((side, side), np.uint8)
    for ty in range(T):
        for tx in range(T):
            plane[ty * t:(ty + 1) * t, tx * t:(tx + 1) * t] = rng.integers(0, min(40 * (1 + tx + ty), 255) + 1, size=(t, t))
    return strided(np.repeat(plane[..., None], 3, axis=-1))


def case(name, group, img, tiles=0, clips=(3.0, 1.0), dist=MILD, identity=False, expect=None):
    rows, cols = img.shape[:2]
    if identity:          # zero distortion and an integral principal point: the map is the identity with no fraction
        dist, cx, cy = ZERO, float(cols // 2), float(rows // 2)
    else:
        cx, cy = cols / 2 - 0.37, rows / 2 + 0.21
    focal = max(rows, cols)          # from the longer side, so that MILD stays mild on the 400 x 16 strip
    c = dict(name=name, group=group, rows=rows, cols=cols, tiles=int(tiles), clip_gray=float(clips[0]), clip_color=float(clips[1]),
             dist=tuple(float(d) for d in dist), fx=0.9 * focal, fy=0.92 * focal, cx=cx, cy=cy, image=img, identity=bool(identity))
    if expect is not None:
        c["expect"] = tuple(expect)
    return c


# ------------------------------------------------------------------------------------------------ a. clips
CLIPS_256 = [(0.001, 1e-300), (0.999999, 1.0), (2.0, 255.0), (255.0, 2.0), (256.0, 0.5), (0.5, 256.0), (1e6, 40.0), (1e300, 1e12)]
CLIPS_140 = [(256 / 140 * 7, 0.01), (1e12, 3.0)]
SWAPPED_PAIRS = [("clip 64x64 (2.0, 255.0)", "clip 64x64 (255.0, 2.0)"), ("clip 64x64 (256.0, 0.5)", "clip 64x64 (0.5, 256.0)")]


def _clip_cases():
    out = [case("clip 64x64 (%r, %r)" % cl, "clip", image(64, 64, 41), tiles=4, clips=cl) for cl in CLIPS_256]
    return out + [case("clip 37x53 (%.4g, %r)" % cl, "clip", image(37, 53, 42), clips=cl) for cl in CLIPS_140]


# ------------------------------------------------------------------------------------------------ b. controlled excess
COLOURS = {"0": (0, 0, 0), "128": (128, 128, 128), "255": (255, 255, 255), "teal": (200, 90, 15)}
# 64 x 64, tiles = 4: area 256, limit == (int)clip, every tile one bin of 256.  limit -> (excess, batch, res, step)
LIMITS_256 = {1: (255, 0, 255, 1), 127: (129, 0, 129, 1), 128: (128, 0, 128, 2), 171: (85, 0, 85, 3), 253: (3, 0, 3, 85), 254: (2, 0, 2, 128),
              255: (1, 0, 1, 256), 256: (0, 0, 0, 0)}
# 128 x 128, tiles = 4: area 1024, limit = 4 clip.  clip -> (excess, batch, res, step)
CLIPS_1024 = {0.25: (1023, 3, 255, 1), 63.75: (769, 3, 1, 256), 64.0: (768, 3, 0, 0)}
TWO_LEVEL_CLIP = 100.0          # area 256: limit 100 cuts both bins of 128 -> excess 56, batch 0, res 56, step 4


def _excess_cases():
    out = []
    for cname, bgr in COLOURS.items():
        for limit, expect in LIMITS_256.items():
            out.append(case("constant %s 64x64 limit %d" % (cname, limit), "excess", constant(64, 64, bgr), tiles=4, clips=(limit, limit), identity=True,
                             expect=expect))
        for clip, expect in CLIPS_1024.items():
            out.append(case("constant %s 128x128 clip %g" % (cname, clip), "excess", constant(128, 128, bgr), tiles=4, clips=(clip, clip), identity=True,
                             expect=expect))
    out.append(case("two levels 64x64", "excess", two_level(64, 64), tiles=4, clips=(TWO_LEVEL_CLIP, TWO_LEVEL_CLIP), identity=True, expect=(56, 0, 56, 4)))
    out.append(case("one value per tile 64x64", "excess", one_value_per_tile(), tiles=4, identity=True))
    out.append(case("one class per tile 64x64", "excess", one_class_per_tile(), tiles=4, identity=True))
    return out


# ------------------------------------------------------------------------------------------------ c. geometry
# name -> (rows, cols, tiles, (T, tile_w, tile_h, ext_rows, ext_cols))
GEOMETRY = {
    "geometry 16x16 default": (16, 16, 0, (4, 4, 4, 16, 16)),           # area 16: the limit raised from 0 to 1, a quarter of a wave per tile
    "geometry 16x16 tiles 8": (16, 16, 8, (8, 2, 2, 16, 16)),           # tile 2 x 2
    "geometry 17x19 default": (17, 19, 0, (4, 5, 5, 20, 20)),           # 323 pixels = 3 mod 4; both dimensions extended
    "geometry 18x21 default": (18, 21, 0, (4, 6, 5, 20, 24)),           # 378 pixels = 2 mod 4
    "geometry 32x32 tiles 4": (32, 32, 4, (4, 8, 8, 32, 32)),           # area exactly a wave
    "geometry 20x52 tiles 4": (20, 52, 4, (4, 13, 5, 20, 52)),          # area 65: one pixel into the second round
    "geometry 32x37 default": (32, 37, 0, (4, 10, 9, 36, 40)),          # rows divide: they grow by a whole T, the reflection runs T rows deep
    "geometry 16x400 tiles 8": (16, 400, 8, (8, 50, 2, 16, 400)),       # tile 50 x 2, area 100: 255 / 100 is where FP32 and FP64 tables part
    "geometry 400x16 tiles 8": (400, 16, 8, (8, 2, 50, 400, 16)),       # tile 2 x 50
    "geometry 50x120 default": (50, 120, 0, (6, 21, 9, 54, 126)),       # T = 6 from cols where rows would give 4
    "geometry 40x48 tiles 4": (40, 48, 4, (4, 12, 10, 40, 48)),         # weights k / 12 and k / 10: FP32 and FP64 blends part here
}


def _geometry_cases():
    out = [case(name, "geometry", image(r, c, 43), tiles=t) for name, (r, c, t, _) in GEOMETRY.items()]
    # at the default clips a tile of 90 pixels has limit 1, which sees only WHICH values a tile holds: the four reflected rows repeat
    # values of their own tile and change nothing.  The same frame at limits 14 and 7 counts them.
    out.append(case("geometry 32x37 default clips (40, 20)", "geometry", image(32, 37, 43), clips=(40.0, 20.0)))
    return out + [case("geometry 64x64 tiles 4 ties", "geometry", one_class_per_tile(), tiles=4)]      # the content of (b) under the mild map


# ------------------------------------------------------------------------------------------------ d. maps
MAPS = {"map 37x53 k3 1e9": (0, 0, 0, 0, 1e9), "map 37x53 k3 1e12": (0, 0, 0, 0, 1e12), "map 37x53 k1 1e4": (1e4, 0, 0, 0, 0), "map 37x53 mild": MILD}


def _map_cases():
    return [case(name, "map", image(37, 53, 44), dist=d) for name, d in MAPS.items()]


CASES = _clip_cases() + _excess_cases() + _geometry_cases() + _map_cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
NAMES = [c["name"] for c in CASES]


def raw(case):
    """the case's frame as a contiguous (rows, cols, 3) array"""
    return np.ascontiguousarray(case["image"])


def freeze(w):
    for v in w.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return w


def chain(c, frame=None):
    """the checker's chain with the case's options, on the case's frame or on another (rows, cols, 3) frame; read-only"""
    frame = raw(c) if frame is None else np.ascontiguousarray(frame)
    return freeze(ck.prepare(frame, c["fx"], c["fy"], c["cx"], c["cy"], list(c["dist"]), c["clip_gray"], c["clip_color"], c["tiles"]))


@functools.lru_cache(maxsize=None)
def want(name):
    """the checker's chain on the case of that name, computed once and shared; read-only"""
    return chain(BY_NAME[name])
