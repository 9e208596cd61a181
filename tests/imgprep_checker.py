"""Independent NumPy restatement of the image preparation specified in include/srlivo_hip.h ("image preparation of the camera stage"):
undistortion map, remap, gray, BGR <-> YCrCb and CLAHE.  Written from the specification, not from the kernels: integer arrays throughout,
np.float64 for the map, np.float32 for CLAHE's two float steps, np.rint (round half to even) for every rounding.  It is the yardstick of
tests/test_image_prep_abi.py (the map), tests/test_gpu_image_prep.py and tests/test_gpu_image_prep_envelope.py (everything else, the
latter on the case grid of tests/imgprep_cases.py); tests/test_imgprep_checker.py holds known answers for the checker itself.  NumPy evaluates every elementwise product and sum as a separate IEEE operation, so nothing here is
contracted."""
import numpy as np


def descale(x, n):
    return (x + (1 << (n - 1))) >> n          # numpy's >> on signed integers is arithmetic


def sat8(x):
    return np.clip(x, 0, 255)


def build_map(rows, cols, fx, fy, cx, cy, dist):
    """(map1 (rows, cols, 2) int16 = (sx, sy), map2 (rows, cols) uint16)"""
    k1, k2, p1, p2, k3 = (np.float64(d) for d in dist)
    fx, fy, cx, cy = np.float64(fx), np.float64(fy), np.float64(cx), np.float64(cy)
    j = np.arange(cols, dtype=np.float64)[None, :]
    i = np.arange(rows, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        x = (j - cx) / fx + np.zeros((rows, 1))
        y = (i - cy) / fy + np.zeros((1, cols))
        r2 = x * x + y * y
        kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = x * kr + (p1 * (2 * x * y) + p2 * (r2 + 2 * x * x))
        yd = y * kr + (p1 * (r2 + 2 * y * y) + p2 * (2 * x * y))
        u = fx * xd + cx
        v = fy * yd + cy
        u32, v32 = u * 32, v * 32
        bad = ~(np.isfinite(u) & np.isfinite(v)) | ~(np.abs(u32) < 2147483647.0) | ~(np.abs(v32) < 2147483647.0)
    iu = np.rint(np.where(bad, 0.0, u32)).astype(np.int64)
    iv = np.rint(np.where(bad, 0.0, v32)).astype(np.int64)
    sx = np.clip(iu >> 5, -32768, 32767)
    sy = np.clip(iv >> 5, -32768, 32767)
    m2 = (iv & 31) * 32 + (iu & 31)
    sx = np.where(bad, -32768, sx)
    sy = np.where(bad, -32768, sy)
    m2 = np.where(bad, 0, m2)
    return np.stack([sx, sy], axis=-1).astype(np.int16), m2.astype(np.uint16)


def weights(ax, ay):
    return (32 - ax) * (32 - ay) * 32, ax * (32 - ay) * 32, (32 - ax) * ay * 32, ax * ay * 32


def remap(img, map1, map2):
    """img (rows, cols, 3) uint8 -> the same shape; constant border 0"""
    rows, cols = img.shape[:2]
    src = np.zeros((rows + 2, cols + 2, 3), dtype=np.int64)          # a one-pixel frame of zeros stands for everything outside
    src[1:-1, 1:-1] = img
    sx, sy = map1[..., 0].astype(np.int64), map1[..., 1].astype(np.int64)
    m2 = map2.astype(np.int64)
    w00, w01, w10, w11 = weights(m2 & 31, m2 >> 5)

    def p(yy, xx):
        inside = (yy >= 0) & (yy < rows) & (xx >= 0) & (xx < cols)
        return src[np.where(inside, yy + 1, 0), np.where(inside, xx + 1, 0)]
    acc = w00[..., None] * p(sy, sx) + w01[..., None] * p(sy, sx + 1) + w10[..., None] * p(sy + 1, sx) + w11[..., None] * p(sy + 1, sx + 1)
    return ((acc + 16384) >> 15).astype(np.uint8)


def gray(img):
    c = img.astype(np.int64)
    return ((9798 * c[..., 0] + 19235 * c[..., 1] + 3735 * c[..., 2] + 16384) >> 15).astype(np.uint8)


def bgr_to_ycrcb(img):
    c = img.astype(np.int64)
    b, g, r = c[..., 0], c[..., 1], c[..., 2]
    Y = descale(1868 * b + 9617 * g + 4899 * r, 14)
    Cr = sat8(descale((r - Y) * 11682 + (128 << 14), 14))
    Cb = sat8(descale((b - Y) * 9241 + (128 << 14), 14))
    return Y.astype(np.uint8), Cr.astype(np.uint8), Cb.astype(np.uint8)


def ycrcb_to_bgr(Y, Cr, Cb):
    Y, Cr, Cb = Y.astype(np.int64), Cr.astype(np.int64), Cb.astype(np.int64)
    b = sat8(Y + descale((Cb - 128) * 29049, 14))
    g = sat8(Y + descale((Cb - 128) * (-5636) + (Cr - 128) * (-11698), 14))
    r = sat8(Y + descale((Cr - 128) * 22987, 14))
    return np.stack([b, g, r], axis=-1).astype(np.uint8)


def tiling(rows, cols, tiles=0):
    """(T, tw, th, ext_rows, ext_cols)"""
    T = int(tiles) if tiles else max(int(cols * 32.0 / 640), 4)
    ext_rows, ext_cols = rows, cols
    if cols % T != 0 or rows % T != 0:
        ext_cols = cols + (T - cols % T)
        ext_rows = rows + (T - rows % T)
    return T, ext_cols // T, ext_rows // T, ext_rows, ext_cols


def clip_limit(clip, area):
    return max(int(min(np.float64(clip) * np.float64(area) / 256, 2147483647.0)), 1)      # the min first: the cast stays inside int32


def tile_lut(hist, limit, area):
    """one tile: the 256-bin histogram -> (lut (256,) uint8, excess, batch, res, step)"""
    h = np.asarray(hist, dtype=np.int64).copy()
    excess = int(np.sum(np.maximum(h - limit, 0)))
    h = np.minimum(h, limit)
    batch = excess // 256
    res = excess - batch * 256
    h += batch
    step = 0
    if res > 0:
        step = max(256 // res, 1)
        i = np.arange(256)
        h += ((i % step == 0) & (i // step < res)).astype(np.int64)
    scale = np.float32(255.0) / np.float32(area)
    lut = sat8(np.rint(np.cumsum(h).astype(np.float32) * scale)).astype(np.uint8)
    return lut, excess, batch, res, step


def extend(plane, T):
    rows, cols = plane.shape
    _, _, _, er, ec = tiling(rows, cols, T)
    yy = np.arange(er)
    xx = np.arange(ec)
    yy = np.where(yy >= rows, 2 * (rows - 1) - yy, yy)
    xx = np.where(xx >= cols, 2 * (cols - 1) - xx, xx)
    return plane[yy][:, xx]


def clahe_luts(plane, clip, tiles=0):
    """(luts (T, T, 256) uint8, limit)"""
    rows, cols = plane.shape
    T, tw, th, _, _ = tiling(rows, cols, tiles)
    ext = extend(plane, T)
    area = tw * th
    limit = clip_limit(clip, area)
    luts = np.zeros((T, T, 256), dtype=np.uint8)
    for ty in range(T):
        band = ext[ty * th:(ty + 1) * th]
        for tx in range(T):
            hist = np.bincount(band[:, tx * tw:(tx + 1) * tw].ravel(), minlength=256)
            luts[ty, tx] = tile_lut(hist, limit, area)[0]
    return luts, limit


def clahe_apply(plane, luts, tw, th):
    rows, cols = plane.shape
    T = luts.shape[0]
    f32 = np.float32

    def axis(n, t):
        tf = np.arange(n).astype(f32) * (f32(1.0) / f32(t)) - f32(0.5)
        fl = np.floor(tf)
        a = (tf - fl).astype(f32)
        a1 = (f32(1.0) - a).astype(f32)
        t1 = fl.astype(np.int64)
        t2 = t1 + 1
        return np.maximum(t1, 0), np.minimum(t2, T - 1), a, a1
    tx1, tx2, xa, xa1 = axis(cols, tw)
    ty1, ty2, ya, ya1 = axis(rows, th)
    v = plane.astype(np.int64)
    Y1, Y2 = ty1[:, None], ty2[:, None]
    X1, X2 = tx1[None, :], tx2[None, :]
    l11, l12 = luts[Y1, X1, v].astype(f32), luts[Y1, X2, v].astype(f32)
    l21, l22 = luts[Y2, X1, v].astype(f32), luts[Y2, X2, v].astype(f32)
    xa, xa1, ya, ya1 = xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]
    r = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya
    assert r.dtype == np.float32
    return sat8(np.rint(r)).astype(np.uint8)


def clahe(plane, clip, tiles=0):
    T, tw, th, _, _ = tiling(plane.shape[0], plane.shape[1], tiles)
    luts, _ = clahe_luts(plane, clip, tiles)
    return clahe_apply(plane, luts, tw, th)


def prepare(raw, fx, fy, cx, cy, dist, clip_gray=3.0, clip_color=1.0, tiles=0):
    """the whole chain on raw (rows, cols, 3) uint8: a dict of every stage, both results and the info tuple
    (tiles, tile_w, tile_h, ext_rows, ext_cols, limit_gray, limit_color)"""
    rows, cols = raw.shape[:2]
    map1, map2 = build_map(rows, cols, fx, fy, cx, cy, dist)
    undist = remap(raw, map1, map2)
    g = gray(undist)
    Y, Cr, Cb = bgr_to_ycrcb(undist)
    T, tw, th, er, ec = tiling(rows, cols, tiles)
    lut_gray, limit_gray = clahe_luts(g, clip_gray, tiles)
    lut_y, limit_color = clahe_luts(Y, clip_color, tiles)
    gray_eq = clahe_apply(g, lut_gray, tw, th)
    bgr_eq = ycrcb_to_bgr(clahe_apply(Y, lut_y, tw, th), Cr, Cb)
    return dict(map1=map1, map2=map2, undist=undist, gray=g, y=Y, cr=Cr, cb=Cb, lut_gray=lut_gray, lut_y=lut_y, gray_eq=gray_eq, bgr_eq=bgr_eq,
                info=(T, tw, th, er, ec, limit_gray, limit_color))
