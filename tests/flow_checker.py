"""Sequential restatement of the optical-flow step of the camera stage (reference src/lkpyramid.cpp): the 8-bit pyramid with its 21-pixel
REFLECT_101 borders (pyrDown: separable [1 4 6 4 1], integer sums, (s + 128) >> 8), the Scharr derivative per level (int16 (Ix, Iy),
zero border) and LKOpticalFlowKernel::trackImage's per-point track for cn = 1, err = nullptr.  Integer parts are NumPy integer arrays;
every float statement is an np.float32 (or, for the stop test, float64) scalar operation in the reference's order, and every float
accumulation is a strictly sequential chain in the order of the reference's SSE loops (np.add.accumulate is sequential):

  A-matrix   four chains k = 0..3 over the exact products of x = 4 g + k, y ascending then g = 0..4, a fifth chain over x = 20;
             result = tail + (((c0 + c1) + c2) + c3)
  b-vector   eight chains (component, i = 0..3) over float(int32(It_x D_x + It_{x+4} D_{x+4})), x = 8 g + i, y ascending then g = 0..1;
             a tail chain over x = 16..20 in (y, x) order; ib = tail + ((c_i0 + c_i2) + (c_i1 + c_i3))

pyrDown, copyMakeBorder, cvRound (round to nearest even) and cvFloor are OpenCV library behaviour restated here from its documentation;
tests/stub_opencv_lk restates them a second time, independently, for the reference's own compiled statements (tests/flow_reader.py).

The scenes are generated with integers only (seeded byte noise, integer box blurs, integer shifts and integer-weight blends), so they are
the same bytes on every machine.  The device path (sr_livo_amd/csrc/srl_flow.hip) must equal this file bit for bit."""
import zlib

import numpy as np

WIN = 21
F32 = np.float32
HALF = F32(10.0)                   # (winSize - 1) * 0.5f
W_BITS = 14
FLT_SCALE = F32(1.0) / F32(1 << 20)
FLT_EPSILON = F32(1.1920929e-07)
INT_MIN, INT_MAX = -2**31, 2**31 - 1

# exit classes of one (point, level) visit
START_OUTSIDE, MIN_EIG, WALKED_OUT, EPSILON, OSCILLATION, MAX_COUNT, GUARD = "start_outside", "min_eig", "walked_out", "epsilon", "oscillation", "max_count", "guard"
EXIT_CLASSES = (START_OUTSIDE, MIN_EIG, WALKED_OUT, EPSILON, OSCILLATION, MAX_COUNT)


class Opts:
    def __init__(self, win=21, max_level=3, max_count=10, epsilon=0.05, min_eig_threshold=1e-4):
        self.win, self.max_level, self.max_count, self.epsilon, self.min_eig_threshold = win, max_level, max_count, epsilon, min_eig_threshold


# ---------------------------------------------------------------------------------------------------------------- pyramid and derivative
def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101)"""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def _reflect_index(lo, hi, n):
    return np.array([reflect101(p, n) for p in range(lo, hi)], dtype=np.int64)


def pyr_down(img):
    """cv::pyrDown of an 8-bit single-channel image to ((w + 1) / 2, (h + 1) / 2)"""
    img = np.asarray(img, dtype=np.uint8)
    h, w = img.shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    K = (1, 4, 6, 4, 1)
    src = img.astype(np.int32)
    rowsum = np.zeros((h, dw), dtype=np.int32)
    for k in range(5):
        cx = np.array([reflect101(2 * x + k - 2, w) for x in range(dw)], dtype=np.int64)
        rowsum += K[k] * src[:, cx]
    out = np.zeros((dh, dw), dtype=np.int32)
    for k in range(5):
        ry = np.array([reflect101(2 * y + k - 2, h) for y in range(dh)], dtype=np.int64)
        out += K[k] * rowsum[ry, :]
    return ((out + 128) >> 8).astype(np.uint8)


def pad_reflect(img, b=WIN):
    """cv::copyMakeBorder(img, b, b, b, b, BORDER_REFLECT_101)"""
    h, w = img.shape
    return np.ascontiguousarray(img[_reflect_index(-b, h + b, h)][:, _reflect_index(-b, w + b, w)])


def scharr(img):
    """calcSharrDeriv (lkpyramid.cpp:57-154): (rows, cols, 2) int16, (Ix, Iy).  |values| <= 4080: nothing wraps int16."""
    img = np.asarray(img, dtype=np.uint8)
    h, w = img.shape
    s = img.astype(np.int32)
    up, down = s[_reflect_index(-1, h - 1, h)], s[_reflect_index(1, h + 1, h)]
    t0 = (up + down) * 3 + s * 10
    t1 = down - up
    xl, xr = _reflect_index(-1, w - 1, w), _reflect_index(1, w + 1, w)
    ix = t0[:, xr] - t0[:, xl]
    iy = (t1[:, xr] + t1[:, xl]) * 3 + t1 * 10
    assert max(np.abs(ix).max(), np.abs(iy).max()) <= 4080
    return np.stack([ix, iy], axis=-1).astype(np.int16)


def pad_zero(deriv, b=WIN):
    h, w, _ = deriv.shape
    out = np.zeros((h + 2 * b, w + 2 * b, 2), dtype=np.int16)
    out[b:b + h, b:b + w] = deriv
    return out


def num_levels(rows, cols, max_level, win=WIN):
    """opencvBuildOpticalFlowPyramid's return value (lkpyramid.cpp:609-619)"""
    w, h = cols, rows
    for level in range(max_level + 1):
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= win or h <= win:
            return level
    return max_level


class Pyramid:
    """levels 0 ... L of one image: padded images (uint8) and padded derivatives (int16, interleaved)"""

    def __init__(self, gray, max_level):
        gray = np.ascontiguousarray(gray, dtype=np.uint8)
        self.L = num_levels(gray.shape[0], gray.shape[1], max_level)
        self.sizes, self.image, self.deriv = [], [], []
        level = gray
        for k in range(self.L + 1):
            if k:
                level = pyr_down(level)
            self.sizes.append(level.shape)
            self.image.append(pad_reflect(level))
            self.deriv.append(pad_zero(scharr(level)))

    def crcs(self):
        return (np.array([zlib.crc32(a.tobytes()) for a in self.image], dtype=np.uint32),
                np.array([zlib.crc32(a.tobytes()) for a in self.deriv], dtype=np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------- the track
def cv_floor(v):
    """cvFloor of a float; None where the value does not fit int32 (cvtss2si gives INT_MIN there, and the comparison that follows
    turns it into INT_MIN or INT_MAX: outside every admitted range either way)"""
    v = float(v)
    if not np.isfinite(v):
        return None
    f = int(np.floor(v))
    return f if INT_MIN <= f <= INT_MAX else None


def _weights(a, b):
    one, s = F32(1.0), F32(1 << W_BITS)
    iw00 = int(np.rint((one - a) * (one - b) * s))
    iw01 = int(np.rint(a * (one - b) * s))
    iw10 = int(np.rint((one - a) * b * s))
    return iw00, iw01, iw10, (1 << W_BITS) - iw00 - iw01 - iw10


def _chain(addends):
    """0.f + a0 + a1 + ... strictly left to right in float32"""
    a = np.concatenate([np.zeros(1, np.float32), np.asarray(addends, dtype=np.float32).ravel()])
    return np.add.accumulate(a, dtype=np.float32)[-1]


def _bilinear(win22, w, shift):
    iw00, iw01, iw10, iw11 = w
    v = win22.astype(np.int64)
    s = v[:-1, :-1] * iw00 + v[:-1, 1:] * iw01 + v[1:, :-1] * iw10 + v[1:, 1:] * iw11
    return (s + (1 << (shift - 1))) >> shift


def _a_sum(prod):
    """prod: 21 x 21 exact integer products"""
    p = prod.astype(np.float32)                      # |values| < 2^24: exact
    c = [_chain(p[:, k:20:4]) for k in range(4)]     # row-major: y ascending, then g
    return _chain(p[:, 20]) + (((c[0] + c[1]) + c[2]) + c[3])


def _b_sum(It, D):
    prod = It * D                                    # int64, |values| < 2^26
    pair = (prod[:, :16].reshape(21, 2, 8)[:, :, :4] + prod[:, :16].reshape(21, 2, 8)[:, :, 4:]).astype(np.float32)   # [y, g, i]: x = 8 g + i
    c = [_chain(pair[:, :, i]) for i in range(4)]
    tail = _chain(prod[:, 16:21].astype(np.float32))
    return tail + ((c[0] + c[2]) + (c[1] + c[3]))


def guarded(x, y):
    """the contract departure: a coordinate that is not finite, or whose window corner does not fit int32"""
    for v in (x, y):
        if not np.isfinite(v) or cv_floor(F32(v) - HALF) is None:
            return True
    return False


def track_point(prev_pyr, cur_pyr, L, pt, opts, trace=None):
    """one point through levels L ... 0; returns (next_x, next_y, status) with np.float32 coordinates.  trace (a list) receives
    (level, exit class, details) per visited level."""
    px0, py0 = F32(pt[0]), F32(pt[1])
    if guarded(px0, py0):
        if trace is not None:
            trace.append((-1, GUARD, {}))
        return px0, py0, 0
    status = 1
    nx = ny = F32(0)
    min_eig_thr = F32(opts.min_eig_threshold)
    for level in range(L, -1, -1):
        rows, cols = prev_pyr.sizes[level]
        I, dI, J = prev_pyr.image[level], prev_pyr.deriv[level], cur_pyr.image[level]
        sc = F32(1.0 / (1 << level))
        ppx, ppy = px0 * sc, py0 * sc
        if level == L:
            nx, ny = ppx, ppy
        else:
            nx, ny = nx * F32(2.0), ny * F32(2.0)
        ppx, ppy = ppx - HALF, ppy - HALF
        ix, iy = cv_floor(ppx), cv_floor(ppy)
        if ix is None or iy is None or ix < -WIN or ix >= cols or iy < -WIN or iy >= rows:
            if level == 0:
                status = 0
            if trace is not None:
                trace.append((level, START_OUTSIDE, {}))
            continue
        info = {"ix": ix, "iy": iy, "cols": cols, "rows": rows}
        a, b = ppx - F32(ix), ppy - F32(iy)
        w = _weights(a, b)
        Iw = _bilinear(I[iy + WIN:iy + WIN + 22, ix + WIN:ix + WIN + 22], w, W_BITS - 5)
        Dx = _bilinear(dI[iy + WIN:iy + WIN + 22, ix + WIN:ix + WIN + 22, 0], w, W_BITS)
        Dy = _bilinear(dI[iy + WIN:iy + WIN + 22, ix + WIN:ix + WIN + 22, 1], w, W_BITS)
        A11, A12, A22 = _a_sum(Dx * Dx) * FLT_SCALE, _a_sum(Dx * Dy) * FLT_SCALE, _a_sum(Dy * Dy) * FLT_SCALE
        D = A11 * A22 - A12 * A12
        min_eig = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + F32(4.0) * A12 * A12)) / F32(2 * WIN * WIN)
        if min_eig < min_eig_thr or D < FLT_EPSILON:
            if level == 0:
                status = 0
            if trace is not None:
                trace.append((level, MIN_EIG, info))
            continue
        D = F32(1.0) / D
        tx, ty = nx - HALF, ny - HALF
        pdx = pdy = F32(0)
        why = MAX_COUNT
        for j in range(opts.max_count):
            jx, jy = cv_floor(tx), cv_floor(ty)
            if jx is None or jy is None or jx < -WIN or jx >= cols or jy < -WIN or jy >= rows:
                if level == 0:
                    status = 0
                why = WALKED_OUT
                break
            a, b = tx - F32(jx), ty - F32(jy)
            w = _weights(a, b)
            It = _bilinear(J[jy + WIN:jy + WIN + 22, jx + WIN:jx + WIN + 22], w, W_BITS - 5) - Iw
            b1, b2 = _b_sum(It, Dx) * FLT_SCALE, _b_sum(It, Dy) * FLT_SCALE
            dx, dy = (A12 * b2 - A22 * b1) * D, (A12 * b1 - A11 * b2) * D
            tx, ty = tx + dx, ty + dy
            nx, ny = tx + HALF, ty + HALF
            if float(dx) * float(dx) + float(dy) * float(dy) <= opts.epsilon:
                why = EPSILON
                break
            if j > 0 and float(np.abs(dx + pdx)) < 0.01 and float(np.abs(dy + pdy)) < 0.01:
                info = dict(info, delta=(dx, dy), before=(nx, ny))
                nx, ny = nx - dx * F32(0.5), ny - dy * F32(0.5)
                why = OSCILLATION
                break
            pdx, pdy = dx, dy
        if trace is not None:
            trace.append((level, why, info))
    return nx, ny, status


class Tracker:
    """LKOpticalFlowKernel::trackImage (lkpyramid.cpp:755-795) over a sequence of images"""

    def __init__(self, opts=None):
        self.opts = opts or Opts()
        assert self.opts.win == WIN
        self.max_level = self.opts.max_level
        self.prev = None
        self.cur = None                      # the set the swap left behind (the image before the previous one)
        self.shape = None

    def track_image(self, gray, prev_xy, trace=None):
        """returns (next_xy float32 (n, 2), status uint8 (n,) or None on the first image, number tracked)"""
        gray = np.ascontiguousarray(gray, dtype=np.uint8)
        if self.shape is not None and gray.shape != self.shape:
            raise ValueError("image size differs from the tracker's first image")
        self.shape = gray.shape
        pyr = Pyramid(gray, self.max_level)
        self.max_level = pyr.L
        prev_xy = np.ascontiguousarray(prev_xy, dtype=np.float32).reshape(-1, 2)
        if self.prev is None:
            self.prev = pyr
            return prev_xy.copy(), None, 0
        nxt = np.zeros_like(prev_xy)
        status = np.zeros(len(prev_xy), dtype=np.uint8)
        with np.errstate(all="ignore"):
            for i, pt in enumerate(prev_xy):
                tr = None if trace is None else []
                nxt[i, 0], nxt[i, 1], status[i] = track_point(self.prev, pyr, pyr.L, pt, self.opts, tr)
                if trace is not None:
                    trace.append(tr)
        self.cur, self.prev = self.prev, pyr
        return nxt, status, int(status.sum())


def exit_counts(trace):
    """how often every exit class occurred over the (point, level) visits of a trace"""
    out = {k: 0 for k in EXIT_CLASSES + (GUARD,)}
    for tr in trace:
        for _, why, _ in tr:
            out[why] += 1
    return out


def admission_edges(trace):
    """admitted visits at the extreme window corners: ix == -21, ix == cols - 1, iy == -21, iy == rows - 1"""
    out = {"ix_min": 0, "ix_max": 0, "iy_min": 0, "iy_max": 0}
    for tr in trace:
        for _, why, info in tr:
            if "ix" in info:
                out["ix_min"] += info["ix"] == -WIN
                out["ix_max"] += info["ix"] == info["cols"] - 1
                out["iy_min"] += info["iy"] == -WIN
                out["iy_max"] += info["iy"] == info["rows"] - 1
    return out


# --------------------------------------------------------------------------------------------------------------------------- the scenes
def box_blur(a, k):
    """k x k integer box mean of an integer array (valid region), rounded to nearest"""
    a = a.astype(np.int64)
    c = np.cumsum(np.cumsum(np.pad(a, ((1, 0), (1, 0))), axis=0), axis=1)
    s = c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]
    return (s + k * k // 2) // (k * k)


def texture(seed, rows, cols, margin=24, blurs=(5, 3), gain=3):
    """a smooth random texture of (rows + 2 margin) x (cols + 2 margin) bytes"""
    extra = sum(k - 1 for k in blurs)
    a = np.random.RandomState(seed).randint(0, 256, (rows + 2 * margin + extra, cols + 2 * margin + extra)).astype(np.int64)
    for k in blurs:
        a = box_blur(a, k)
    a = (a - 128) * gain + 128                        # the blurs flatten the noise: stretch it again
    return np.clip(a, 0, 255).astype(np.uint8)


def crop(tex, rows, cols, dy, dx, margin=24, sub=(0, 0)):
    """the rows x cols view of a texture displaced by (dy, dx) whole pixels plus sub = (sy, sx) quarter pixels (integer-weight blend)"""
    y0, x0 = margin + dy, margin + dx
    t = tex.astype(np.int64)
    sy, sx = sub
    p00 = t[y0:y0 + rows, x0:x0 + cols]
    p01 = t[y0:y0 + rows, x0 + 1:x0 + cols + 1]
    p10 = t[y0 + 1:y0 + rows + 1, x0:x0 + cols]
    p11 = t[y0 + 1:y0 + rows + 1, x0 + 1:x0 + cols + 1]
    v = (p00 * (4 - sy) * (4 - sx) + p01 * (4 - sy) * sx + p10 * sy * (4 - sx) + p11 * sy * sx + 8) // 16
    return np.ascontiguousarray(v.astype(np.uint8))


def grid_points(seed, rows, cols, n, lo=-0.0, spread=1.0):
    """n float32 points inside the image, on sixteenths of a pixel (seeded integers only)"""
    rs = np.random.RandomState(seed)
    x = rs.randint(int(lo * 16), int((cols - 1) * 16 * spread) + 1, n)
    y = rs.randint(int(lo * 16), int((rows - 1) * 16 * spread) + 1, n)
    return (np.stack([x, y], axis=1).astype(np.float32) / np.float32(16.0)).astype(np.float32)


def scene(name):
    """(images, prev_xy, Opts): a sequence of gray images and the points tracked through it (the same points at every call)"""
    if name in ("shift_160x120", "shift_203x157", "shift_233x185"):
        cols, rows = (int(v) for v in name.split("_")[1].split("x"))
        tex = texture(11 + cols, rows, cols)
        imgs = [crop(tex, rows, cols, 0, 0), crop(tex, rows, cols, 1, 2), crop(tex, rows, cols, 3, 1, sub=(2, 1))]
        return imgs, grid_points(5 + rows, rows, cols, 96), Opts()
    if name == "edges_160x120":
        # window corners on the first and last admitted column and row, starts outside, and points near the rim that walk out
        rows, cols = 120, 160
        tex = texture(77, rows, cols)
        imgs = [crop(tex, rows, cols, 0, 0), crop(tex, rows, cols, 2, -3)]
        xs = [-11.0, -10.75, -11.0625, cols + 9.0, cols + 9.9375, cols + 10.0, 80.0, 80.0, 80.0, 80.0, -11.0, cols + 9.5, -40.0, 400.0, 3.0, cols - 2.0]
        ys = [60.0, 60.0, 60.0, 60.0, 60.0, 60.0, -11.0, -11.0625, rows + 9.5, rows + 10.0, -11.0, rows + 9.5, 50.0, 50.0, 2.0, rows - 1.5]
        return imgs, np.stack([xs, ys], axis=1).astype(np.float32), Opts()
    if name == "flat_far_160x120":
        # a flat part (minEig rejection) and a shift larger than the window on the textured part (max_count exhausted, walks out of range)
        rows, cols = 120, 160
        tex = texture(203, rows, cols, gain=4)
        a, b = crop(tex, rows, cols, 0, 0), crop(tex, rows, cols, 0, 19)
        a[:, :60] = 90
        b[:, :60] = 90
        pts = np.concatenate([grid_points(1, rows, 50, 12), grid_points(3, rows, 90, 36) + np.float32([65.0, 0.0])]).astype(np.float32)
        return [a, b], pts, Opts()
    if name == "gain_160x120":
        # the second image has twice the contrast of the first: every Gauss-Newton step overshoots to the other side of the answer, so
        # the update alternates in sign (the oscillation rule and its half step) or runs out of steps
        rows, cols = 120, 160
        tex = texture(1, rows, cols, gain=1)
        a, b = crop(tex, rows, cols, 0, 0), crop(tex, rows, cols, 0, 2, sub=(1, 3))
        b = np.clip((b.astype(np.int64) - 128) * 2 + 128, 0, 255).astype(np.uint8)
        return [a, b], grid_points(3, rows, cols, 64), Opts()
    if name == "lowered_60x44":
        # max_level = 3 is lowered to 1 by the size rule
        rows, cols = 44, 60
        tex = texture(9, rows, cols)
        return [crop(tex, rows, cols, 0, 0), crop(tex, rows, cols, 1, 1), crop(tex, rows, cols, 2, 1)], grid_points(4, rows, cols, 40), Opts()
    raise KeyError(name)


SCENES = ("shift_160x120", "shift_203x157", "shift_233x185", "edges_160x120", "flat_far_160x120", "gain_160x120", "lowered_60x44")


def run_scene(name, trace=None):
    """every call of the scene through a Tracker: list of (next_xy, status, n_tracked, Pyramid of the image given)"""
    imgs, pts, opts = scene(name)
    tr = Tracker(opts)
    out = []
    for im in imgs:
        t = None if trace is None else []
        nxt, status, nt = tr.track_image(im, pts, t)
        if trace is not None and status is not None:
            trace.extend(t)
        out.append((nxt, status, nt, tr.prev))
    return out
