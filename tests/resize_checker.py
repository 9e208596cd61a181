"""Independent NumPy restatement of the resize specified in include/srlivo_hip.h (stage (r) of "image preparation of the camera stage"):
the tables of srl_image_resize_build_tables and the pixel rule of srl_image_prepare_resized.  Written from the specification, not from
the C: np.float64 for the sample position, np.float32 for the fraction and the two coefficient products, np.rint (round half to even),
int64 arrays for the pixel rule.  NumPy evaluates every elementwise product and sum as a separate IEEE operation, so nothing here is
contracted.  It is the yardstick of tests/test_resize_checker.py (the tables, and the checker against FP64 bilinear interpolation) and of
tests/test_gpu_image_resize.py (the pixels)."""
import numpy as np


def build_tables(src_len, dst_len):
    """(ofs (dst_len,) int32, coef (dst_len, 2) int16)"""
    f32 = np.float32
    d = np.arange(dst_len, dtype=np.float64)
    scale = np.float64(src_len) / np.float64(dst_len)
    f = ((d + 0.5) * scale - 0.5).astype(f32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(f32)).astype(f32)
    low = s < 0
    s = np.where(low, 0, s)
    f = np.where(low, f32(0), f)
    high = s >= src_len - 1
    s = np.where(high, src_len - 1, s)
    f = np.where(high, f32(0), f).astype(f32)
    c0 = np.rint((f32(1.0) - f) * f32(2048.0))
    c1 = np.rint(f * f32(2048.0))
    assert c0.dtype == np.float32 and c1.dtype == np.float32
    return s.astype(np.int32), np.stack([c0, c1], axis=-1).astype(np.int16)


def sample_positions(src_len, dst_len):
    """where the tables sample, in FP64: (s (dst_len,) int64, fraction (dst_len,) float64) with the two clamps of the specification"""
    d = np.arange(dst_len, dtype=np.float64)
    pos = (d + 0.5) * (np.float64(src_len) / np.float64(dst_len)) - 0.5
    s = np.floor(pos).astype(np.int64)
    f = pos - s
    low = s < 0
    s, f = np.where(low, 0, s), np.where(low, 0.0, f)
    high = s >= src_len - 1
    return np.where(high, src_len - 1, s), np.where(high, 0.0, f)


def is_exact_half(src_shape, dst_rows, dst_cols):
    return src_shape[0] == 2 * dst_rows and src_shape[1] == 2 * dst_cols


def box_mean(img):
    """img (2 r, 2 c, 3) uint8 -> (r, c, 3): (s00 + s01 + s10 + s11 + 2) >> 2"""
    s = img.astype(np.int64)
    return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def linear(img, dst_rows, dst_cols):
    """the general rule, whatever the ratio"""
    src_rows, src_cols = img.shape[:2]
    ox, cx = build_tables(src_cols, dst_cols)
    oy, cy = build_tables(src_rows, dst_rows)
    ox, oy = ox.astype(np.int64), oy.astype(np.int64)
    x1 = np.minimum(ox + 1, src_cols - 1)
    y1 = np.minimum(oy + 1, src_rows - 1)
    s = img.astype(np.int64)
    a0, a1 = cx[:, 0].astype(np.int64)[None, :, None], cx[:, 1].astype(np.int64)[None, :, None]
    h = s[:, ox] * a0 + s[:, x1] * a1                      # (src_rows, dst_cols, 3)
    b0, b1 = cy[:, 0].astype(np.int64)[:, None, None], cy[:, 1].astype(np.int64)[:, None, None]
    h0, h1 = h[oy], h[y1]
    assert int(h.max(initial=0)) >> 4 <= 32767 and int((b0 * (h0 >> 4)).max(initial=0)) < 2 ** 31
    out = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2
    return np.minimum(out, 255).astype(np.uint8)


def resize(img, dst_rows, dst_cols):
    """img (src_rows, src_cols, 3) uint8 -> (dst_rows, dst_cols, 3) uint8 as srl_image_prepare_resized leaves it (equal sizes: the image)"""
    img = np.asarray(img)
    if img.shape[0] == dst_rows and img.shape[1] == dst_cols:
        return np.ascontiguousarray(img)
    if is_exact_half(img.shape, dst_rows, dst_cols):
        return box_mean(img)
    return linear(img, dst_rows, dst_cols)


def bilinear_fp64(img, dst_rows, dst_cols):
    """FP64 bilinear interpolation at the same sample positions, unrounded: (dst_rows, dst_cols, 3) float64"""
    src_rows, src_cols = img.shape[:2]
    ox, fx = sample_positions(src_cols, dst_cols)
    oy, fy = sample_positions(src_rows, dst_rows)
    x1 = np.minimum(ox + 1, src_cols - 1)
    y1 = np.minimum(oy + 1, src_rows - 1)
    s = img.astype(np.float64)
    fx = fx[None, :, None]
    fy = fy[:, None, None]
    h = s[:, ox] * (1.0 - fx) + s[:, x1] * fx
    return h[oy] * (1.0 - fy) + h[y1] * fy
