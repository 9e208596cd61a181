"""The JPEG test grid: images, encoder settings and names.  The streams come from Pillow's encoder (tests/golden/make_golden_jpeg.py writes
them into tests/golden/golden_jpeg.npz with Pillow's decoded pixels; tests/test_jpeg_checker_reference.py encodes the whole grid afresh)."""
import io
import os

import numpy as np

SIZES = [(1, 1), (8, 9), (16, 16), (33, 17), (37, 43), (40, 48)]      # (cols, rows)
SAMPLINGS = ["444", "422", "420", "gray"]
QUALITIES = [35, 90, 100]                                              # 90: with optimised Huffman tables
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_jpeg.npz")


def image(cols, rows, seed, noise=False):
    """(rows, cols, 3) uint8 R G B: smooth ramps with some texture, or uniform noise"""
    rng = np.random.default_rng(seed)
    if noise:
        return rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    base = np.stack([40 + 5.0 * x + 1.5 * y, 220 - 3.0 * x + 2.0 * y, 128 + 90 * np.sin(0.7 * x) * np.cos(0.45 * y)], axis=2)
    return np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)


def encode(rgb, sampling, quality=90, optimize=False, restart_blocks=0, restart_rows=0, qtables=None, progressive=False):
    """Pillow's encoder; sampling "444" / "422" / "420" / "gray" """
    from PIL import Image
    kw = dict(format="JPEG", optimize=optimize, progressive=progressive)
    if qtables is None:
        kw["quality"] = quality                            # (with tables of its own Pillow would scale them by it)
    if restart_blocks:
        kw["restart_marker_blocks"] = restart_blocks
    if restart_rows:
        kw["restart_marker_rows"] = restart_rows
    if qtables is not None:
        kw["qtables"] = qtables
    if sampling == "gray":
        img = Image.fromarray(np.ascontiguousarray(rgb[:, :, 1]), "L")
    else:
        img = Image.fromarray(np.ascontiguousarray(rgb), "RGB")
        kw["subsampling"] = {"444": "4:4:4", "422": "4:2:2", "420": "4:2:0"}[sampling]
    out = io.BytesIO()
    img.save(out, **kw)
    return out.getvalue()


def pillow_decode(data):
    """(rows, cols, 3) uint8 B G R, libjpeg-turbo's defaults; a gray stream replicated as toCvCopy(..., BGR8) does"""
    from PIL import Image
    img = Image.open(io.BytesIO(data))
    img.load()
    a = np.asarray(img)
    return np.repeat(a[:, :, None], 3, axis=2) if a.ndim == 2 else np.ascontiguousarray(a[:, :, ::-1])


def grid():
    """(name, cols, rows, sampling, keywords of encode, noise) for the whole grid"""
    out = []
    for si, (cols, rows) in enumerate(SIZES):
        for sj, sampling in enumerate(SAMPLINGS):
            for q in QUALITIES:
                out.append((f"{cols}x{rows}_{sampling}_q{q}", cols, rows, sampling, dict(quality=q, optimize=q == 90), False))
            out.append((f"{cols}x{rows}_{sampling}_noise", cols, rows, sampling, dict(quality=100), True))
            out.append((f"{cols}x{rows}_{sampling}_t255", cols, rows, sampling, dict(qtables=[[255] * 64] * 2), False))
            out.append((f"{cols}x{rows}_{sampling}_r1", cols, rows, sampling, dict(quality=90, restart_blocks=1), False))
            out.append((f"{cols}x{rows}_{sampling}_r2", cols, rows, sampling, dict(quality=90, restart_blocks=2), False))
            out.append((f"{cols}x{rows}_{sampling}_rrow", cols, rows, sampling, dict(quality=90, restart_rows=1), False))
    return out


def golden_names():
    """the part of the grid that is committed: every size with every sampling once (the quality rotating), and the 37 x 43 and 40 x 48
    frames also with noise, the all-255 tables and the three restart intervals for one sampling each"""
    names = []
    for si, (cols, rows) in enumerate(SIZES):
        for sj, sampling in enumerate(SAMPLINGS):
            names.append(f"{cols}x{rows}_{sampling}_q{QUALITIES[(si + sj) % 3]}")
    names += ["37x43_420_noise", "37x43_422_t255", "37x43_420_r1", "37x43_422_r2", "40x48_420_rrow", "40x48_gray_r2", "33x17_444_r1", "40x48_444_noise"]
    return names


def make(case):
    name, cols, rows, sampling, kw, noise = case
    seed = sum(name.encode()) * 7919 + cols * 131 + rows
    return encode(image(cols, rows, seed, noise), sampling, **kw)


def load_golden():
    """{name: (jpeg bytes, Pillow's (rows, cols, 3) B G R)}"""
    z = np.load(GOLDEN, allow_pickle=False)
    return {k[5:]: (z[k].tobytes(), z["bgr_" + k[5:]]) for k in z.files if k.startswith("jpeg_")}
