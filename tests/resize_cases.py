"""The shapes and source images shared by tests/test_resize_checker.py (CPU) and tests/test_gpu_image_resize.py (GPU): the smallest at
which lanes, tails and borders of the resize can go wrong.  Images are built like `image` of tests/imgprep_cases.py (gradients,
noise, saturated blocks, all 216 pixels of {0, 1, 127, 128, 254, 255}^3 where they fit), handed over with a row stride of 3 cols + 13
bytes and a padding of 0xA5, read-only."""
import functools
import itertools

import numpy as np

# (source rows, cols), (destination rows, cols), what it exercises
SHAPES = [
    ((74, 106), (37, 53), "exact half, odd sizes, tail of the four-pixels-per-lane pass"),
    ((61, 91), (37, 53), "non-integer down"),
    ((19, 27), (37, 53), "up, clamped last taps"),
    ((1, 1), (37, 53), "degenerate source"),
    ((192, 340), (96, 170), "more than one wave per row"),
    ((193, 341), (96, 170), "not the shortcut: general rule at a ratio near 2"),
]


@functools.lru_cache(maxsize=None)
def image(rows, cols, seed):
    """(rows, cols, 3) uint8 view with a stride of 3 cols + 13 bytes into a buffer whose padding is 0xA5; read-only"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols]
    img = np.stack([(xx * 255 // max(cols - 1, 1)), (yy * 255 // max(rows - 1, 1)), ((xx + yy) * 255 // max(rows + cols - 2, 1))], axis=-1).astype(np.int64)
    img += rng.integers(-12, 13, size=img.shape)
    if rows >= 4 and cols >= 4:
        for _ in range(max(4, rows * cols // 1500)):          # saturated blocks: steps of 255 between neighbours
            r, c = rng.integers(0, rows), rng.integers(0, cols)
            h, w = rng.integers(2, max(3, rows // 4)), rng.integers(2, max(3, cols // 4))
            img[r:r + h, c:c + w] = rng.choice([0, 255], size=3) if rng.random() < 0.5 else rng.choice([0, 255])
    img = np.clip(img, 0, 255).astype(np.uint8)
    combos = np.array(list(itertools.product((0, 1, 127, 128, 254, 255), repeat=3)), np.uint8)
    if rows * cols >= len(combos):
        at = rng.choice(rows * cols, size=len(combos), replace=False)
        img.reshape(-1, 3)[at] = combos
    else:
        img.reshape(-1, 3)[:] = combos[rng.choice(len(combos), size=rows * cols, replace=False)]
    stride = 3 * cols + 13
    buf = np.full(rows * stride, 0xA5, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, shape=(rows, cols, 3), strides=(stride, 3, 1))
    view[...] = img
    view.setflags(write=False)
    buf.setflags(write=False)
    return view
