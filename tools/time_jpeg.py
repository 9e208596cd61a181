"""A compressed camera frame at the shipped 1280 x 1024, 4:2:0, quality 90: where the time of srl_jpeg_decode / srl_image_prepare_jpeg goes,
beside the raw path (srl_image_prepare of the same frame given decoded: the code that was there before) in the same process.
50 calls behind 5 warm-up calls, medians.

  host entropy decode   srl_jpeg_entropy_decode alone into a prepared block (ms): the sequential part, on one core
  srl_jpeg_decode       HIP events (torch.cuda.Event on the context's device) and the host clock around the synchronous call: parse,
                        entropy decode into staging, ONE upload (tables + coefficients), k_jpeg_idct, k_jpeg_color, the wait
  upload + kernels      the call minus the entropy decode measured beside it (us); the two kernels alone: run this script under
                        `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_jpeg.py` in a run of its own and read k_jpeg_idct /
                        k_jpeg_color from the statistics (tracing slows the host: the whole-call figures of such a run are not to quote)
  srl_image_prepare_jpeg / srl_image_prepare of the decoded frame / where Pillow is importable its decode (libjpeg-turbo with SIMD)

The frame comes from Pillow's encoder; without Pillow there is no frame and the script says so."""
import ctypes as C
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
try:
    from PIL import Image
except ImportError:
    print("tools/time_jpeg.py: Pillow is needed to encode the synthetic frame")
    sys.exit(2)
import torch  # noqa: E402
import sr_livo_amd as srl  # noqa: E402
from sr_livo_amd import capi  # noqa: E402

ROWS, COLS = 1024, 1280
WARMUP, CALLS = 5, 50

rng = np.random.default_rng(7)
yy, xx = np.mgrid[0:ROWS, 0:COLS]
rgb = np.stack([xx * 255 // (COLS - 1), yy * 255 // (ROWS - 1), (xx + yy) * 255 // (ROWS + COLS - 2)], axis=-1) + rng.integers(-12, 13, size=(ROWS, COLS, 3))
rgb = np.ascontiguousarray(np.clip(rgb, 0, 255).astype(np.uint8))
buf = io.BytesIO()
Image.fromarray(rgb, "RGB").save(buf, format="JPEG", quality=90, subsampling="4:2:0")
jpeg = np.frombuffer(buf.getvalue(), np.uint8)
opts = capi.default_image_prep_opts(rows=ROWS, cols=COLS, fx=863.4, fy=863.4, cx=640.6, cy=518.3, dist=[-0.1080, 0.1050, -1.2872e-4, 5.7923e-5, -0.0222])


def timed(name, fn, device=True):
    for _ in range(WARMUP):
        fn()
    ev, wall = [], []
    for _ in range(CALLS):
        if device:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
        w0 = time.perf_counter()
        if device:
            a.record()
        fn()
        if device:
            b.record()
            b.synchronize()
        wall.append((time.perf_counter() - w0) * 1e6)
        ev.append(a.elapsed_time(b) * 1e3 if device else wall[-1])
    ev, wall = np.array(ev), np.array(wall)
    print("%-62s %s median %9.1f us (p10 %9.1f, p90 %9.1f); host wall median %9.1f us; calls = %d" % (
        name, "HIP events" if device else "host clock", np.median(ev), np.percentile(ev, 10), np.percentile(ev, 90), np.median(wall), len(ev)))
    return float(np.median(ev))


lib = capi.load_library()
info = capi.jpeg_parse(jpeg)
coef = np.zeros((info.total_blocks, 64), np.int16)
qt = np.zeros((3, 64), np.uint16)
print("frame %d x %d, 4:2:0, quality 90: %d bytes compressed, %d bytes raw; %d blocks = %d bytes of coefficients uploaded" % (
    COLS, ROWS, jpeg.size, rgb.size, info.total_blocks, info.total_blocks * 128 + 384))
entropy = timed("srl_jpeg_entropy_decode (host, one core)", lambda: lib.srl_jpeg_entropy_decode(capi._ptr(jpeg), jpeg.size, C.byref(info), capi._ptr(coef),
                                                                                                len(coef), capi._ptr(qt)), device=False)

ctx = srl.Context(0)
ctx.color_map_create()
prep = srl.ImagePrep(ctx, opts)
ctx.jpeg_decode(jpeg)
frame = ctx.jpeg_download(ROWS, COLS)
pil = np.asarray(Image.open(io.BytesIO(jpeg.tobytes())))
assert np.array_equal(frame, pil[:, :, ::-1]), "the device's frame is not Pillow's"
decode = timed("srl_jpeg_decode (whole call)", lambda: ctx.jpeg_decode(jpeg))
print("%-62s %9.1f us (the call minus the entropy decode beside it)" % ("  upload + k_jpeg_idct + k_jpeg_color + launches + wait", decode - entropy))
prep_jpeg = timed("srl_image_prepare_jpeg (whole call)", lambda: prep.prepare_jpeg(jpeg))
prep_raw = timed("srl_image_prepare of the decoded frame (the raw path)", lambda: prep.prepare(frame))


def pillow_decode():
    im = Image.open(io.BytesIO(jpeg.tobytes()))
    im.load()


pillow = timed("Pillow decode (libjpeg-turbo, host)", pillow_decode, device=False)
print("entropy decode %.2f ms; JPEG path %.1f us against host decode + raw path %.1f + %.1f = %.1f us -> the JPEG path is %s by %.1f us" % (
    entropy * 1e-3, prep_jpeg, pillow, prep_raw, pillow + prep_raw, "BELOW" if prep_jpeg < pillow + prep_raw else "ABOVE", abs(prep_jpeg - pillow - prep_raw)))
ctx.close()
