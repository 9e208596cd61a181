"""The bound behind the 32-bit form of the device's IDCT (sr_livo_amd/csrc/srl_jpeg.hip, k_jpeg_idct<false>), recomputed from the checker's
own 1-D pass: run on linear forms instead of numbers it yields, for every value the pass computes, that value's coefficients on the eight
inputs.  g is the largest single |coefficient| over all of them, gout over the eight results.  With L1 the block's sum of |coef x table|:
  pass 1: |intermediate| <= g L1 + 2^10;   |ws| <= gout (its column's L1) / 2^11 + 1, so one row of ws sums to <= gout L1 / 2^11 + 8;
  pass 2: |intermediate| <= g (gout L1 / 2^11 + 8) + 2^17.
The kernel's limit must keep that below 2^31, and the constants its comment states must be these."""
import os
import re

import numpy as np

import jpeg_checker as ck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEN = []


class Form:
    """a linear form of the pass's eight inputs; every one ever made is recorded"""

    def __init__(self, v):
        self.v = np.array(v, dtype=object)
        SEEN.append(self.v)

    def __add__(self, o):
        return Form(self.v + (o.v if isinstance(o, Form) else 0))      # (the rounding constant is accounted for separately)

    def __sub__(self, o):
        return Form(self.v - o.v)

    def __mul__(self, k):
        return Form(self.v * k)

    def __rshift__(self, n):
        return self


def _gains():
    SEEN.clear()
    out = ck._pass([Form([int(i == k) for i in range(8)]) for k in range(8)], 11)
    g = max(int(max(abs(x) for x in v)) for v in SEEN)
    gout = max(int(max(abs(x) for x in o.v)) for o in out)
    return g, gout


def test_the_limit_of_the_32_bit_idct_follows_from_the_pass():
    g, gout = _gains()
    text = open(os.path.join(ROOT, "sr_livo_amd", "csrc", "srl_jpeg.hip")).read()
    limit = int(re.search(r"#define SRL_JPEG_L1_INT32 (\d+)", text).group(1))
    assert (g, gout) == (int(re.search(r"g = (\d+)", text).group(1)), int(re.search(r"gout = (\d+)", text).group(1)))
    worst = lambda l1: g * (-(-gout * l1 // 2048) + 8) + 2 ** 17
    assert g * limit + 2 ** 10 < 2 ** 31 and worst(limit) < 2 ** 31
    assert worst(limit) == int(re.search(r"that is ([\d ]+) < 2\^31", text).group(1).replace(" ", ""))
    # the limit is not needlessly small: a tenth more would no longer be covered by this bound
    assert worst(limit * 11 // 10) >= 2 ** 31
    # frames of valid pixels stay below it: an orthonormal 8 x 8 DCT of samples in -128 ... 127 has an L2 norm of at most 8 x 128 and so
    # an L1 norm of at most 8 x 1024 = 8192, and a quantiser moves each coefficient by at most half its table entry
    assert 8192 + 64 * 20 // 2 < limit


def test_the_64_bit_form_cannot_overflow():
    """|coef x table| <= 32767 x 255: the crude bound of pass 1 (every input at that size) stays far inside int64, and its results
    inside the int libjpeg keeps them in"""
    g, _ = _gains()
    SEEN.clear()
    ck._pass([Form([int(i == k) for i in range(8)]) for k in range(8)], 11)
    s = max(int(sum(abs(x) for x in v)) for v in SEEN)          # largest sum of |coefficients|: the gain on inputs of one size
    d = 32767 * 255
    assert s * d + 2 ** 10 < 2 ** 41 and (s * d + 2 ** 10) >> 11 < 2 ** 30
    assert s * ((s * d + 2 ** 10) >> 11) + 2 ** 17 < 2 ** 63
