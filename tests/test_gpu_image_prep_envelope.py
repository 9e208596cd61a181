"""The image preparer on the device over its clip, tile, content and map envelope: every case of tests/imgprep_cases.py through
srl_image_prepare, a few through srl_image_prepare_resized, preparers following one another on one context, and repeats.

Every comparison is BYTEWISE with tests/imgprep_checker.py: every stage (undist, gray, Y / CrCb, both sets of look-up tables), both
results and the info record.  No tolerance: integer arithmetic and uncontracted FP32 are exact on both sides.  What each case is there
for, and which mistake of the rule it would show, is proved on the CPU by tests/test_imgprep_cases.py."""
import numpy as np
import pytest

import imgprep_cases as ic
import resize_checker as rk
import sr_livo_amd as srl
from imgprep_device import all_bytes, check_all, same
from sr_livo_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = srl.Context(0)
    yield c
    c.close()


def _opts(c):
    return capi.default_image_prep_opts(rows=c["rows"], cols=c["cols"], fx=c["fx"], fy=c["fy"], cx=c["cx"], cy=c["cy"], dist=list(c["dist"]),
                                        clip_gray=c["clip_gray"], clip_color=c["clip_color"], tiles=c["tiles"])


# ------------------------------------------------------------------------------------------------ 1. every case
@pytest.mark.parametrize("name", ic.NAMES)
def test_every_stage_of_every_case_equals_the_checker(ctx, name):
    c = ic.BY_NAME[name]
    prep = srl.ImagePrep(ctx, _opts(c))
    try:
        info = prep.prepare(c["image"])
        check_all(prep, info, ic.want(name))
    finally:
        prep.close()


# ------------------------------------------------------------------------------------------------ 2. behind the resize
RESIZED = [
    ("clip 64x64 (2.0, 255.0)", (128, 128), "exact half"),
    ("clip 64x64 (2.0, 255.0)", (91, 77), "general rule, down"),
    ("constant teal 64x64 limit 171", (40, 50), "general rule, up: a constant frame stays constant"),
    ("geometry 16x400 tiles 8", (23, 301), "rows down, columns up"),
]


@pytest.mark.parametrize("name,src,what", RESIZED, ids=["%s from %dx%d" % (n, s[0], s[1]) for n, s, _ in RESIZED])
def test_cases_behind_the_resize_equal_the_checkers_chain_on_the_checkers_resize(ctx, name, src, what):
    c = ic.BY_NAME[name]
    source = ic.constant(src[0], src[1], ic.raw(c)[0, 0]) if name.startswith("constant") else ic.image(src[0], src[1], 45)
    resized = rk.resize(np.ascontiguousarray(source), c["rows"], c["cols"])
    assert rk.is_exact_half(src, c["rows"], c["cols"]) == what.startswith("exact half")
    if name.startswith("constant"):
        assert np.array_equal(resized, ic.raw(c))
    want = ic.chain(c, resized)
    prep = srl.ImagePrep(ctx, _opts(c))
    try:
        info = prep.prepare_resized(source)
        same("resized", prep.download_resized(), resized)
        check_all(prep, info, want)
    finally:
        prep.close()


# ------------------------------------------------------------------------------------------------ 3. one preparer after another
def test_preparers_in_turn_on_one_context_keep_nothing_of_the_one_before(ctx):
    # small T, large T, small T again: sizes, tiles, limits and table blocks all change (limits (6, 1), (54, 30), (14, 7))
    wide = ic.case("lifetime 96x128 tiles 16", "geometry", ic.image(96, 128, 46), tiles=16, clips=(288.0, 160.0))
    turns = [ic.BY_NAME["clip 37x53 (12.8, 0.01)"], wide, ic.BY_NAME["geometry 32x37 default clips (40, 20)"]]
    seen = []
    for c in turns:
        want = ic.chain(c)
        prep = srl.ImagePrep(ctx, _opts(c))
        try:
            info = prep.prepare(c["image"])
            check_all(prep, info, want)
            seen.append(info.as_tuple()[:7])
        finally:
            prep.close()
    assert [s[0] for s in seen] == [4, 16, 4] and [s[5:] for s in seen] == [(6, 1), (54, 30), (14, 7)]


# ------------------------------------------------------------------------------------------------ 4. repeats
LARGEST = ["constant teal 128x128 clip 0.25", "geometry 16x400 tiles 8", "geometry 400x16 tiles 8"]      # the three largest frame sizes of the grid


@pytest.mark.parametrize("name", LARGEST)
def test_a_second_run_gives_the_same_bytes(ctx, name):
    c = ic.BY_NAME[name]
    assert c["rows"] * c["cols"] >= sorted({k["rows"] * k["cols"] for k in ic.CASES})[-2]
    prep = srl.ImagePrep(ctx, _opts(c))
    try:
        info = prep.prepare(c["image"])
        first = all_bytes(prep, info.tiles)
        again = prep.prepare(c["image"])
        assert again.as_tuple() == info.as_tuple() and all_bytes(prep, again.tiles) == first
        check_all(prep, again, ic.want(name))
    finally:
        prep.close()
