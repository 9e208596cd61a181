"""tests/jpeg_checker.py, the independent restatement the library's JPEG decode is compared with, is bytewise libjpeg-turbo's decode at its
defaults (JDCT_ISLOW, fancy upsampling), through Pillow's encoder and decoder: the whole grid of tests/jpeg_cases.py -- six sizes x
4:4:4 / 4:2:2 / 4:2:0 / gray x quality 35 / 90 with optimised Huffman tables / 100, uniform noise at quality 100, quantisation tables of
all 255 and restart intervals of one MCU, two MCUs and one MCU row.  No case is left out and no tolerance applies.  Without Pillow the
checker is still compared with the committed fixtures (tests/golden/golden_jpeg.npz: Pillow's streams and Pillow's pixels)."""
import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_checker as ck


def test_the_checker_equals_the_committed_pillow_decodes():
    golden = jc.load_golden()
    assert sorted(golden) == sorted(jc.golden_names()) and len(golden) >= 12
    for name, (data, bgr) in golden.items():
        got = ck.decode(data)
        assert got.shape == bgr.shape and np.array_equal(got, bgr), name


def test_the_committed_cases_cover_every_rule():
    golden = jc.load_golden()
    hdrs = {name: ck.parse(data) for name, (data, _) in golden.items()}
    assert {(h["cols"], h["rows"]) for h in hdrs.values()} == set(jc.SIZES)
    assert {(h["components"], h["h"][0], h["v"][0]) for h in hdrs.values()} == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    r = {name: h["restart"] for name, h in hdrs.items()}
    assert r["37x43_420_r1"] == 1 and r["37x43_422_r2"] == 2 and r["40x48_420_rrow"] == hdrs["40x48_420_rrow"]["mcus_per_row"] and r["33x17_444_r1"] == 1
    assert all(v == 255 for t in hdrs["37x43_422_t255"]["qt"].values() for v in t)


@pytest.mark.parametrize("sampling", jc.SAMPLINGS)
def test_the_checker_is_bytewise_pillows_decode_on_the_whole_grid(sampling):
    pytest.importorskip("PIL")
    cases = [c for c in jc.grid() if c[3] == sampling]
    assert len(cases) == len(jc.SIZES) * 8
    restarts = set()
    for case in cases:
        data = jc.make(case)
        ref = jc.pillow_decode(data)
        got = ck.decode(data)
        assert got.shape == ref.shape == (case[2], case[1], 3), case[0]
        assert np.array_equal(got, ref), (case[0], int(np.sum(got != ref)))
        hdr = ck.parse(data)
        if hdr["restart"]:
            restarts.add(case[0].rsplit("_", 1)[1])
    assert restarts == {"r1", "r2", "rrow"}                 # the encoder did write the intervals that were asked for


def test_the_fixture_is_what_its_generator_writes():
    pytest.importorskip("PIL")
    golden = jc.load_golden()
    by_name = {c[0]: c for c in jc.grid()}
    for name in jc.golden_names():
        data = jc.make(by_name[name])
        # (another libjpeg-turbo may choose other bytes for the same image; the pixels of ITS decode of ITS stream still equal the checker's)
        if data == golden[name][0]:
            assert np.array_equal(jc.pillow_decode(data), golden[name][1]), name
