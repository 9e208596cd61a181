"""The restatement of cloudProcessing::livoxHandler (tests/livox_checker.py) pinned to the reference's own function, bit for bit.

Which form: the reference's translation unit ITSELF.  src/cloudProcessing.cpp is compiled where it lies, together with
tests/livox_ref_reader.cpp, into the test's temporary directory (tests/livox_reader.py); tests/stub_livox puts a CustomMsg with real
points, point_num and header (and the two members more the file's other handlers need to compile) ahead of oracle/ref_shim.  The loop,
std::sort with time_list and point3D are the reference's; nothing is written out statement by statement.  Neither the binary nor
anything of the reference is committed; the tests skip where the reference tree, oracle/_ref/libref_path.so or g++ is absent.

Compared: every queued record (raw_point, point, relative_time, timestamp, alpha_time) and last_end_time, bitwise, on every case of
tests/livox_cases.py except the named tie cases -- std::sort is not stable, so among equal offsets the reference's order is its
library's own, and this project specifies message order there (livox_checker.decode).  Two further cases have no valid point: upstream
that is .back() of an empty vector, there is nothing to compare with, and the call is left out (livox_cases.UNDEFINED_UPSTREAM)."""
import os

import numpy as np
import pytest

import livox_cases as lc
import livox_checker as lk
import livox_reader as lr

pytestmark = pytest.mark.skipif(not lr.available(), reason="needs the reference tree, oracle/_ref/libref_path.so and g++")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_livox.npz")


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    return lr.build(tmp_path_factory.mktemp("livox_ref_reader"))


def _check(case):
    return lk.decode(case["points"], case["stamp"], case["n_scans"], lk.time_unit_scale(case["unit"]), case["blind"], case["pfn"])


def test_the_excluded_cases_are_the_tie_cases_and_the_undefined_ones():
    names = [c["name"] for c in lc.all_cases()]
    assert len(set(names)) == len(names)
    for c in lc.all_cases():
        w = _check(c)
        assert w["has_ties"] == c["ties"] == (c["name"] in lc.TIE_CASES), c["name"]
        assert (w["valid"] == 0) == (c["name"] in lc.UNDEFINED_UPSTREAM), c["name"]
        assert np.all(np.abs(np.nan_to_num(np.stack([c["points"]["x"], c["points"]["y"], c["points"]["z"]]), nan=0.0, posinf=0.0, neginf=0.0)) < 2.0 ** 31)
    assert {c["name"] for c in lc.reference_cases()} == set(names) - set(lc.TIE_CASES)


def test_every_tie_free_case_equals_the_reference_bitwise(reader):
    compared = 0
    for c in lc.reference_cases():
        w = _check(c)
        if c["name"] in lc.UNDEFINED_UPSTREAM:
            assert w["valid"] == 0 and w["appended"] == 0 and np.isnan(w["last_end_time"])
            continue
        rows, last_end = lr.run(reader, c)
        assert len(rows) == w["appended"], c["name"]
        assert lr.records_of(rows).tobytes() == w["records"].tobytes(), c["name"]
        assert rows[:, 3:6].tobytes() == rows[:, 0:3].tobytes(), c["name"]                 # point = raw_point (cloudProcessing.cpp:143)
        assert not rows[:, 8].any(), c["name"]                                              # alpha_time = 0.0
        assert np.float64(last_end).tobytes() == np.float64(w["last_end_time"]).tobytes(), c["name"]
        compared += 1
    assert compared == len(lc.reference_cases()) - len(lc.UNDEFINED_UPSTREAM) >= 30


def test_the_golden_file_holds_what_the_reader_gives(reader):
    g = np.load(GOLDEN)
    assert sorted(str(n) for n in g["names"]) == sorted(c["name"] for c in lc.reference_cases() if c["name"] not in lc.UNDEFINED_UPSTREAM)
    for c in lc.reference_cases():
        if c["name"] in lc.UNDEFINED_UPSTREAM:
            continue
        rows, last_end = lr.run(reader, c)
        rec = lr.records_of(rows)
        assert int(g[c["name"] + "/count"]) == len(rec)
        assert np.float64(g[c["name"] + "/last_end_time"]).tobytes() == np.float64(last_end).tobytes()
        if len(rec) <= lr.GOLDEN_FULL_RECORDS:
            assert g[c["name"] + "/records"].tobytes() == rec.tobytes(), c["name"]
        else:
            assert np.array_equal(g[c["name"] + "/sha256"], lr.digest(rec)), c["name"]
