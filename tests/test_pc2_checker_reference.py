"""The restatement of the three PointCloud2 handlers (tests/pc2_checker.py) pinned to the reference's own functions, bit for bit.

Which form: the reference's translation unit ITSELF.  src/cloudProcessing.cpp is compiled where it lies, together with
tests/pc2_ref_reader.cpp, into the test's temporary directory (tests/pc2_reader.py); tests/stub_pc2 puts a PointCloud2 with real bytes
and a declared pcl::fromROSMsg ahead of oracle/ref_shim, and the reader's three explicit specialisations copy the named fields into the
reference's point structs -- the test's stand-in for PCL.  cloudProcessing::process, the handlers' loops, std::sort with time_list* and
point3D are the reference's; nothing is written out statement by statement.  One cloudProcessing object lives across the messages of a
case, so last_end_time carries as it does in the node.  Neither the binary nor anything of the reference is committed; the tests skip
where the reference tree, oracle/_ref/libref_path.so or g++ is absent.

Compared per message: every queued record (raw_point, point, relative_time, timestamp, alpha_time), last_end_time and
isPointTimeEnable() --
  bitwise and in order on every case of tests/pc2_cases.py without two equal sort keys;
  as a multiset on the tie cases with point_filter_num 1 whose every point passes the last_end_time test (std::sort is not stable: among
  equal keys the reference's order is its library's own, and this project specifies message order there); that covers the multi-ring
  yaw messages, whose ring-first points all tie at relative_time 0;
  not at all on the remaining tie cases, which are held to the checker alone, and on the refused cases, for which the reference has no
  defined behaviour (an index out of bounds, std::sort under < with a NaN)."""
import os

import numpy as np
import pytest

import pc2_cases as pc
import pc2_checker as pk
import pc2_reader as pr

needs_reference = pytest.mark.skipif(not pr.available(), reason="needs the reference tree, oracle/_ref/libref_path.so and g++")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_pc2.npz")


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    return pr.build(tmp_path_factory.mktemp("pc2_ref_reader"))


def _same(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def _as_multiset(records):
    """sorted by relative_time, then by bytes"""
    r = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, 5)
    return sorted((float(row[3]), row.tobytes()) for row in r)


def test_the_cases_left_out_of_order_exact_pinning_are_exactly_the_named_tie_cases():
    names = [c["name"] for c in pc.all_cases()]
    assert len(set(names)) == len(names)
    ties, multiset = set(), set()
    for c in pc.all_cases():
        ws = pk.decode_case(c)
        assert all(w["status"] == "ok" for w in ws), c["name"]
        if any(w["has_ties"] for w in ws):
            ties.add(c["name"])
            if c["pfn"] == 1 and all(w["all_pass"] for w in ws):
                multiset.add(c["name"])
    assert ties == set(pc.TIE_CASES) == {c["name"] for c in pc.all_cases() if c["ties"]}
    assert multiset == set(pc.MULTISET_CASES)
    assert {c["name"] for c in pc.exact_cases()} == set(names) - ties and len(pc.exact_cases()) >= 24
    # every multi-ring yaw message ties at relative_time 0: order-exact pinning of the yaw branch rests on the single-ring messages
    exact_yaw = [c["name"] for c in pc.exact_cases() if pk.decode_case(c)[0]["given"] == 0]
    assert len(exact_yaw) >= 8 and all(len(np.unique(m["points"]["ring"])) == 1 for n in exact_yaw for m in pc.case_by_name(n)["msgs"])
    assert {"yaw_16_rings", "yaw_duplicate_of_first"} <= multiset
    assert all(pk.decode_case(c)[0]["status"] == "refused" for c in pc.refused_cases())


@needs_reference
def test_every_tie_free_case_equals_the_reference_bitwise(reader):
    compared = 0
    for c in pc.exact_cases():
        for k, (w, (rows, last_end, given)) in enumerate(zip(pk.decode_case(c), pr.run(reader, c))):
            where = (c["name"], k)
            assert len(rows) == w["appended"], where
            assert pr.records_of(rows).tobytes() == w["records"].tobytes(), where
            assert rows[:, 3:6].tobytes() == rows[:, 0:3].tobytes(), where                     # point = raw_point
            assert not rows[:, 8].any(), where                                                  # alpha_time = 0.0
            if w["points"] > 0:
                assert _same(last_end, w["last_end_time"]) and given == w["given"], where
        compared += 1
    assert compared == len(pc.exact_cases()) >= 24


@needs_reference
def test_tie_cases_with_every_point_kept_equal_the_reference_as_a_multiset(reader):
    assert len(pc.multiset_cases()) == len(pc.MULTISET_CASES)
    for c in pc.multiset_cases():
        for k, (w, (rows, last_end, given)) in enumerate(zip(pk.decode_case(c), pr.run(reader, c))):
            where = (c["name"], k)
            assert len(rows) == w["appended"], where
            assert _as_multiset(pr.records_of(rows)) == _as_multiset(w["records"]), where
            assert np.array_equal(pr.records_of(rows)[:, 3], w["records"][:, 3]), where         # the keys themselves are in the same order
            assert _same(last_end, w["last_end_time"]) and given == w["given"], where


@needs_reference
def test_the_golden_file_holds_what_the_reader_gives(reader):
    g = np.load(GOLDEN)
    assert sorted(str(n) for n in g["names"]) == sorted(c["name"] for c in pc.exact_cases() + pc.multiset_cases())
    for c in pc.exact_cases() + pc.multiset_cases():
        for k, (rows, last_end, given) in enumerate(pr.run(reader, c)):
            key = f"{c['name']}/{k}"
            rec = pr.records_of(rows)
            if c["name"] in pc.MULTISET_CASES:
                rec = np.array([np.frombuffer(b, dtype=np.float64) for _, b in _as_multiset(rec)]).reshape(-1, 5)
            assert int(g[key + "/count"]) == len(rec), key
            if c["msgs"][k]["layout"].width * c["msgs"][k]["layout"].height > 0:
                assert _same(g[key + "/last_end_time"], last_end) and int(g[key + "/given"]) == given, key
            if len(rec) <= pr.GOLDEN_FULL_RECORDS:
                assert g[key + "/records"].tobytes() == rec.tobytes(), key
            else:
                assert np.array_equal(g[key + "/sha256"], pr.digest(rec)), key
