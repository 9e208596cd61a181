"""tests/flow_checker.py pinned to the reference's own compiled statements, bit for bit, and tests/golden/golden_flow.npz pinned to
the reader that produced it.

tests/flow_reader.py compiles the reference's src/lkpyramid.cpp where it lies against tests/stub_opencv_lk into the test's temporary
directory and drives its LKOpticalFlowKernel::trackImage through tests/flow_ref_reader.cpp.  Nothing of the reference is committed; the
tests skip where the reference tree is absent.

What this pins and what it cannot: calculateLKOpticalFlow (the window extraction, the SSE accumulation, the float statements, the
side effects per level) and calcSharrDeriv are the reference's own code, compiled by the host compiler.  cv::pyrDown, cv::copyMakeBorder,
cvRound and cvFloor are OpenCV library behaviour, restated in the stand-in and, independently, in the checker; no OpenCV exists here to
confirm either.  The two restatements agree bytewise on every level of every scene."""
import os

import numpy as np
import pytest

import flow_checker as fc
import flow_reader as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not fr.available(), reason="needs the reference tree and g++")


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    return fr.build(tmp_path_factory.mktemp("flow_ref_reader") / "build")


@pytest.mark.parametrize("name", fc.SCENES)
def test_checker_equals_the_reader(reader, name):
    ref, chk = fr.run_scene(reader, name), fc.run_scene(name)
    assert len(ref) == len(chk)
    imgs, pts, _ = fc.scene(name)
    for k, ((nxt, status, got, L, images, derivs), (c_next, c_status, c_nt, c_pyr)) in enumerate(zip(ref, chk)):
        assert L == c_pyr.L and len(images) == L + 1
        for level in range(L + 1):
            assert images[level].tobytes() == c_pyr.image[level].tobytes(), (name, k, level)
            assert derivs[level].tobytes() == c_pyr.deriv[level].tobytes(), (name, k, level)
        assert got == c_nt
        if k == 0:
            assert nxt.tobytes() == pts.tobytes()
        else:
            bad = np.flatnonzero((nxt.view(np.uint32) != c_next.view(np.uint32)).any(axis=1) | (status != c_status))
            assert bad.size == 0, (name, k, bad[:8], nxt[bad[:8]], c_next[bad[:8]])


def test_the_reference_clamps_its_criteria_like_the_checker_assumes(reader):
    tr = fr.Tracker(reader, fc.Opts(max_count=500, epsilon=50.0))
    assert tr.criteria() == (100, 10.0)
    tr.close()
    tr = fr.Tracker(reader)
    assert tr.criteria() == (10, 0.05)           # epsilon is compared with |delta|^2 as it is: the class does not square it
    tr.close()


def test_golden_file_is_what_the_reader_produces_now(reader):
    golden = np.load(os.path.join(ROOT, "tests", "golden", "golden_flow.npz"), allow_pickle=False)
    now = fr.golden_pack(reader)
    assert sorted(golden.files) == sorted(now)
    for k, v in now.items():
        assert golden[k].dtype == np.asarray(v).dtype and np.array_equal(golden[k], v), k
    largest = max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden")) if f != "golden_flow.npz")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_flow.npz")) <= largest
