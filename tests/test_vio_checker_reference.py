"""The sequential restatement of the camera ESIKF's measurement loops (tests/vio_checker.py) pinned to the reference's own translation
units, bit for bit, and the recorded states of the updates pinned to the reader that produced them.

tests/vio_ref_reader.cpp calls cloudFrame::getRgb with gradients (on tests/stub_opencv's cv::Mat, a view of the test's image with OpenCV's
byte arithmetic), refreshPoseForProjection, numType::skewSymmetric / quatToSo3 / so3ToQuat and rgbPoint::getPosition / getRgb / getCovRgb,
writes out the loop statements of imageProcessing.cpp:308-349 and :463-518 between those calls on the stand-in Eigen of oracle/ref_shim,
and does the literal solve with the explicit K (:358-377, :525-549).  tests/vio_reader.py compiles it into the test's temporary
directory and links it to oracle/_ref/libref_path.so.  Neither the reader's binary nor anything of the reference is committed; the tests
skip where the reference tree or the library is absent.

What this pins and what it cannot: imageProcessing.cpp itself cannot be compiled here (the include mirror shadows it, there is no
OpenCV), the stand-in Eigen has no RowMajor fixed matrices, and the comparison holds the contract to the STAND-IN's evaluation order.
With real Eigen the one block whose order is not forced is J_color_pc * R_imu_camera^T (three-term sums; every other product has at
most two non-zero terms per entry): its order cannot be verified on this machine.  The pixel arithmetic is tests/stub_opencv's, whose
OpenCV semantics the known answers of tests/test_render_checker.py pin."""
import os

import numpy as np
import pytest

import vio_checker as vc
import vio_reader as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not vr.available(), reason="needs oracle/_ref/libref_path.so, the reference tree and g++")


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    return vr.build(tmp_path_factory.mktemp("vio_ref_reader") / "build")


@pytest.mark.parametrize("which", range(len(vc.SCENE_RENDERS)))
def test_rows_and_outcomes_equal_the_readers_bit_for_bit(reader, which):
    sc = vc.scene(which)
    for (mode, ext, intr), want in zip(vc.CONFIGS, vc.scene_results(which)):
        rows, outcome = vr.rows(reader, sc, mode, ext, intr)
        assert outcome.tobytes() == want.outcome.tobytes(), (which, mode, ext, intr, np.flatnonzero(outcome != want.outcome)[:8])
        assert rows.tobytes() == want.rows.tobytes(), (which, mode, ext, intr, np.argwhere(rows.view(np.uint64) != want.rows.view(np.uint64))[:8])
        assert want.counts[vc.USED] >= 10


def test_the_footprints_edges_and_every_class_through_the_reader(reader):
    sc = vc.scene(1)
    edges, designed = vc.edge_list(sc)
    pts = np.concatenate([edges, sc.points])
    for mode in (vc.PHOTOMETRIC, vc.REPROJECTION):
        want = vc.vio_rows(sc, mode, points=pts)
        rows, outcome = vr.rows(reader, sc, mode, points=pts)
        assert outcome.tobytes() == want.outcome.tobytes() and rows.tobytes() == want.rows.tobytes(), mode
    assert tuple(outcome[:0]) == () and tuple(vc.vio_rows(sc, vc.PHOTOMETRIC, points=edges).outcome) == designed


def test_the_golden_states_are_the_readers(reader):
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_color_vio.npz"), allow_pickle=False)
    for name, value in vc.golden_pack_reader(reader).items():
        assert np.asarray(g[name]).tobytes() == np.asarray(value).tobytes(), name
    for which in range(len(vc.SCENE_RENDERS)):
        for name in ("esikf", "photometric"):
            assert int(g["s%d_%s_used" % (which, name)][0]) == 1 and len(g["s%d_%s_states" % (which, name)]) >= 1


def test_the_readers_gates(reader):
    """fewer than ten tracked points: the function returns false at once; ten or more of which fewer than ten are used: the loop breaks
    at the gate, K, H_mat and `solution` are zero, and the covariance comes back as it went in"""
    sc = vc.scene(0)
    for (ok, states, cov, used) in vr.sequence(reader, 0, sc.points[:9]):
        assert not ok and len(states) == 0 and np.array_equal(cov, vc.initial_cov())
    nine = sc.points[vc.scene_results(0)[0].outcome == vc.USED][:9]
    unknown = np.zeros(3, vc.POINT_DTYPE); unknown["pool"] = -1
    a, b = vr.sequence(reader, 0, np.concatenate([nine, unknown]))
    assert a[0] and len(a[1]) == 0 and a[3] == 9 and np.array_equal(a[2], vc.initial_cov())
    assert b[0] and len(b[1]) == 0 and b[3] < 10 and np.array_equal(b[2], vc.initial_cov())
