"""The checker of the insertion report (tests/cloud_checker.py) tied to the reference's own addPointToMap: its one-at-a-time
classification through the oracle equals the same classification through the reference's translation units (pyref.Node: the node's
addPointsToMap and its voxel count), and inserting one at a time builds the map a whole-batch insertion builds."""
import numpy as np
import pytest

import cloud_checker as cc
from oracle import pyref as pr
from sr_livo_amd import synth

pytestmark = pytest.mark.skipif(not pr.available(), reason="oracle/_ref/libref_path.so not built (needs the reference tree at build time)")


class _NodeMap:
    """the reference node's voxel_map behind the two calls the checker uses"""

    def __init__(self, node):
        self.node = node

    def add_points(self, xyz, voxel_size, cap, min_dist, min_num_points):
        return self.node.add_points_to_map(xyz, voxel_size, cap, min_dist, min_num_points)

    def num_voxels(self):
        return int(self.node.lib.ref_node_map_num_voxels(self.node.h))


def _scene(seed, n):
    """a seeded room scan, shuffled so that the points of a voxel are spread over the batch, with near-duplicates that the
    min-distance test rejects"""
    pts, _ = synth.map_candidates(seed, n)
    rng = np.random.default_rng(seed)
    pts = pts[rng.permutation(len(pts))][:n]
    dup = pts[rng.integers(0, len(pts), len(pts) // 8)] + rng.normal(0.0, 0.02, (len(pts) // 8, 3))
    pts = np.concatenate([pts, dup])
    return pts[rng.permutation(len(pts))]


@pytest.mark.parametrize("min_num_points", [0, 3])
def test_checker_equals_the_reference_node(oracle_lib, oracle_backend, min_num_points):
    base, batch = _scene(5101, 3000), _scene(5102, 3000)
    kw = dict(voxel_size=0.5, cap=20, min_dist=0.1)
    om, node = oracle_lib.Map(oracle_backend), pr.Node(True)
    try:
        om.add_points(base, min_num_points=0, **kw)                      # a map to append to (min_num_points 3 creates nothing)
        node.add_points_to_map(base, min_num_points=0, **kw)
        mine = cc.classify(om, batch, min_num_points=min_num_points, **kw)
        theirs = cc.classify(_NodeMap(node), batch, min_num_points=min_num_points, **kw)
        assert np.array_equal(mine, theirs)
        assert (mine == 0).any() and (mine == 1).any() and ((mine == 2).any() or min_num_points > 0)
        if min_num_points > 0:
            assert not (mine == 2).any()
        # one at a time == the whole batch at once, on both sides
        whole = oracle_lib.Map(oracle_backend)
        whole.add_points(base, min_num_points=0, **kw)
        assert whole.add_points(batch, min_num_points=min_num_points, **kw) == int((mine != 0).sum())
        a, b, c = pr.map_as_dict(*om.export()), pr.map_as_dict(*whole.export()), pr.map_as_dict(*node.map_export())
        assert a.keys() == b.keys() == c.keys()
        for k in a:
            assert np.array_equal(cc.bits(a[k]), cc.bits(b[k])) and np.array_equal(cc.bits(a[k]), cc.bits(c[k]))
        assert np.array_equal(om.export()[0], whole.export()[0])          # same creation order
    finally:
        node.close()
