"""The ragged-occupancy scene (tests/ragged_scene.py) on the CPU: is it the scene the GPU tests need, and does the oracle follow the
reference on it?

`threshold_voxel_occupancy` (optimize.cpp:21-23, :389) and `voxel_neighborhood` = 2 outside the init mode are inert or unused on every
other scene of the suite: synth.map_candidates() saturates its maps, so thresholds 1, 2, 5 and 12 select the same voxels there.

  * preconditions, from the oracle alone: what tests/test_gpu_option_envelope.py rests on.  They are conditions, not measurements: if a
    change to the generators made the thresholds inert again these tests fail, instead of the GPU tests going vacuous;
  * an independent NumPy count of the candidates P_k against the oracle's;
  * the oracle against golden_ref_tu_ragged.npz (the reference's own translation units, tests/golden/make_golden_ref.py), bitwise --
    this runs wherever the repository is;
  * live (where oracle/_ref/libref_path.so was built): buildPlaneResiduals, searchNeighbors and updateIEKF side by side, bitwise, over
    threshold x neighbourhood, with the default options and with those of odometryOptions::defaultRobustOutdoorLowInertia.
"""
import os

import numpy as np
import pytest

import ragged_scene as rs
from oracle import pyoracle as po
from oracle import pyref as pr
from sr_livo_amd import synth

from test_reference_tu import assert_pass_equals, live

INT_MAX = rs.INT_MAX
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = {"small": rs.SMALL, "large": rs.LARGE}


@pytest.fixture(scope="module")
def scenes(oracle_backend):
    """(name, voxel size) -> scene, built on first use"""
    cache = {}

    def get(name, voxel_size=1.0):
        if (name, voxel_size) not in cache:
            cache[name, voxel_size] = rs.ragged_scene(po, oracle_backend, *SCENES[name], voxel_size=voxel_size)
        return cache[name, voxel_size]
    return get


def _pass(sc, **kw):
    sw = sc["sweep"]
    kw.setdefault("max_num_residuals", INT_MAX)
    return sc["map"].build_plane_residuals(po.default_opts(**kw), sw["raw"], sw["q_pred"], sw["t_pred"], sw["t_last"])


def _eigen_gaps(ids, xyz):
    """(lambda_1 - lambda_0) / lambda_2 of every full neighbour row's scatter matrix (as tests/test_gpu_parity.py: eigen_gap)"""
    flat = np.asarray(xyz, np.float64).reshape(-1, 3)
    out = []
    for row in ids:
        row = row[row >= 0]
        P = flat[row]
        E = P - P.sum(0) / len(P)
        w = np.linalg.eigvalsh(E.T @ E)
        out.append((w[1] - w[0]) / max(w[2], 1e-300))
    return np.array(out)


# ----------------------------------------------------------------------------- preconditions (oracle alone)
@pytest.mark.parametrize("name", ["small", "large"])
def test_every_occupancy_from_1_to_20_is_common(scenes, name):
    h = rs.occupancy_histogram(scenes(name)["counts"])
    assert h[0] == 0.0 and abs(h.sum() - 1.0) < 1e-12
    assert h[1:].min() >= 0.01, h


@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("name", ["small", "large"])
def test_every_threshold_changes_neighbours_and_every_status_occurs(scenes, name, nb):
    sc = scenes(name)
    base = _pass(sc, voxel_neighborhood=nb)
    assert base["neq"].nan_error == 0 and base["neq"].num_visited == len(sc["sweep"]["raw"])
    for thr in (2, 5, 12, 20):
        o = _pass(sc, voxel_neighborhood=nb, threshold_voxel_occupancy=thr)
        assert o["neq"].nan_error == 0
        assert np.all(o["status"] != 3)                                       # no cut: every keypoint visited
        differs = np.any(o["ids"] != base["ids"], axis=1)
        assert differs.mean() >= 0.05, (thr, differs.mean())
        n_status = np.bincount(o["status"], minlength=3)
        if thr in (5, 12):
            assert n_status[:3].min() >= 5, (thr, n_status)
        has_plane = o["status"] >= 1
        gaps = _eigen_gaps(o["ids"][has_plane], sc["xyz"])
        assert gaps.min() > 1e-6, (thr, gaps.min())
    # at the map's capacity + 1 no voxel qualifies: nothing found, nothing accepted, a failed pass
    o = _pass(sc, voxel_neighborhood=nb, threshold_voxel_occupancy=21)
    assert np.all(o["status"] == 0) and np.all(o["ids"] == -1) and o["neq"].num_residuals == 0 and o["neq"].success == 0 and o["neq"].sum_candidates == 0


@pytest.mark.parametrize("K", [5, 20, 32])
def test_eigen_gaps_stay_clear_of_the_ill_posed_line_for_every_k(scenes, K):
    """K = 5 / 32 are run on the device too (the K / min pairs of the option envelope): no keypoint needs a well-posedness mask"""
    sc = scenes("small")
    for thr, nb in ((5, 1), (12, 2)):
        o = _pass(sc, voxel_neighborhood=nb, threshold_voxel_occupancy=thr, max_number_neighbors=K, min_number_neighbors=min(K, 20))
        assert o["neq"].nan_error == 0 and o["neq"].num_ties == 0
        assert _eigen_gaps(o["ids"][o["status"] >= 1], sc["xyz"]).min() > 1e-6


def test_nonpositive_thresholds_behave_as_one(scenes):
    """NumPoints() < threshold never holds for threshold <= 1 (optimize.cpp:389)"""
    sc = scenes("small")
    base = _pass(sc)
    for thr in (0, -3):
        o = _pass(sc, threshold_voxel_occupancy=thr)
        assert np.array_equal(o["ids"], base["ids"]) and np.array_equal(o["status"], base["status"])
        assert np.array_equal(o["HtH"], base["HtH"]) and o["neq"].sum_candidates == base["neq"].sum_candidates


def test_init_mode_ignores_threshold_and_neighbourhood(scenes):
    """frame_id < init_num_frames: threshold 1 and two layers whatever the options say (optimize.cpp:21-23)"""
    sc = scenes("small"); sw = sc["sweep"]
    outs = [sc["map"].build_plane_residuals(po.default_opts(max_num_residuals=INT_MAX, threshold_voxel_occupancy=thr, voxel_neighborhood=nb),
                                            sw["raw"], sw["q_pred"], sw["t_pred"], sw["t_last"], frame_id=5) for thr, nb in ((12, 1), (1, 2))]
    assert np.array_equal(outs[0]["ids"], outs[1]["ids"]) and np.array_equal(outs[0]["HtH"], outs[1]["HtH"])
    assert outs[0]["neq"].sum_candidates == outs[1]["neq"].sum_candidates


# ----------------------------------------------------------------------------- the NumPy candidate count
@pytest.mark.parametrize("size", [1.0, 0.8])
def test_numpy_candidate_count_equals_the_oracles(scenes, size):
    """ragged_scene.candidate_counts is what the GPU tests hold the device's per-keypoint P_k against: per point against the oracle's
    searchNeighbors, and as a sum against buildPlaneResiduals"""
    sc = scenes("small", size)
    o = _pass(sc, size_voxel_map=size)
    world = o["point_world"]
    for thr, nb in ((1, 1), (5, 1), (12, 2), (20, 2), (21, 1)):
        want = rs.candidate_counts(sc["keys"], sc["counts"], world, size, nb, thr)
        o = _pass(sc, size_voxel_map=size, threshold_voxel_occupancy=thr, voxel_neighborhood=nb)
        assert int(want.sum()) == o["neq"].sum_candidates
        got = np.array([sc["map"].search_neighbors(p, nb=nb, size=size, K=20, thr=thr)["num_candidates"] for p in world[:300]])
        assert np.array_equal(got, want[:300])
    assert np.array_equal(rs.candidate_counts(sc["keys"], sc["counts"], world, size, 1, 0), rs.candidate_counts(sc["keys"], sc["counts"], world, size, 1, 1))


# ----------------------------------------------------------------------------- golden of the reference's translation units
@pytest.fixture(scope="module")
def gragged():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "golden_ref_tu_ragged.npz"), allow_pickle=False))


RAGGED_GOLDEN_CASES = [("t5n1", "map", dict(threshold_voxel_occupancy=5, voxel_neighborhood=1, max_num_residuals=INT_MAX)),
                       ("t12n2", "map", dict(threshold_voxel_occupancy=12, voxel_neighborhood=2, max_num_residuals=INT_MAX)),
                       ("lowinertia", "map08", rs.LOW_INERTIA)]


@pytest.mark.parametrize("prefix,which,kw", RAGGED_GOLDEN_CASES)
def test_oracle_reproduces_the_ragged_reference_golden_bitwise(gragged, oracle_backend, prefix, which, kw):
    g = gragged
    m = po.Map(oracle_backend)
    m.import_(g[f"{which}_keys"], g[f"{which}_counts"], g[f"{which}_xyz"])
    o = m.build_plane_residuals(po.default_opts(**kw), g["raw"], g["q_pred"], g["t_pred"], g["t_last"])
    r = {k[len(prefix) + 5:]: v for k, v in g.items() if k.startswith(prefix + "_ref_")}
    r["success"] = int(r["success"]); r["num_residuals"] = int(r["num_residuals"]); r["loss"] = float(r["loss"])
    assert_pass_equals(o, r)
    assert np.array_equal(g["raw"][o["status"] == 2], r["location"])
    assert r["num_residuals"] >= 500                                      # a case that accepts nothing would pin nothing


def test_the_ragged_golden_is_the_ragged_scene(gragged, oracle_backend):
    """the committed map is what the generator gives today: the fixture and the live scene cannot drift apart unnoticed"""
    for which, size in (("map", 1.0), ("map08", 0.8)):
        sc = rs.ragged_scene(po, oracle_backend, rs.SMALL[0], rs.SMALL[1], len(gragged["raw"]), voxel_size=size)
        assert np.array_equal(sc["keys"], gragged[f"{which}_keys"]) and np.array_equal(sc["counts"], gragged[f"{which}_counts"])
        assert np.array_equal(sc["xyz"], gragged[f"{which}_xyz"])
    assert np.array_equal(sc["sweep"]["raw"], gragged["raw"])


# ----------------------------------------------------------------------------- live: oracle and reference side by side
@live
@pytest.mark.parametrize("profile", ["default", "low_inertia"])
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("thr", [1, 2, 5, 12, 20, 21])
def test_ragged_build_plane_residuals_bitwise(scenes, thr, nb, profile):
    kw = dict(max_num_residuals=INT_MAX) if profile == "default" else dict(rs.LOW_INERTIA)
    kw.update(threshold_voxel_occupancy=thr, voxel_neighborhood=nb)
    for name in ("small", "large"):
        sc = scenes(name, kw.get("size_voxel_map", 1.0)); sw = sc["sweep"]
        rm = pr.Map.from_oracle(sc["map"])
        opts = po.default_opts(**kw)
        o = sc["map"].build_plane_residuals(opts, sw["raw"], sw["q_pred"], sw["t_pred"], sw["t_last"])
        r = rm.build_plane_residuals(opts, sw["raw"], sw["q_pred"], sw["t_pred"], sw["t_last"])
        assert_pass_equals(o, r)
        assert o["neq"].num_residuals == 0 if thr == 21 else (o["neq"].num_residuals > 0 or profile != "default")


@live
@pytest.mark.parametrize("K", [5, 20, 32])
@pytest.mark.parametrize("nb", [1, 2])
def test_ragged_search_neighbors_bitwise(scenes, nb, K):
    sc = scenes("small")
    rm = pr.Map.from_oracle(sc["map"])
    flat = sc["xyz"].reshape(-1, 3)
    world = _pass(sc)["point_world"][:256]
    short = 0
    for thr in (0, 1, 5, 20, 21):
        for p in world:
            o = sc["map"].search_neighbors(p, nb=nb, K=K, thr=thr)
            r = rm.search_neighbors(p, nb=nb, K=K, thr=thr)
            assert o["n"] == r["n"]
            assert np.array_equal(flat[o["ids"]].astype(np.float64), r["xyz"])
            assert np.array_equal(sc["keys"][o["ids"] // 20], r["voxels"])
            assert np.all(sc["counts"][o["ids"] // 20] >= thr)                # only qualifying voxels were read
            short += int(0 < o["n"] < K)
            assert thr != 21 or o["n"] == 0
    assert short > 0 or K == 5                                                # some neighbourhoods hold fewer than K qualifying points


@live
@pytest.mark.parametrize("kw", [dict(threshold_voxel_occupancy=5, voxel_neighborhood=1, max_num_residuals=INT_MAX),
                                dict(threshold_voxel_occupancy=5, voxel_neighborhood=2, max_num_residuals=INT_MAX), rs.LOW_INERTIA],
                         ids=["thr5-nb1", "thr5-nb2", "low_inertia"])
def test_ragged_update_iekf_bitwise(scenes, oracle_backend, kw):
    sc = scenes("small", kw.get("size_voxel_map", 1.0)); sw = sc["sweep"]
    rm = pr.Map.from_oracle(sc["map"])
    opts = po.default_opts(**kw)
    e = po.Eskf(oracle_backend); synth.eskf_prior(e, sw["q_pred"], sw["t_pred"], sw["vel"])
    re_ = pr.Eskf(); re_.set_state(e.get_state()); re_.set_cov(e.get_cov())
    st = np.concatenate([sw["q_pred"], sw["t_pred"], sw["vel"], np.zeros(6)])
    u = po.update_iekf(sc["map"], e, opts, sw["raw"], st, sw["t_last"])
    r = pr.update_iekf(rm, re_, opts, sw["raw"], st, sw["t_last"])
    assert u["rc"] > 1 and r["rc"] == 1 and u["num_residuals"] == r["num_residuals"] > 0
    assert np.array_equal(u["state"], r["state"])
    assert np.array_equal(e.get_state(), re_.get_state()) and np.array_equal(e.get_cov(), re_.get_cov())
